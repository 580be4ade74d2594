// train.hip -- the training path of the GausPcgc context network (network_ue_4stage_conv.py:100-182 with gradients).
//
// gpcc_train_frame    the encoder's octree and its ONE tile pool (prior set = levels 0..L-2, target set = levels 1..L-1), built in
//                     the workspace arena and copied into caller memory, plus a per-(block, offset) run index of each set's tiles.
// gpcc_train_weights  (K, 32, 32) device weights -> the fragment layouts k_sparse_conv reads (the host loops of gpcc_model_create as a
//                     kernel); mirror = 1 gives the dgrad weights W'[o] = W[K-1-o]^T.
// gpcc_train_conv     one convolution over a set with those fragments: the codec's sparse_conv, unchanged.  The input gradient of a
//                     stride-1 submanifold convolution is the same kernel on the same tile lists with the mirrored weights (the
//                     neighbour relation is symmetric: j = i + d_o  <=>  i = j + d_{K-1-o}).
// gpcc_train_wgrad    dW[o] = sum over the (i, j) pairs of offset o of X[j]^T dY[i]: one wave per (offset, fixed group of consecutive
//                     blocks) walks the group's runs of that offset on v_mfma_f32_32x32x2_f32 and writes one 32x32 partial; a second
//                     pass adds the partials of each offset in group order.  The group size is a function of the set's block count and
//                     K only, and nothing is added atomically: the gradient is bitwise reproducible on every machine and stream.
// Rows are in the library's physical channel order (network.hpp); weights and weight gradients in the upstream logical layout.
#include <algorithm>

#include "codec_shared.hpp"
#include "network_dev.hpp"

using namespace gpcc;

namespace {

constexpr uint32_t FRAME_MAGIC = 0x31465447u;   // "GTF1"
constexpr int WGRAD_WAVES_TARGET = 8192;        // (offset, group) waves of one wgrad launch the group size aims at

struct TrainFrame {
    uint32_t magic;
    int k, K, L;
    int64_t npts, nodes, nP, nC;
    int64_t level_nodes[MAXLV];
    int64_t level_base[MAXLV + 1];   // first node of each level in the all-levels arrays (levels 0..L-2 = the prior set's rows)
    ConvTiles set[2];                // 0: prior set, 1: target set
    const uint32_t *runs[2];         // [set block][K + 1]: first tile of offset o in the block's list; [K] = end of the list
    int64_t group[2];                // wgrad: blocks per group
    uint8_t *occ;                    // (nodes)
    int32_t *coords;                 // (nodes, 3), un-biased
    int32_t *parent;                 // (nC) row of the parent in the prior set
    uint8_t *octant;                 // (nC)
};
static_assert(sizeof(TrainFrame) <= 8 * GPCC_TRAIN_STATE_WORDS, "the frame record must fit the caller's state words");

struct FrameNodes {
    int L;
    int64_t base[MAXLV + 1];
    int64_t bias[MAXLV][3];
    const uint8_t *occ[MAXLV];
    const uint64_t *rkey[MAXLV];
    const uint32_t *parent[MAXLV];
};

__global__ __launch_bounds__(256) void k_frame_nodes(FrameNodes S, uint8_t *__restrict__ occ, int32_t *__restrict__ xyz, int32_t *__restrict__ parent,
                                                     uint8_t *__restrict__ octant)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= S.base[S.L]) return;
    int d = 0;
    for (int q = 1; q < S.L; ++q) d = g >= S.base[q] ? q : d;
    const int64_t j = g - S.base[d];
    const uint64_t k = S.rkey[d][j];
    occ[g] = S.occ[d][j];
    xyz[3 * g] = (int32_t)((int64_t)rk_x(k) - S.bias[d][0]);
    xyz[3 * g + 1] = (int32_t)((int64_t)rk_y(k) - S.bias[d][1]);
    xyz[3 * g + 2] = (int32_t)((int64_t)rk_z(k) - S.bias[d][2]);
    if (d >= 1) {
        const int64_t i = g - S.base[1];
        parent[i] = (int32_t)(S.base[d - 1] + S.parent[d][j]);
        octant[i] = (uint8_t)((rk_x(k) & 1) | ((rk_y(k) & 1) << 1) | ((rk_z(k) & 1) << 2));
    }
}

// runs[s][o] = first tile of the set's block s whose offset is >= o (the tiles of a block are grouped by offset, ascending; the
// padding tile of a paired run carries the run's offset)
__global__ __launch_bounds__(256) void k_run_index(ConvTiles T, uint32_t *__restrict__ runs)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int K1 = T.K + 1;
    if (t >= T.nblk * K1) return;
    const int64_t s = t / K1;
    const uint32_t o = (uint32_t)(t % K1);
    const uint32_t blk = T.lv_blk0[0] + (uint32_t)s;
    uint32_t lo = T.first[blk], hi = T.first[blk + 1];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((T.toc[mid] & 0xFFFFu) < o) lo = mid + 1;
        else hi = mid;
    }
    runs[t] = lo;
}

// [o][half][q][lane][r] of conv_weight_fragments, then of conv_weight_fragments_t (network.hpp), from the device kernel W (K, 32, 32);
// mirror: the source is W'[o] = W[K-1-o]^T
__global__ __launch_bounds__(256) void k_train_frags(const float *__restrict__ W, int K, int mirror, float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)K * 2048) return;
    const int tr = t >= (int64_t)K * 1024;
    const int64_t u = t - (tr ? (int64_t)K * 1024 : 0);
    const int r = (int)(u & 3), lane = (int)((u >> 2) & 63), q = (int)((u >> 8) & 1), hh = (int)((u >> 9) & 1);
    const int o = (int)(u >> 10);
    const int m = lane & 15;
    const int kk = 4 * (4 * q + r) + (lane >> 4);
    const int nn = 16 * hh + (tr ? 4 * (m & 3) + (m >> 2) : m);
    out[t] = mirror ? W[((size_t)(K - 1 - o) * 32 + nn) * 32 + kk] : W[((size_t)o * 32 + kk) * 32 + nn];
}

struct WgradArgs {
    ConvTiles T;
    const uint32_t *runs;
    const float *x, *dy;
    float *part;
    int64_t G;
    int ngroups;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// one wave per (offset o, group g): partial[o][g] = sum over the group's blocks, tiles and entries (in that order) of X[j] (x) dY[i],
// rows and columns in the physical channel order.  A tile's 16 pairs are 8 k-steps of the 32x32x2 MFMA: lane l supplies pair 2 q + l / 32
// -- column l % 32 of the neighbour row (A) and of the output row's gradient (B).
__global__ __launch_bounds__(256) void k_wgrad_part(WgradArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const ConvTiles &T = a.T;
    const int K = T.K;
    if (w >= K * a.ngroups) return;
    const int o = w / a.ngroups, g = w % a.ngroups;
    const int64_t s0 = (int64_t)g * a.G, s1 = s0 + a.G < T.nblk ? s0 + a.G : T.nblk;
    const int c = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int64_t s = s0; s < s1; ++s) {
        const uint32_t t0 = a.runs[s * (K + 1) + o], t1 = a.runs[s * (K + 1) + o + 1];
        if (t0 == t1) continue;
        const int blk = (int)T.lv_blk0[0] + (int)s;
        int lvi = 0;
        for (int i = 1; i < T.nlv; ++i) lvi = blk >= (int)T.lv_blk0[i] ? i : lvi;
        const int64_t row0 = (int64_t)T.lv_row0[lvi] + (int64_t)(blk - (int)T.lv_blk0[lvi]) * T.H;   // set row of the block's slot 1
        const float *xl = a.x + (size_t)T.lv_row0[lvi] * 32 + c;
        const float *yl = a.dy + (size_t)row0 * 32 + c;
        for (uint32_t t = t0; t < t1; ++t) {
            float xa[8], yb[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = 2 * q + h;
                const int j = T.tj[(size_t)t * 16 + e];
                const int sl = T.tr[(size_t)t * 16 + e];   // 0: padding (the dummy slot)
                const float xv = xl[(size_t)j * 32];
                const float yv = yl[(size_t)(sl ? sl - 1 : 0) * 32];
                xa[q] = sl ? xv : 0.f;
                yb[q] = sl ? yv : 0.f;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q], yb[q], acc, 0, 0, 0);
        }
    }
    float *p = a.part + ((size_t)o * a.ngroups + g) * 1024;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + c] = acc[r];
}

// dW[o][logical a][logical b] = sum over g ascending of partial[o][g][phys a][phys b]
__global__ __launch_bounds__(256) void k_wgrad_sum(const float *__restrict__ part, int K, int ngroups, float *__restrict__ dw)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)K * 1024) return;
    const int o = (int)(t >> 10), idx = (int)(t & 1023);
    const float *p = part + (size_t)o * ngroups * 1024 + idx;
    float s = 0.f;
    for (int g = 0; g < ngroups; ++g) s += p[(size_t)g * 1024];
    dw[((size_t)o * 32 + logical_of(idx >> 5)) * 32 + logical_of(idx & 31)] = s;
}

int frame_get(const uint64_t *state, TrainFrame *F)
{
    if (!state) return fail(GPCC_ERR_ARG, "null frame state");
    memcpy(F, state, sizeof(TrainFrame));
    if (F->magic != FRAME_MAGIC) return fail(GPCC_ERR_ARG, "not a training frame (gpcc_train_frame)");
    return GPCC_OK;
}

int frame_set(const TrainFrame &F, int set, int64_t *rows)
{
    if (set != 0 && set != 1) return fail(GPCC_ERR_ARG, "set must be 0 (prior) or 1 (target)");
    *rows = set ? F.nC : F.nP;
    return GPCC_OK;
}

int frame_body(gpcc_ctx *ctx, hipStream_t st, const int32_t *xyz, int64_t n, int k, gsr_alloc_fn alloc, void *user, TrainFrame *F, bool *alloc_failed)
{
    ctx->arena.reset();
    Tree T;
    GP_TRY(tree_build(ctx, st, xyz, n, &T));
    const int L = T.L;
    F->magic = FRAME_MAGIC; F->k = k; F->K = k * k * k; F->L = L; F->npts = n;
    int64_t nodes = 0;
    for (int d = 0; d < L; ++d) { F->level_nodes[d] = T.lv[d].n; F->level_base[d] = nodes; nodes += T.lv[d].n; }
    F->level_base[L] = nodes;
    F->nodes = nodes;
    F->nP = L > 1 ? F->level_base[L - 1] : 0;
    F->nC = L > 1 ? nodes - T.lv[0].n : 0;
    TilePool pool;
    uint32_t total = 0;
    if (L > 1) {
        GP_TRY(tile_sets(ctx, st, T, nullptr, nullptr, k, nullptr, &pool, &F->set[0], &F->set[1]));
        HIP_TRY(hipMemcpyAsync(&total, pool.first + pool.nblk, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // caller memory: the pool (tiles + CONV_HDR_PAD zeroed ones the conv kernel may read past a list), block ranges, pair flags,
    // the two dispatch orders and run indexes, the per-node arrays
    const int64_t ntile = L > 1 ? (int64_t)total + CONV_HDR_PAD : 0;
    const int64_t npflag = pool.pflag ? pool.nblk : 0;
    int32_t *tj;
    uint8_t *tr, *pflag;
    uint32_t *toc, *first, *order[2], *runs[2];
    const int rc = caller_block(alloc, user, "gpcc_train_frame", [&](Carver &c) {
        tj = c.take<int32_t>(16 * ntile); tr = c.take<uint8_t>(16 * ntile); toc = c.take<uint32_t>(ntile); first = c.take<uint32_t>(pool.nblk + 1);
        pflag = c.take<uint8_t>(npflag);
        for (int s = 0; s < 2; ++s) order[s] = c.take<uint32_t>(F->set[s].nblk);
        for (int s = 0; s < 2; ++s) runs[s] = c.take<uint32_t>(F->set[s].nblk * (F->K + 1));
        F->occ = c.take<uint8_t>(nodes); F->coords = c.take<int32_t>(3 * nodes); F->parent = c.take<int32_t>(F->nC); F->octant = c.take<uint8_t>(F->nC);
    });
    if (rc != GPCC_OK) { *alloc_failed = true; return rc; }
    if (L > 1) {
        HIP_TRY(hipMemcpyAsync(tj, pool.tj, 64 * (size_t)ntile, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(tr, pool.tr, 16 * (size_t)ntile, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(toc, pool.toc, 4 * (size_t)ntile, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(first, pool.first, 4 * (size_t)(pool.nblk + 1), hipMemcpyDeviceToDevice, st));
        if (npflag) HIP_TRY(hipMemcpyAsync(pflag, pool.pflag, (size_t)npflag, hipMemcpyDeviceToDevice, st));
        for (int s = 0; s < 2; ++s) {
            ConvTiles &V = F->set[s];
            HIP_TRY(hipMemcpyAsync(order[s], V.order, 4 * (size_t)V.nblk, hipMemcpyDeviceToDevice, st));
            V.tj = tj; V.tr = tr; V.toc = toc; V.first = first; V.pflag = npflag ? pflag : nullptr; V.order = order[s];
            F->runs[s] = runs[s];
            k_run_index<<<(unsigned)cdiv(V.nblk * (F->K + 1), 256), 256, 0, st>>>(V, runs[s]);
            LAUNCH_CHECK();
            const int64_t ng = std::max<int64_t>(1, std::min<int64_t>(V.nblk, cdiv(WGRAD_WAVES_TARGET, F->K)));
            F->group[s] = std::max<int64_t>(1, cdiv(V.nblk, ng));
        }
    }
    FrameNodes S = {};
    S.L = L;
    for (int d = 0; d <= L; ++d) S.base[d] = F->level_base[d];
    for (int d = 0; d < L; ++d) {
        for (int a = 0; a < 3; ++a) S.bias[d][a] = T.bias[a] >> T.lv[d].lvl;   // a multiple of 2^L: the shift is exact
        S.occ[d] = T.lv[d].occ; S.rkey[d] = T.lv[d].rkey; S.parent[d] = T.lv[d].parent;
    }
    k_frame_nodes<<<(unsigned)cdiv(nodes, 256), 256, 0, st>>>(S, F->occ, F->coords, F->parent, F->octant);
    LAUNCH_CHECK();
    // the copies read the arena: the next call on this context (on any stream) may reuse it only after they have run
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}

}  // namespace

extern "C" int gpcc_train_frame(gpcc_ctx *ctx, const int32_t *xyz_dev, int64_t n, int kernel_size, gsr_alloc_fn alloc, void *alloc_user, uint64_t *state,
                                int32_t *levels_out, int64_t *level_nodes_out, void *stream)
{
    if (!ctx || !xyz_dev || !alloc || !state) return fail(GPCC_ERR_ARG, "null argument");
    if (n < 1) return fail(GPCC_ERR_ARG, "empty cloud");
    if (kernel_size != 3 && kernel_size != 5 && kernel_size != 7) return fail(GPCC_ERR_ARG, "kernel_size must be 3, 5 or 7");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int K = kernel_size * kernel_size * kernel_size;
    size_t want = arena_estimate(n, K);
    TrainFrame F = {};
    int rc = GPCC_OK;
    for (int attempt = 0; attempt < 6; ++attempt) {
        GP_TRY(ctx->arena.reserve(want));
        F = TrainFrame{};
        bool alloc_failed = false;
        rc = frame_body(ctx, st, xyz_dev, n, kernel_size, alloc, alloc_user, &F, &alloc_failed);
        if (rc != GPCC_ERR_NOMEM || alloc_failed) break;   // the arena was too small: grow it; the caller's allocator is not asked twice
        HIP_TRY(hipStreamSynchronize(st));
        want *= 2;
    }
    if (const int de = device_error_check(ctx)) rc = de;
    if (rc != GPCC_OK) return rc;
    memset(state, 0, 8 * GPCC_TRAIN_STATE_WORDS);
    memcpy(state, &F, sizeof F);
    if (levels_out) *levels_out = F.L;
    if (level_nodes_out) for (int d = 0; d < 24; ++d) level_nodes_out[d] = d < F.L ? F.level_nodes[d] : 0;
    return GPCC_OK;
}

extern "C" int gpcc_train_frame_nodes(gpcc_ctx *ctx, const uint64_t *state, uint8_t *occ_dev, int32_t *parent_dev, uint8_t *octant_dev, int32_t *coords_dev, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "null argument");
    TrainFrame F;
    GP_TRY(frame_get(state, &F));
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (occ_dev && F.nodes) HIP_TRY(hipMemcpyAsync(occ_dev, F.occ, (size_t)F.nodes, hipMemcpyDeviceToDevice, st));
    if (coords_dev && F.nodes) HIP_TRY(hipMemcpyAsync(coords_dev, F.coords, (size_t)F.nodes * 12, hipMemcpyDeviceToDevice, st));
    if (parent_dev && F.nC) HIP_TRY(hipMemcpyAsync(parent_dev, F.parent, (size_t)F.nC * 4, hipMemcpyDeviceToDevice, st));
    if (octant_dev && F.nC) HIP_TRY(hipMemcpyAsync(octant_dev, F.octant, (size_t)F.nC, hipMemcpyDeviceToDevice, st));
    return GPCC_OK;
}

extern "C" int gpcc_train_weights(gpcc_ctx *ctx, const float *w_dev, int channels, int kernel_size, int mirror, float *frag_dev, void *stream)
{
    if (!ctx || !w_dev || !frag_dev) return fail(GPCC_ERR_ARG, "null argument");
    if (channels != 32) return fail(GPCC_ERR_ARG, "the training path runs 32 channels (got %d)", channels);
    if (kernel_size != 3 && kernel_size != 5 && kernel_size != 7) return fail(GPCC_ERR_ARG, "kernel_size must be 3, 5 or 7");
    HIP_TRY(hipSetDevice(ctx->device));
    const int K = kernel_size * kernel_size * kernel_size;
    k_train_frags<<<(unsigned)cdiv((int64_t)K * 2048, 256), 256, 0, (hipStream_t)stream>>>(w_dev, K, mirror ? 1 : 0, frag_dev);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gpcc_train_conv(gpcc_ctx *ctx, const uint64_t *state, int set, const float *in_dev, const float *frag_dev, const float *res_dev, int relu,
                               float *out_dev, void *stream)
{
    if (!ctx || !in_dev || !frag_dev || !out_dev) return fail(GPCC_ERR_ARG, "null argument");
    TrainFrame F;
    GP_TRY(frame_get(state, &F));
    int64_t rows = 0;
    GP_TRY(frame_set(F, set, &rows));
    if (rows == 0) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    ConvBatch cb = {};
    cb.C = 32;
    cb.job[0] = ConvJob{in_dev, frag_dev, res_dev, out_dev};
    return sparse_conv(ctx, -1, (hipStream_t)stream, cb, 1, F.set[set], rows, relu ? 1 : 0);
}

extern "C" int gpcc_train_wgrad(gpcc_ctx *ctx, const uint64_t *state, int set, const float *x_dev, const float *dy_dev, gsr_alloc_fn alloc, void *alloc_user,
                                float *grad_w_dev, void *stream)
{
    if (!ctx || !x_dev || !dy_dev || !alloc || !grad_w_dev) return fail(GPCC_ERR_ARG, "null argument");
    TrainFrame F;
    GP_TRY(frame_get(state, &F));
    int64_t rows = 0;
    GP_TRY(frame_set(F, set, &rows));
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        HIP_TRY(hipMemsetAsync(grad_w_dev, 0, (size_t)F.K * 4096, st));
        return GPCC_OK;
    }
    const ConvTiles &T = F.set[set];
    const int64_t G = F.group[set];
    const int ng = (int)cdiv(T.nblk, G);
    float *part;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)F.K * ng * 4096, &part, "gpcc_train_wgrad"));
    WgradArgs a = {T, F.runs[set], x_dev, dy_dev, part, G, ng};
    k_wgrad_part<<<(unsigned)cdiv((int64_t)F.K * ng, 4), 256, 0, st>>>(a);
    LAUNCH_CHECK();
    k_wgrad_sum<<<(unsigned)cdiv((int64_t)F.K * 1024, 256), 256, 0, st>>>(part, F.K, ng, grad_w_dev);
    LAUNCH_CHECK();
    return GPCC_OK;
}
