// knn.hip -- exact k-nearest-neighbour search over a float32 point cloud:
//   gpcc_knn  simple_knn._C.distCUDA2   simple-knn.zip!simple-knn/spatial.cu:16-23, simple_knn.cu:185-219 (k = 3, the mean)
//             sklearn NearestNeighbors(n_neighbors=K).kneighbors(X) on its fit data   TC-GS/scene/gaussian_model.py:1052-1059
// The contract (include/gauspcc.h): d(i, j) = (dx*dx + dy*dy) + dz*dz with dx = p_j.x - p_i.x in float32 without contraction (the
// library builds with -ffp-contract=off); L_i = the k smallest (d, j) over j != i in lexicographic order, pairs with d > FLT_MAX left
// out, padded with (FLT_MAX, -1); mean = the sequential float32 sum of L_i's distances / (float)k.
//
// Pipeline, all on the caller's stream:
//   k_bbox / k_bbox_final  the cloud's float box and a non-finite flag (read back: the call's only synchronisation)
//   k_keys                 63-bit Morton keys (21 bits per axis over the box), sorted by the stable radix_sort_u64
//   k_gather               the points in key order as float4 (x, y, z, original index)
//   k_node_box             leaves = 64 consecutive sorted points (one wave's worth); an implicit 64-ary tree of boxes above them,
//                          each box with the smallest original index below it
//   k_knn_search           one wave per leaf, one query per lane: seed from the own leaf, then a nearest-first walk of the tree
//                          with a wave-uniform stack; a visited leaf's points are broadcast to every lane and inserted branch-free
// The keys only order the points: quantisation never changes a result, only how many leaves a wave visits.
#include "primitives.hpp"

#include <algorithm>
#include <float.h>
#include <limits.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int LEAF = 64;                 // points per leaf = children per node = lanes per wave
constexpr int KNN_MAX_K = 16;
constexpr int MAX_LEVELS = 6;            // n < 2^31: 2^25 leaves, then 2^19, 2^13, 2^7, 2, 1 nodes
constexpr int STACK = 1 + (MAX_LEVELS - 1) * (LEAF - 1);   // a pop removes one entry and pushes at most 64
constexpr int BB_MAX_BLOCKS = 1024;
constexpr int LVL_SHIFT = 29;            // stack entry = level << 29 | node (node < 2^25)

struct Levels {
    int levels;                          // level 0 = leaves, levels - 1 = the root (one node)
    int off[MAX_LEVELS];                 // first box of a level in the box array
    int cnt[MAX_LEVELS];                 // nodes of a level
};

// ------------------------------------------------------------------ bounding box and non-finite flag
// min / max do not depend on the order of the reduction, so partial boxes per block and one final block give the same box every run
__global__ __launch_bounds__(TB) void k_bbox(const float *__restrict__ xyz, int64_t n, float *__restrict__ part)
{
    __shared__ float s[6][TB];
    __shared__ uint32_t sbad[TB];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * i + a];
            bad |= isfinite(v) ? 0u : 1u;
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
    for (int a = 0; a < 3; ++a) { s[a][threadIdx.x] = lo[a]; s[3 + a][threadIdx.x] = hi[a]; }
    sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fminf(s[a][threadIdx.x], s[a][threadIdx.x + w]);
                s[3 + a][threadIdx.x] = fmaxf(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + w]);
            }
            sbad[threadIdx.x] |= sbad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[8 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
    if (threadIdx.x == 6) part[8 * blockIdx.x + 6] = __uint_as_float(sbad[0]);
}

// box[0..2] = lo, box[3..5] = hi, box[6] = the flag's bits (non-zero: a coordinate is NaN or +-inf)
__global__ __launch_bounds__(TB) void k_bbox_final(const float *__restrict__ part, int nb, float *__restrict__ box)
{
    __shared__ float s[6][TB];
    __shared__ uint32_t sbad[TB];
    float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    uint32_t bad = 0;
    for (int b = threadIdx.x; b < nb; b += TB) {
        for (int a = 0; a < 3; ++a) { v[a] = fminf(v[a], part[8 * b + a]); v[3 + a] = fmaxf(v[3 + a], part[8 * b + 3 + a]); }
        bad |= __float_as_uint(part[8 * b + 6]);
    }
    for (int a = 0; a < 6; ++a) s[a][threadIdx.x] = v[a];
    sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fminf(s[a][threadIdx.x], s[a][threadIdx.x + w]);
                s[3 + a][threadIdx.x] = fmaxf(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + w]);
            }
            sbad[threadIdx.x] |= sbad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) box[threadIdx.x] = s[threadIdx.x][0];
    if (threadIdx.x == 6) box[6] = __uint_as_float(sbad[0]);
}

// ------------------------------------------------------------------ Morton keys, gather
__device__ __forceinline__ uint64_t spread21(uint64_t x)
{
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// quantised in double (an extent of up to 2 FLT_MAX stays finite); an axis of zero extent maps to 0
__device__ __forceinline__ uint64_t quant21(float v, float lo, float hi)
{
    const double ext = (double)hi - (double)lo;
    if (!(ext > 0.0)) return 0;
    const double t = ((double)v - (double)lo) / ext * 2097151.0;
    return t >= 2097151.0 ? 2097151ull : (uint64_t)t;
}

__global__ __launch_bounds__(TB) void k_keys(const float *__restrict__ xyz, int64_t n, const float *__restrict__ box, uint64_t *__restrict__ key,
                                             uint32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint64_t qx = quant21(xyz[3 * i], box[0], box[3]), qy = quant21(xyz[3 * i + 1], box[1], box[4]), qz = quant21(xyz[3 * i + 2], box[2], box[5]);
    key[i] = spread21(qx) | spread21(qy) << 1 | spread21(qz) << 2;
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(TB) void k_gather(const float *__restrict__ xyz, const uint32_t *__restrict__ order, int64_t n, float4 *__restrict__ pts)
{
    const int64_t s = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = order[s];
    pts[s] = make_float4(xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1], xyz[3 * (int64_t)i + 2], __int_as_float((int)i));
}

// ------------------------------------------------------------------ the tree
// node box = (lo.x, lo.y, lo.z, smallest original index as bits), (hi.x, hi.y, hi.z, 0); one wave per node, four nodes per block.
// pts != nullptr: the children are points (the leaves); otherwise boxes of the level below.
__global__ __launch_bounds__(TB) void k_node_box(const float4 *__restrict__ pts, const float4 *__restrict__ child, int nchild, int nnodes,
                                                 float4 *__restrict__ out)
{
    const int node = blockIdx.x * (TB / LEAF) + (int)(threadIdx.x / LEAF), lane = threadIdx.x % LEAF;
    if (node >= nnodes) return;
    const int c = node * LEAF + lane;
    float lx = FLT_MAX, ly = FLT_MAX, lz = FLT_MAX, hx = -FLT_MAX, hy = -FLT_MAX, hz = -FLT_MAX;
    int mi = INT_MAX;
    if (c < nchild) {
        if (pts) {
            const float4 p = pts[c];
            lx = hx = p.x; ly = hy = p.y; lz = hz = p.z; mi = __float_as_int(p.w);
        } else {
            const float4 a = child[2 * c], b = child[2 * c + 1];
            lx = a.x; ly = a.y; lz = a.z; mi = __float_as_int(a.w); hx = b.x; hy = b.y; hz = b.z;
        }
    }
    for (int m = LEAF / 2; m > 0; m >>= 1) {
        lx = fminf(lx, __shfl_xor(lx, m)); ly = fminf(ly, __shfl_xor(ly, m)); lz = fminf(lz, __shfl_xor(lz, m));
        hx = fmaxf(hx, __shfl_xor(hx, m)); hy = fmaxf(hy, __shfl_xor(hy, m)); hz = fmaxf(hz, __shfl_xor(hz, m));
        mi = min(mi, __shfl_xor(mi, m));
    }
    if (lane == 0) {
        out[2 * node] = make_float4(lx, ly, lz, __int_as_float(mi));
        out[2 * node + 1] = make_float4(hx, hy, hz, 0.0f);
    }
}

// ------------------------------------------------------------------ the search
// The contract's distance: candidate minus query, squares summed as (x + y) + z, no contraction.
__device__ __forceinline__ float dist2(float px, float py, float pz, float qx, float qy, float qz)
{
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Distance from q to the box [lo, hi], by the same formula on the per-axis gaps.  It is a lower bound of d(q, p) for every p in the
// box, in float32: on an axis where q < lo, p >= lo gives p - q >= lo - q exactly, and rounding is monotone, so fl(p - q) >=
// fl(lo - q) >= 0 (the same for q > hi; the gap is 0 when q lies between).  Squaring a non-negative float and adding non-negative
// floats are monotone too (no fused multiply-add can change one side only), so box distance <= fl(d(q, p)), overflow to inf included.
// A box whose distance exceeds a lane's k-th entry therefore holds nothing that lane's list could take.
__device__ __forceinline__ float box_dist2(float qx, float qy, float qz, float4 lo, float4 hi)
{
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.0f), gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.0f), gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}
// the same bound for every q in the box [qlo, qhi] at once (fl(a - b) is monotone in a and in -b): orders and prunes a node's children
// for the whole wave
__device__ __forceinline__ float box_box_dist2(float4 qlo, float4 qhi, float4 lo, float4 hi)
{
    const float gx = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.0f), gy = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.0f),
                gz = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ float bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The per-lane list: kd ascending, ties by index.  IDX (indices wanted): (d, j) enters when lexicographically below the k-th pair; the
// k-th slot's sentinel (FLT_MAX, INT_MAX) is above every counted pair, so a pair at exactly FLT_MAX still enters.  Distances only: d
// enters when strictly below the k-th distance -- the multiset of the k smallest distances does not depend on which of equal
// distances is kept, and a lane whose k-th distance is 0 takes nothing more.
template <int K, bool IDX> struct List {
    float kd[K];
    int kj[IDX ? K : 1];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int t = 0; t < K; ++t) kd[t] = FLT_MAX;
#pragma unroll
        for (int t = 0; t < (IDX ? K : 1); ++t) kj[t] = INT_MAX;
    }
    __device__ __forceinline__ static bool below(float d, int j, float d2, int j2) { return IDX ? (d < d2 || (d == d2 && j < j2)) : d < d2; }
    __device__ __forceinline__ bool takes(float d, int j) const { return below(d, j, kd[K - 1], kj[IDX ? K - 1 : 0]); }
    // branch-free sorted insert; slot t is written from the old slots t - 1 and t only, top down
    __device__ __forceinline__ void insert(float d, int j)
    {
#pragma unroll
        for (int t = K - 1; t > 0; --t) {
            const bool prev = below(d, j, kd[t - 1], kj[IDX ? t - 1 : 0]), cur = below(d, j, kd[t], kj[IDX ? t : 0]);
            kd[t] = prev ? kd[t - 1] : (cur ? d : kd[t]);
            if (IDX) kj[t] = prev ? kj[t - 1] : (cur ? j : kj[t]);
        }
        if (below(d, j, kd[0], kj[0])) { kd[0] = d; if (IDX) kj[0] = j; }
    }
};

// every lane's list against the cnt points of one leaf, broadcast from the lanes that loaded them; self: skip lane == candidate (own leaf)
template <int K, bool IDX, bool SELF>
__device__ __forceinline__ void scan_leaf(const float4 *__restrict__ pts, int base, int cnt, int lane, bool act, float qx, float qy, float qz, List<K, IDX> &L)
{
    const float4 c = pts[base + min(lane, cnt - 1)];
    for (int t = 0; t < cnt; ++t) {
        const float px = bcast(c.x, t), py = bcast(c.y, t), pz = bcast(c.z, t);
        const int pj = IDX ? __builtin_amdgcn_readlane(__float_as_int(c.w), t) : 0;
        const float d = dist2(px, py, pz, qx, qy, qz);
        if (act && (!SELF || t != lane) && L.takes(d, pj)) L.insert(d, pj);
    }
}

template <int K, bool IDX>
__global__ __launch_bounds__(LEAF) void k_knn_search(const float4 *__restrict__ pts, const float4 *__restrict__ boxes, Levels T, int n,
                                                     int64_t *__restrict__ idx_out, float *__restrict__ dist_out, float *__restrict__ mean_out,
                                                     uint32_t *__restrict__ visits)
{
    __shared__ uint32_t stack[STACK];
    const int leaf = blockIdx.x, lane = threadIdx.x, base = leaf * LEAF;
    const int cnt0 = min(LEAF, n - base);
    const bool act = lane < cnt0;
    const float4 q = pts[base + min(lane, cnt0 - 1)];
    List<K, IDX> L;
    L.init();
    scan_leaf<K, IDX, true>(pts, base, cnt0, lane, act, q.x, q.y, q.z, L);
    const float4 qlo = boxes[2 * leaf], qhi = boxes[2 * leaf + 1];
    uint32_t nvis = 1, npop = 0;
    int sp = 0;
    if (T.levels > 1) {
        if (lane == 0) stack[0] = (uint32_t)(T.levels - 1) << LVL_SHIFT;
        sp = 1;
    }
    __syncthreads();
    while (sp > 0) {
        const uint32_t e = __builtin_amdgcn_readfirstlane(stack[sp - 1]);
        --sp;
        ++npop;
        const int lvl = (int)(e >> LVL_SHIFT), node = (int)(e & ((1u << LVL_SHIFT) - 1));
        if (lvl == 0 && node == leaf) continue;
        int off = 0, below_off = 0, below_cnt = 0;
#pragma unroll
        for (int l = 0; l < MAX_LEVELS; ++l) {
            if (l == lvl) off = T.off[l];
            if (l + 1 == lvl) { below_off = T.off[l]; below_cnt = T.cnt[l]; }
        }
        const float4 blo = boxes[2 * (off + node)], bhi = boxes[2 * (off + node) + 1];
        const bool need = act && L.takes(box_dist2(q.x, q.y, q.z, blo, bhi), __float_as_int(blo.w));
        if (!__any(need)) continue;
        if (lvl == 0) {
            scan_leaf<K, IDX, false>(pts, node * LEAF, min(LEAF, n - node * LEAF), lane, act, q.x, q.y, q.z, L);
            ++nvis;
            continue;
        }
        // push the children any lane may still need (a child farther from the wave's box than every lane's k-th distance is not), in
        // the order of their distance from the neediest lane's query -- the lane with the largest k-th distance, which the wave waits
        // for: farthest deepest, so its nearest child is popped next.  (Ordered by the wave's box instead, a wave whose leaf straddles
        // a jump of the Morton curve walks the whole stretch between the two ends in index order.)
        float maxkd = act ? L.kd[K - 1] : -1.0f;
        for (int m = LEAF / 2; m > 0; m >>= 1) maxkd = fmaxf(maxkd, __shfl_xor(maxkd, m));
        const int needy = __ffsll((unsigned long long)__ballot(act && L.kd[K - 1] == maxkd)) - 1;
        const float nx = bcast(q.x, needy), ny = bcast(q.y, needy), nz = bcast(q.z, needy);
        const int c = node * LEAF + lane;
        float key = 0.0f;
        bool push = c < below_cnt && !(lvl == 1 && c == leaf);
        if (push) {
            const float4 clo = boxes[2 * (below_off + c)], chi = boxes[2 * (below_off + c) + 1];
            const float dbb = box_box_dist2(qlo, qhi, clo, chi);
            push = IDX ? dbb <= maxkd : dbb < maxkd;
            key = box_dist2(nx, ny, nz, clo, chi);
        }
        uint64_t m = __ballot(push);
        const int npush = __popcll(m);
        int rank = 0;
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const float v = bcast(key, l);
            rank += (v > key || (v == key && l > lane)) ? 1 : 0;
        }
        if (push) stack[sp + rank] = (uint32_t)(lvl - 1) << LVL_SHIFT | (uint32_t)c;
        sp += npush;
        __syncthreads();
    }
    if (visits && lane == 0) { visits[2 * leaf] = nvis; visits[2 * leaf + 1] = npop; }
    if (!act) return;
    const int64_t i = __float_as_int(q.w);
    if (mean_out) {
        float s = L.kd[0];
#pragma unroll
        for (int t = 1; t < K; ++t) s += L.kd[t];
        mean_out[i] = s / (float)K;
    }
    if (dist_out) {
#pragma unroll
        for (int t = 0; t < K; ++t) dist_out[i * K + t] = L.kd[t];
    }
    if (IDX && idx_out) {
#pragma unroll
        for (int t = 0; t < K; ++t) idx_out[i * K + t] = L.kj[IDX ? t : 0] == INT_MAX ? -1 : L.kj[IDX ? t : 0];
    }
}

template <int K>
int launch_search(hipStream_t st, int nleaves, const float4 *pts, const float4 *boxes, const Levels &T, int n, int64_t *idx, float *dist, float *mean,
                  uint32_t *visits)
{
    if (idx) k_knn_search<K, true><<<nleaves, LEAF, 0, st>>>(pts, boxes, T, n, idx, dist, mean, visits);
    else k_knn_search<K, false><<<nleaves, LEAF, 0, st>>>(pts, boxes, T, n, nullptr, dist, mean, visits);
    LAUNCH_CHECK();
    return GPCC_OK;
}

}  // namespace

// Workspace layout (one alloc call): the bytes are at most 26 n + 64 KiB (header).  The sorted points (16 n) reuse the two key buffers.
extern "C" int gpcc_knn(gpcc_ctx *ctx, const float *xyz, int64_t n, int k, int64_t *idx_out, float *dist2_out, float *mean_out, gsr_alloc_fn alloc,
                       void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gpcc_knn: null context");
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(GPCC_ERR_ARG, "gpcc_knn: n = %lld outside [0, 2^31)", (long long)n);
    if (k < 1 || k > KNN_MAX_K) return fail(GPCC_ERR_ARG, "gpcc_knn: k = %d outside [1, %d]", k, KNN_MAX_K);
    if (n == 0) return GPCC_OK;
    if (!xyz || !alloc) return fail(GPCC_ERR_ARG, "gpcc_knn: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;

    Levels T = {};
    int64_t nodes = 0;
    for (int64_t c = cdiv(n, LEAF);; c = cdiv(c, LEAF)) {
        T.off[T.levels] = (int)nodes;
        T.cnt[T.levels] = (int)c;
        nodes += c;
        ++T.levels;
        if (c == 1) break;
    }
    const int nleaves = T.cnt[0];
    static const bool stats = dev_env_int("GAUSPCC_KNN_STATS", 0) != 0;   // developer: visited leaves and popped nodes per wave on stderr (synchronises)
    const int nb = (int)std::min<int64_t>(BB_MAX_BLOCKS, cdiv(n, (int64_t)TB * 8));
    float *box, *part;
    uint64_t *ka;
    uint32_t *va, *hist, *visits;
    float4 *boxes;
    GP_TRY(caller_block(alloc, alloc_user, "gpcc_knn", [&](Carver &c) {
        box = c.take<float>(8); part = c.take<float>(8 * nb); ka = c.take<uint64_t>(2 * n); va = c.take<uint32_t>(2 * n);
        hist = c.take<uint32_t>(radix_sort_hist_words(n)); boxes = c.take<float4>(2 * nodes); visits = stats ? c.take<uint32_t>(2 * nleaves) : nullptr;
    }));
    uint64_t *kb = ka + n;
    uint32_t *vb = va + n;
    float4 *pts = reinterpret_cast<float4 *>(ka);   // the sorted points, over the keys once the sort is done with them

    k_bbox<<<nb, TB, 0, st>>>(xyz, n, part);
    LAUNCH_CHECK();
    k_bbox_final<<<1, TB, 0, st>>>(part, nb, box);
    LAUNCH_CHECK();
    GP_TRY(ctx->hstage.reserve(64));
    uint32_t *hflag = reinterpret_cast<uint32_t *>(ctx->hstage.p);
    HIP_TRY(hipMemcpyAsync(hflag, box + 6, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (*hflag) return fail(GPCC_ERR_ARG, "gpcc_knn: the points hold a NaN or infinite coordinate");
    if (!idx_out && !dist2_out && !mean_out) return GPCC_OK;

    k_keys<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(xyz, n, box, ka, va);
    LAUNCH_CHECK();
    uint64_t *k0 = ka, *k1 = kb;
    uint32_t *v0 = va, *v1 = vb;
    GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, n, 63, hist));
    k_gather<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(xyz, v0, n, pts);   // the keys are dead: pts takes their 16 n bytes
    LAUNCH_CHECK();
    for (int l = 0; l < T.levels; ++l) {
        const int nchild = l == 0 ? (int)n : T.cnt[l - 1];
        k_node_box<<<(unsigned)cdiv(T.cnt[l], TB / LEAF), TB, 0, st>>>(l == 0 ? pts : nullptr, l == 0 ? nullptr : boxes + 2 * T.off[l - 1], nchild,
                                                                       T.cnt[l], boxes + 2 * T.off[l]);
        LAUNCH_CHECK();
    }
    const int ni = (int)n;
    switch (k) {
#define KNN_K(K) case K: GP_TRY(launch_search<K>(st, nleaves, pts, boxes, T, ni, idx_out, dist2_out, mean_out, visits)); break;
        KNN_K(1) KNN_K(2) KNN_K(3) KNN_K(4) KNN_K(5) KNN_K(6) KNN_K(7) KNN_K(8)
        KNN_K(9) KNN_K(10) KNN_K(11) KNN_K(12) KNN_K(13) KNN_K(14) KNN_K(15) KNN_K(16)
#undef KNN_K
    }
    if (stats) {
        std::vector<uint32_t> both(2 * (size_t)nleaves);
        HIP_TRY(hipMemcpyAsync(both.data(), visits, 8 * (size_t)nleaves, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        fprintf(stderr, "[knn] n=%lld k=%d idx=%d waves=%d", (long long)n, k, idx_out != nullptr, nleaves);
        for (int w = 0; w < 2; ++w) {
            std::vector<uint32_t> v((size_t)nleaves);
            double sum = 0;
            for (size_t i = 0; i < v.size(); ++i) sum += (v[i] = both[2 * i + w]);
            std::sort(v.begin(), v.end());
            fprintf(stderr, "  %s per wave: mean %.2f p50 %u p99 %u max %u", w ? "popped nodes" : "visited leaves", sum / nleaves, v[v.size() / 2],
                    v[(size_t)(0.99 * (v.size() - 1))], v.back());
        }
        fputc('\n', stderr);
    }
    return GPCC_OK;
}
