// cat_chain.hip -- gsac_decode_normal_chain: CAT-3DGS's channel-wise context chain decoded as a pipeline (include/gauspcc.h has the contract).
//
// The attribute streams of a 500-anchor slice (feat groups 0 .. G - 1, scaling, offsets: S = G + 2 files) depend on one another per ANCHOR: group i of
// anchor a is coded under parameters an MLP computes from groups 0 .. i - 1 of anchor a.  Decoded stage after stage with the wave-per-stream decoder of
// attributes.hip that is S launches of nslices waves, each waiting for the one before.  Here a WORKGROUP takes a slice and a WAVE a stage: the slice's
// anchors are cut into blocks of B, and in step t the wave of stage k continues its stream over block t - lag_k (lag 0 without an MLP, i for feat group
// i, G for scaling / offsets with an MLP), so every channel its MLP reads was published to the LDS window in an earlier step.  One __syncthreads() per
// step is the only synchronisation; every wave runs nblocks + max_lag steps whatever its stream holds.
//
// Arithmetic: the MLP in gshac_mlp2's specified order (mlp2.hip: acc = bias, fmaf over k ascending, ReLU x > 0 ? x : 0), mean = ctx + dmean one rounded
// add, scale = fmaxf(ctx + dscale, 1e-9f), the CDF entries normal_cdf_entry's, the value ((float)sym + (float)min) * Q as k_hac_decode_slices writes
// it: the result equals gshac_mlp2 + gsac_decode_normal_streams run stage after stage (tests/test_gpu_cat_codec.py).
// The weights are read by each wave from L2 (a wave needs only its own MLP, ~25 KB: Linear(<= 50, 100) and Linear(100, <= 60)); a block's hidden
// activations and parameter rows live in a per-wave LDS scratch of SB anchors at a time.
#include "primitives.hpp"
#include "attr_dev.hpp"

using namespace gpcc;

namespace {

constexpr int CHAIN_STAGES = 8;        // waves of a workgroup
constexpr int CHAIN_CH = 64;           // symbols per anchor of a stage, and feat channels an MLP reads
constexpr int CHAIN_DH = 128;          // hidden units
constexpr int CHAIN_B_MAX = 64;
constexpr int CHAIN_B_DEFAULT = 8;     // anchors per block: a 500-anchor slice is 63 steps + the lags
constexpr int SB = 4;                  // anchors whose parameters a wave computes at a time (one weight load serves SB chains)
constexpr size_t CHAIN_LDS_MAX = 160 * 1024;

struct DevStage {
    int32_t ch, dep_ch, dh, lag, mean_col, scale_col, feat_col, out_col, out_pitch, keep_group;
    const float *w1, *b1, *w2, *b2, *q;
    float *out;
    const uint8_t *keep;
    const uint8_t *bytes;              // device: the stage's streams, slice after slice
};
struct StreamRec { uint32_t off, nbytes; int32_t mn, lp; };      // one per (stage, slice)

struct WaveScratch {                   // LDS of one wave
    float hid[SB * CHAIN_DH];          // hidden activations of the sub-block
    float pm[SB * CHAIN_CH], ps[SB * CHAIN_CH];   // mean / scale of element e = a * ch + c
    float q[SB];
    int32_t sym[SB * CHAIN_CH];        // decoded symbols, in stream order
    int32_t idx[SB * CHAIN_CH];        // stream position -> element (stages with keep flags)
};

// LDS written by some lanes of the wave is read by others: the wave runs in lockstep, the fences keep the compiler from moving the accesses
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct CoderState { WaveBits in; uint32_t low, high, value; };

__device__ __forceinline__ int row_centre(const NormalRow &r) { return (int)__builtin_rintf(r.mean / r.q) - r.min_value; }
__device__ __forceinline__ int row_estimate(const NormalRow &r, float p)
{
    const float z = normcdfinvf(fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f));
    return (int)__builtin_rintf((r.mean + fmaxf(r.scale, 1e-9f) * z) / r.q) - r.min_value;
}

// hac_decode_chunk (attributes.hip) in resumable form: the coder's state comes in and goes out, the lane is threadIdx.x & 63, the rows are the
// sub-block's parameters in the wave's scratch (stream position j -> element idx[j] when `listed`), the symbols go to ws.sym in stream order.
// The search is that function's, tier by tier: 16 candidates around the mean for four rows per pass, a 64-wide window at the quantile, the binary search.
__device__ __forceinline__ void chain_decode_symbols(CoderState &cs, WaveScratch &ws, bool listed, int nsym, int ch, int mn, int lp)
{
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const float scale = (float)(65536 - (lp - 1));
    const int max_symbol = lp - 2;
    uint32_t low = cs.low, high = cs.high, value = cs.value;
    WaveBits &in = cs.in;
    for (int j0 = 0; j0 < nsym; j0 += 64) {
        const int jm = min(j0 + lane, nsym - 1);
        const int em = listed ? ws.idx[jm] : jm;
        const NormalRow mine{ws.pm[em], ws.ps[em], ws.q[em / ch], mn};
        const int jn = min(64, nsym - j0);
        for (int u0 = 0; u0 < jn; u0 += 4) {
            const int ug = min(u0 + g, jn - 1);
            const NormalRow rowg{__shfl(mine.mean, ug), __shfl(mine.scale, ug), __shfl(mine.q, ug), mn};
            const int s0g = max_symbol > 15 ? max(0, min(row_centre(rowg) - 7, max_symbol - 15)) : 0;
            const int mg = s0g + c;
            const uint32_t preg = mg <= max_symbol ? cdf_int(rowg, mg, scale) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (u0 + u >= jn) break;
                const uint64_t span = (uint64_t)high - (uint64_t)low + 1u;
                const uint32_t x = value - low;
                const uint32_t t = (uint32_t)((span * (uint64_t)preg) >> 16);
                const uint32_t bal = (uint32_t)(__ballot(g == u && mg <= max_symbol && (mg == 0 || t <= x)) >> (16 * u)) & 0xFFFFu;
                const int top = 31 - clz32(bal);
                int s = (int)lane_value((uint32_t)s0g, 16 * u) + top;
                uint32_t lo, hi;
                if (bal != 0u && (top < 15 || s == max_symbol)) {
                    lo = lane_value(t, 16 * u + top);
                    const uint32_t nxt = lane_value(t, 16 * u + min(top + 1, 15));
                    hi = s == max_symbol ? (uint32_t)span : nxt;
                } else {
                    const int uu = u0 + u;
                    const NormalRow row{__shfl(mine.mean, uu), __shfl(mine.scale, uu), __shfl(mine.q, uu), mn};
                    const int w0 = max_symbol > 63 ? max(0, min(row_estimate(row, (float)x / (float)span) - 31, max_symbol - 63)) : 0;
                    const int m = w0 + lane;
                    const uint32_t tw = m <= max_symbol ? (uint32_t)((span * (uint64_t)cdf_int(row, m, scale)) >> 16) : 0u;
                    const uint64_t balw = __ballot(m <= max_symbol && (m == 0 || tw <= x));
                    const int topw = 63 - __clzll((long long)balw);
                    s = w0 + topw;
                    if (balw != 0ull && (topw < 63 || s == max_symbol)) {
                        lo = lane_value(tw, topw);
                        const uint32_t nxt = lane_value(tw, min(topw + 1, 63));
                        hi = s == max_symbol ? (uint32_t)span : nxt;
                    } else {
                        int left = 0, right = max_symbol + 1;
                        while (left + 1 < right) {
                            const int mid = (left + right) / 2;
                            const uint32_t v = uniform(cdf_int(row, mid, scale));
                            if ((uint32_t)((span * (uint64_t)v) >> 16) <= x) left = mid; else right = mid;
                        }
                        s = left;
                        lo = (uint32_t)((span * (uint64_t)uniform(cdf_int(row, s, scale))) >> 16);
                        hi = s == max_symbol ? (uint32_t)span : (uint32_t)((span * (uint64_t)uniform(cdf_int(row, s + 1, scale))) >> 16);
                    }
                }
                if (lane == 0) ws.sym[j0 + u0 + u] = s;
                high = (low - 1u) + hi;
                low = low + lo;
                const int n1 = clz32(low ^ high);
                low <<= n1; high = (high << n1) | ((1u << n1) - 1u); value = (value << n1) | in.take((uint32_t)n1);
                const int n2 = min(min(clz32(~(low << 1)), clz32(high << 1)), 31);
                low = (low << n2) & (n2 ? 0x7FFFFFFFu : 0xFFFFFFFFu);
                high = (high << n2) | (n2 ? 0x80000000u : 0u) | ((1u << n2) - 1u);
                value = ((value << n2) ^ (n2 ? 0x80000000u : 0u)) | in.take((uint32_t)n2);
                low = uniform(low); high = uniform(high); value = uniform(value);
            }
        }
    }
    cs.low = low; cs.high = high; cs.value = value;
}

// grid: one workgroup per slice; block: 64 * S threads, wave k = stage k.  LDS: the window ring[W][B][fc] of decoded feat channels (W = max_lag + 1
// blocks: the slot of block b is reused by block b + W, which no stage reads before step b + W > b + max_lag), then one WaveScratch per wave.
__global__ __launch_bounds__(64 * CHAIN_STAGES) void k_normal_chain(const DevStage *__restrict__ stages, const StreamRec *__restrict__ recs,
                                                                    const float *__restrict__ ctx, int ctx_pitch, int64_t n, int slice_anchors, int B, int W,
                                                                    int fc, int max_lag)
{
    extern __shared__ float lds[];
    const int wave = (int)uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float *ring = lds;
    WaveScratch &ws = *reinterpret_cast<WaveScratch *>(lds + (size_t)W * B * fc + (size_t)wave * (sizeof(WaveScratch) / 4));
    const int slice = blockIdx.x;
    const int64_t a_first = (int64_t)slice * slice_anchors;
    const int na = (int)min((int64_t)slice_anchors, n - a_first);
    const int nblocks = (na + B - 1) / B;

    const DevStage st = stages[wave];
    const int ch = (int)uniform((uint32_t)st.ch), dep_ch = (int)uniform((uint32_t)st.dep_ch), dh = (int)uniform((uint32_t)st.dh);
    const int lag = (int)uniform((uint32_t)st.lag), feat_col = (int)uniform((uint32_t)st.feat_col);
    const bool listed = st.keep != nullptr;
    const int kpa = listed ? ch / st.keep_group : 0;
    const StreamRec rec = recs[(size_t)wave * gridDim.x + slice];
    const int mn = (int)uniform((uint32_t)rec.mn), lp = (int)uniform((uint32_t)rec.lp);
    CoderState cs;
    cs.in.init(st.bytes + uniform(rec.off), uniform(rec.nbytes));
    cs.low = 0; cs.high = 0xFFFFFFFFu;
    cs.value = cs.in.take(32);

    for (int t = 0; t < nblocks + max_lag; ++t) {
        const int blk = t - lag;
        if (blk >= 0 && blk < nblocks) {
            const int nb = min(B, na - blk * B);
            float *slot = ring + (size_t)(blk % W) * B * fc;
            for (int a0 = 0; a0 < nb; a0 += SB) {
                const int nsb = min(SB, nb - a0);
                const int64_t row0 = a_first + (int64_t)blk * B + a0;
                // 1  the parameter rows of the sub-block
                if (lane < nsb) ws.q[lane] = st.q[row0 + lane];
                if (dep_ch > 0) {
                    const float *xr[SB];
#pragma unroll
                    for (int a = 0; a < SB; ++a) xr[a] = slot + (size_t)(a0 + min(a, nsb - 1)) * fc;
                    for (int j = lane; j < dh; j += 64) {
                        const float *w = st.w1 + (size_t)j * dep_ch;
                        float acc[SB];
                        const float bj = st.b1[j];
#pragma unroll
                        for (int a = 0; a < SB; ++a) acc[a] = bj;
                        for (int k = 0; k < dep_ch; ++k) {
                            const float wk = w[k];
#pragma unroll
                            for (int a = 0; a < SB; ++a) acc[a] = __builtin_fmaf(xr[a][k], wk, acc[a]);
                        }
#pragma unroll
                        for (int a = 0; a < SB; ++a) ws.hid[a * CHAIN_DH + j] = acc[a] > 0.0f ? acc[a] : 0.0f;
                    }
                    wave_sync();
                    for (int o = lane; o < 2 * ch; o += 64) {
                        const float *w = st.w2 + (size_t)o * dh;
                        float acc[SB];
                        const float bo = st.b2[o];
#pragma unroll
                        for (int a = 0; a < SB; ++a) acc[a] = bo;
                        for (int k = 0; k < dh; ++k) {
                            const float wk = w[k];
#pragma unroll
                            for (int a = 0; a < SB; ++a) acc[a] = __builtin_fmaf(ws.hid[a * CHAIN_DH + k], wk, acc[a]);
                        }
                        const bool is_mean = o < ch;
                        const int cc = is_mean ? o : o - ch;
#pragma unroll
                        for (int a = 0; a < SB; ++a) {
                            if (a < nsb) {
                                const float base = ctx[(size_t)(row0 + a) * ctx_pitch + (is_mean ? st.mean_col : st.scale_col) + cc];
                                const float v = __fadd_rn(base, acc[a]);
                                if (is_mean) ws.pm[a * ch + cc] = v; else ws.ps[a * ch + cc] = fmaxf(v, 1e-9f);
                            }
                        }
                    }
                } else {
                    for (int e = lane; e < nsb * ch; e += 64) {
                        const int a = e / ch, cc = e - a * ch;
                        const float *cr = ctx + (size_t)(row0 + a) * ctx_pitch;
                        ws.pm[e] = cr[st.mean_col + cc];
                        ws.ps[e] = fmaxf(cr[st.scale_col + cc], 1e-9f);
                    }
                }
                // the kept elements in stream order; the others are written as 0
                int nsym = nsb * ch;
                if (listed) {
                    int base = 0;
                    for (int e0 = 0; e0 < nsb * ch; e0 += 64) {
                        const int e = e0 + lane;
                        bool kept = false;
                        if (e < nsb * ch) {
                            const int a = e / ch, cc = e - a * ch;
                            kept = st.keep[(size_t)(row0 + a) * kpa + cc / st.keep_group] != 0;
                            if (!kept) st.out[(size_t)(row0 + a) * st.out_pitch + st.out_col + cc] = 0.0f;
                        }
                        const uint64_t bal = __ballot(kept);
                        if (kept) ws.idx[base + __popcll(bal & ((1ull << lane) - 1ull))] = e;
                        base += __popcll(bal);
                    }
                    nsym = (int)uniform((uint32_t)base);
                }
                wave_sync();
                // 2  the stream continues over the sub-block's symbols
                chain_decode_symbols(cs, ws, listed, nsym, ch, mn, lp);
                wave_sync();
                // 3  publish
                for (int j = lane; j < nsym; j += 64) {
                    const int e = listed ? ws.idx[j] : j;
                    const int a = e / ch, cc = e - a * ch;
                    const float v = __fmul_rn((float)ws.sym[j] + (float)mn, ws.q[a]);
                    st.out[(size_t)(row0 + a) * st.out_pitch + st.out_col + cc] = v;
                    if (feat_col >= 0) slot[(size_t)(a0 + a) * fc + feat_col + cc] = v;
                }
                wave_sync();
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int gsac_decode_normal_chain(gpcc_ctx *ctx, const gsac_chain_stage *stages, int nstages, const float *ctx_dev, int ctx_pitch, int64_t n,
                                        int slice_anchors, int nslices, int block_anchors, void *stream)
{
    if (!ctx || !stages || !ctx_dev) return fail(GPCC_ERR_ARG, "null argument");
    if (nstages < 1 || nstages > CHAIN_STAGES) return fail(GPCC_ERR_ARG, "a chain of %d stages (1..%d)", nstages, CHAIN_STAGES);
    if (n <= 0 || slice_anchors <= 0 || ctx_pitch <= 0 || nslices <= 0 || (int64_t)nslices != cdiv(n, slice_anchors)) return fail(GPCC_ERR_ARG, "bad size");
    if (block_anchors < 0 || block_anchors > CHAIN_B_MAX) return fail(GPCC_ERR_ARG, "block_anchors %d (0, or 1..%d)", block_anchors, CHAIN_B_MAX);
    const int B = block_anchors ? block_anchors : CHAIN_B_DEFAULT;
    const int S = nstages;
    int fc = 0, max_lag = 0;
    bool published[CHAIN_CH] = {};
    for (int k = 0; k < S; ++k) {
        const gsac_chain_stage &s = stages[k];
        if (s.ch < 1 || s.ch > CHAIN_CH || s.dep_ch < 0 || s.dep_ch > CHAIN_CH) return fail(GPCC_ERR_ARG, "stage %d: ch %d, dep_ch %d (at most %d)", k, s.ch, s.dep_ch, CHAIN_CH);
        if (s.dep_ch > 0 && (s.dh < 1 || s.dh > CHAIN_DH)) return fail(GPCC_ERR_ARG, "stage %d: %d hidden units (1..%d)", k, s.dh, CHAIN_DH);
        if (s.dep_ch > 0 && (!s.w1 || !s.b1 || !s.w2 || !s.b2)) return fail(GPCC_ERR_ARG, "stage %d: null weights", k);
        if (!s.q_dev || !s.out_dev || !s.cnt || !s.min_value || !s.max_value || (!s.bytes && s.nbytes != 0)) return fail(GPCC_ERR_ARG, "stage %d: null argument", k);
        if (s.lag < 0 || s.lag >= CHAIN_STAGES || (s.dep_ch == 0 && s.lag != 0)) return fail(GPCC_ERR_ARG, "stage %d: lag %d", k, s.lag);
        if (s.mean_col < 0 || s.scale_col < 0 || s.mean_col + s.ch > ctx_pitch || s.scale_col + s.ch > ctx_pitch) return fail(GPCC_ERR_ARG, "stage %d: columns outside the context row", k);
        if (s.out_col < 0 || s.out_pitch <= 0 || s.out_col + s.ch > s.out_pitch) return fail(GPCC_ERR_ARG, "stage %d: columns outside the output row", k);
        if (s.feat_col < -1 || (s.feat_col >= 0 && s.feat_col + s.ch > CHAIN_CH)) return fail(GPCC_ERR_ARG, "stage %d: feat channels %d..%d (at most %d)", k, s.feat_col, s.feat_col + s.ch, CHAIN_CH);
        if (s.keep_dev && (s.keep_group < 1 || s.ch % s.keep_group != 0)) return fail(GPCC_ERR_ARG, "stage %d: keep_group %d does not divide ch %d", k, s.keep_group, s.ch);
        if (s.nbytes < 0 || s.nbytes >= ((int64_t)1 << 32)) return fail(GPCC_ERR_FORMAT, "stage %d: byte stream must be shorter than 4 GiB", k);
        if (s.feat_col >= 0) {
            fc = std::max(fc, s.feat_col + s.ch);
            for (int c = 0; c < s.ch; ++c) published[s.feat_col + c] = true;
        }
        max_lag = std::max(max_lag, s.lag);
    }
    for (int k = 0; k < S; ++k) {
        const gsac_chain_stage &s = stages[k];
        for (int c = 0; c < s.dep_ch; ++c)
            if (!published[c]) return fail(GPCC_ERR_ARG, "stage %d reads feat channel %d, which no stage decodes", k, c);
        for (int j = 0; j < S; ++j)
            if (s.dep_ch > 0 && stages[j].feat_col >= 0 && stages[j].feat_col < s.dep_ch && s.lag <= stages[j].lag)
                return fail(GPCC_ERR_ARG, "stage %d (lag %d) reads channels of stage %d (lag %d) before they are decoded", k, s.lag, j, stages[j].lag);
    }
    const int W = max_lag + 1;
    const size_t lds_bytes = 4 * (size_t)W * B * fc + (size_t)S * sizeof(WaveScratch);
    if (lds_bytes > CHAIN_LDS_MAX) return fail(GPCC_ERR_ARG, "block_anchors %d: the window of %d blocks x %d channels exceeds a CU's LDS", B, W, fc);

    // the streams of every (stage, slice): counts and ranges come from files
    std::vector<StreamRec> recs((size_t)S * nslices);
    std::vector<size_t> stage_off((size_t)S);
    size_t total = 0;
    for (int k = 0; k < S; ++k) {
        const gsac_chain_stage &s = stages[k];
        stage_off[(size_t)k] = total;
        uint64_t run = 0;
        for (int sl = 0; sl < nslices; ++sl) {
            StreamRec &r = recs[(size_t)k * nslices + sl];
            if (s.cnt[sl] < 0) return fail(GPCC_ERR_FORMAT, "stage %d: negative stream size", k);
            int mn, lp;
            if (symbol_range(s.min_value[sl], s.max_value[sl], &mn, &lp) != GPCC_OK) return fail(GPCC_ERR_FORMAT, "stage %d, slice %d: bad symbol range", k, sl);
            r = StreamRec{(uint32_t)run, (uint32_t)s.cnt[sl], mn, lp};
            run += (uint32_t)s.cnt[sl];
            if (run > (uint64_t)s.nbytes) return fail(GPCC_ERR_FORMAT, "stage %d: stream sizes exceed the byte stream", k);
        }
        total += ((size_t)s.nbytes + 16 + 15) & ~(size_t)15;
    }

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    GP_TRY(ctx->arena.reserve(total + sizeof(StreamRec) * recs.size() + sizeof(DevStage) * S + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(db, uint8_t, total + 16); TAKE(drecs, StreamRec, recs.size()); TAKE(dst, DevStage, S);
    DevStage hst[CHAIN_STAGES];
    for (int k = 0; k < S; ++k) {
        const gsac_chain_stage &s = stages[k];
        hst[k] = DevStage{s.ch, s.dep_ch, s.dep_ch > 0 ? s.dh : 0, s.lag, s.mean_col, s.scale_col, s.feat_col, s.out_col, s.out_pitch, s.keep_dev ? s.keep_group : 1,
                          s.w1, s.b1, s.w2, s.b2, s.q_dev, s.out_dev, s.keep_dev, db + stage_off[(size_t)k]};
        if (s.nbytes) HIP_TRY(hipMemcpyAsync(db + stage_off[(size_t)k], s.bytes, (size_t)s.nbytes, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(drecs, recs.data(), sizeof(StreamRec) * recs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dst, hst, sizeof(DevStage) * S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope before the stream drains otherwise
    if (lds_bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_normal_chain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    k_normal_chain<<<(unsigned)nslices, 64 * S, lds_bytes, st>>>(dst, drecs, ctx_dev, ctx_pitch, n, slice_anchors, B, W, fc, max_lag);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}
