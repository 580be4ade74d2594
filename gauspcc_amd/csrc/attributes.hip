// attributes.hip -- the chunked range coder of the HAC / HAC++ attributes:
//   gsac_calculate_cdf   arithmetic.calculate_cdf      arithmetic.zip!arithmetic/arithmetic_kernel.cu:7-54
//   gsac_encode/_decode  arithmetic.arithmetic_encode / arithmetic_decode   ...:94-232, 265-403
//   gsac_*_gaussian*     the same without the CDF table: plain Gaussian or HAC++'s mixture, one stream or every slice of an attribute
//   gsac_*_normal_*      TC-GS / CAT-3DGS's torchac files (TC-GS/utils/encodings.py:84-146): the slice form with chunk = slice, Normal.cdf's entries
// (the hash-grid encoder is gridencoder.hip, the context MLP mlp2.hip)
// Same byte format as the reference's CUDA coder (chunks of `chunk_size` symbols, per-chunk byte
// counts), same integerisation of the float CDF rows (rint(cdf * (65536 - (Lp-1))) + index).
//
// Where the reference runs ONE THREAD per chunk (<<<chunks, 1>>>) this version
//   * encodes with the geometry path's lane-per-chunk coder after a fully parallel pre-pass that
//     turns (cdf row, symbol) into the two integers the coder needs;
//   * decodes with one WAVE per chunk: the 64 lanes integerise and scale a whole CDF row at once,
//     a ballot finds the symbol (no binary search, no division), rows are prefetched 4 symbols ahead.
#include "octree.hpp"
#include "primitives.hpp"
#include "rangecoder.hpp"
#include "coder_tail.hpp"
#include "attr_dev.hpp"

using namespace gpcc;

namespace {

constexpr int TB = 256;

// ------------------------------------------------------------------ calculate_cdf
// lower[idx][i] of arithmetic.calculate_cdf (arithmetic_kernel.cu:7-28) -- ONE definition, used by the table kernel and by
// the fused coder below, so a stream coded without the table is byte-identical to one coded with it
__device__ __forceinline__ float gaussian_cdf_entry(float mean, float scale, float q, int min_value, int i)
{
    const float sc = (float)fmax((double)scale, 1e-9);                            // max(scale[idx], 1e-9)
    const float sample = (float)(((double)(min_value + i) - 0.5) * (double)q);    // (min + i - 0.5) * Q
    const float arg = -(sample - mean) / (sc * sqrtf(2.0f));
    return (float)(0.5 * (double)erfcf(arg));
}

__global__ __launch_bounds__(TB) void k_gaussian_cdf(const float *__restrict__ mean, const float *__restrict__ scale, const float *__restrict__ Q, int64_t n,
                                                     int min_value, int lp, float *__restrict__ lower)
{
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= n * lp) return;
    const int64_t idx = t / lp;
    lower[t] = gaussian_cdf_entry(mean[idx], scale[idx], Q[idx], min_value, (int)(t - idx * lp));
}


// Row sources of the coder: a float table row, a uint16 table row (torchac's *_int16_normalized_cdf), or the Gaussian
// parameters of the element -- the table-free path of encoder_gaussian / decoder_gaussian (the reference writes and
// re-reads n x (max - min + 2) floats per slice; here the two entries an encoded symbol needs, or the <= 64 entries a
// decoding wave compares, are evaluated in registers).
struct GaussTable { const float *mean, *scale, *q; int min_value; };
struct GaussRow { float mean, scale, q; int min_value; };
// HAC++'s mixture (HAC-plus/utils/encodings_cuda.py:205-225, 285-299): lower = clamp(sum_i calculate_cdf(mean_i, scale_i, Q) *
// prob_i, 0, 1), the components added in list order in fp32 (a product, then a sum: no fused multiply-add)
constexpr int MIX_MAX = 4;
struct MixTable { const float *mean[MIX_MAX], *scale[MIX_MAX], *prob[MIX_MAX]; const float *q; int k, min_value; };
struct MixRow { float mean[MIX_MAX], scale[MIX_MAX], prob[MIX_MAX]; float q; int k, min_value; };
// one CDF row for every symbol: the Bernoulli coder of the hash tables and masks (encodings_cuda.py: encoder / decoder build an (n, 3) table whose rows
// are all (0, 1 - p, 1) -- 120 MB written and read back for the ten million mask bits of a million anchors)
struct ConstTable { float c[4]; };
struct ConstRow { float c0, c1, c2, c3; };
template <typename CT> struct RowOf { typedef const CT *type; };
template <> struct RowOf<ConstTable> { typedef ConstRow type; };
template <> struct RowOf<GaussTable> { typedef GaussRow type; };
template <> struct RowOf<NormalTable> { typedef NormalRow type; };
template <> struct RowOf<MixTable> { typedef MixRow type; };
__device__ __forceinline__ const float *row_of(const float *t, int64_t idx, int lp) { return t + idx * lp; }
__device__ __forceinline__ const uint16_t *row_of(const uint16_t *t, int64_t idx, int lp) { return t + idx * lp; }
__device__ __forceinline__ ConstRow row_of(const ConstTable &t, int64_t, int) { return ConstRow{t.c[0], t.c[1], t.c[2], t.c[3]}; }
__device__ __forceinline__ GaussRow row_of(const GaussTable &t, int64_t idx, int) { return GaussRow{t.mean[idx], t.scale[idx], t.q[idx], t.min_value}; }
__device__ __forceinline__ NormalRow row_of(const NormalTable &t, int64_t idx, int) { return NormalRow{t.mean[idx], t.scale[idx], t.q[idx], t.min_value}; }
__device__ __forceinline__ MixRow row_of(const MixTable &t, int64_t idx, int)
{
    MixRow r;
    r.q = t.q[idx]; r.k = t.k; r.min_value = t.min_value;
#pragma unroll
    for (int i = 0; i < MIX_MAX; ++i)
        if (i < t.k) { r.mean[i] = t.mean[i][idx]; r.scale[i] = t.scale[i][idx]; r.prob[i] = t.prob[i][idx]; }
    return r;
}
__device__ __forceinline__ float mix_cdf_entry(const MixRow &row, int m)
{
    float acc = gaussian_cdf_entry(row.mean[0], row.scale[0], row.q, row.min_value, m) * row.prob[0];
#pragma unroll
    for (int i = 1; i < MIX_MAX; ++i)
        if (i < row.k) acc = acc + gaussian_cdf_entry(row.mean[i], row.scale[i], row.q, row.min_value, m) * row.prob[i];
    return fminf(fmaxf(acc, 0.0f), 1.0f);
}

// the mixture's table (tests, and callers that want the reference's two-step form)
__global__ __launch_bounds__(TB) void k_mixture_cdf(MixTable t, int64_t n, int lp, float *__restrict__ lower)
{
    const int64_t q = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (q >= n * lp) return;
    const int64_t idx = q / lp;
    lower[q] = mix_cdf_entry(row_of(t, idx, lp), (int)(q - idx * lp));
}

// ------------------------------------------------------------------ encode pre-pass
// CDF entry -> integer: float rows are integerised on the fly (arithmetic_kernel.cu:124-125 == kit/op.py:67-79),
// uint16 rows (torchac's *_int16_normalized_cdf) are used as they are
__device__ __forceinline__ uint32_t cdf_int(const float *row, int m, float scale) { return (uint32_t)((int)__builtin_rintf(row[m] * scale) + m); }
__device__ __forceinline__ uint32_t cdf_int(const uint16_t *row, int m, float) { return row[m]; }
__device__ __forceinline__ uint32_t cdf_int(const ConstRow &row, int m, float scale)
{
    const float v = m == 0 ? row.c0 : m == 1 ? row.c1 : m == 2 ? row.c2 : row.c3;
    return (uint32_t)((int)__builtin_rintf(v * scale) + m);
}
__device__ __forceinline__ uint32_t cdf_int(const GaussRow &row, int m, float scale)
{
    return (uint32_t)((int)__builtin_rintf(gaussian_cdf_entry(row.mean, row.scale, row.q, row.min_value, m) * scale) + m);
}
__device__ __forceinline__ uint32_t cdf_int(const MixRow &row, int m, float scale) { return (uint32_t)((int)__builtin_rintf(mix_cdf_entry(row, m) * scale) + m); }

template <typename CT>
__global__ __launch_bounds__(TB) void k_hac_pack(const CT cdf, const int16_t *__restrict__ sym, int64_t n, int lp, int chunk, uint32_t nch,
                                                 uint32_t *__restrict__ lohi)
{
    const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (r >= n) return;
    const float scale = (float)(65536 - (lp - 1));
    const int s = sym[r];
    const auto row = row_of(cdf, r, lp);
    const uint32_t lo = cdf_int(row, s, scale);
    const uint32_t hi = s == lp - 2 ? 0x10000u : cdf_int(row, s + 1, scale);
    const uint32_t c = (uint32_t)(r / chunk), t = (uint32_t)(r - (int64_t)c * chunk);
    lohi[(size_t)t * nch + c] = (lo & 0xFFFFu) | ((hi - 1u) << 16);
}

// ------------------------------------------------------------------ decode: one wave per chunk

// Row parameters of 64 consecutive symbols at once (round 5): lane j loads row i0 + j -- three coalesced loads per 64 symbols for a GaussTable instead
// of three broadcast loads per symbol whose latency (~1 us from HBM) sat in the decode chain four symbols at a time -- and a row is handed to the
// wave by lane broadcasts.  Table rows (float / uint16) are pointers: nothing to load.
template <typename CT> struct RowLoader {
    __device__ __forceinline__ static auto load(const CT &t, int64_t idx, int lp) { return row_of(t, idx, lp); }
    template <typename R> __device__ __forceinline__ static auto get(const CT &t, const R &, int64_t idx, int lp, int) { return row_of(t, idx, lp); }
    template <typename R> __device__ __forceinline__ static int centre(const R &, int max_symbol) { return max_symbol / 2; }
    template <typename R> __device__ __forceinline__ static int estimate(const R &, float p, int max_symbol) { return (int)(p * (float)max_symbol); }
};
// (GaussTable / GaussRow, and NormalTable / NormalRow: the same three parameters per element)
template <typename T, typename R> struct ParamRowLoader {
    __device__ __forceinline__ static R load(const T &t, int64_t idx, int lp) { return row_of(t, idx, lp); }
    __device__ __forceinline__ static R get(const T &, const R &mine, int64_t, int, int u)
    {
        return R{__shfl(mine.mean, u), __shfl(mine.scale, u), __shfl(mine.q, u), mine.min_value};
    }
    // index of the symbol nearest the mean: where a window of 64 candidates is put when the alphabet is wider than a wave
    __device__ __forceinline__ static int centre(const R &r, int) { return (int)__builtin_rintf(r.mean / r.q) - r.min_value; }
    // index whose CDF entry is about p: the Gaussian's quantile (an ESTIMATE: the window put around it is checked like any other)
    __device__ __forceinline__ static int estimate(const R &r, float p, int)
    {
        const float z = normcdfinvf(fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f));
        return (int)__builtin_rintf((r.mean + fmaxf(r.scale, 1e-9f) * z) / r.q) - r.min_value;
    }
};
template <> struct RowLoader<GaussTable> : ParamRowLoader<GaussTable, GaussRow> {};
template <> struct RowLoader<NormalTable> : ParamRowLoader<NormalTable, NormalRow> {};
template <> struct RowLoader<MixTable> {
    __device__ __forceinline__ static MixRow load(const MixTable &t, int64_t idx, int lp) { return row_of(t, idx, lp); }
    __device__ __forceinline__ static MixRow get(const MixTable &, const MixRow &mine, int64_t, int, int u)
    {
        MixRow r;
        r.q = __shfl(mine.q, u); r.k = mine.k; r.min_value = mine.min_value;
#pragma unroll
        for (int i = 0; i < MIX_MAX; ++i)
            if (i < mine.k) { r.mean[i] = __shfl(mine.mean[i], u); r.scale[i] = __shfl(mine.scale[i], u); r.prob[i] = __shfl(mine.prob[i], u); }
        return r;
    }
    __device__ __forceinline__ static int centre(const MixRow &r, int)
    {
        int best = 0;
#pragma unroll
        for (int i = 1; i < MIX_MAX; ++i)
            if (i < r.k && r.prob[i] > r.prob[best]) best = i;
        float m = r.mean[0];
#pragma unroll
        for (int i = 1; i < MIX_MAX; ++i) m = best == i ? r.mean[i] : m;
        return (int)__builtin_rintf(m / r.q) - r.min_value;
    }
    __device__ __forceinline__ static int estimate(const MixRow &r, float p, int)
    {   // the quantile of the heaviest component: a starting point
        int best = 0;
#pragma unroll
        for (int i = 1; i < MIX_MAX; ++i)
            if (i < r.k && r.prob[i] > r.prob[best]) best = i;
        float m = r.mean[0], sc = r.scale[0];
#pragma unroll
        for (int i = 1; i < MIX_MAX; ++i) { m = best == i ? r.mean[i] : m; sc = best == i ? r.scale[i] : sc; }
        const float z = normcdfinvf(fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f));
        return (int)__builtin_rintf((m + fmaxf(sc, 1e-9f) * z) / r.q) - r.min_value;
    }
};

// One wave decodes one chunk: `cn` symbols whose rows are base .. base+cn-1 of `cdf`; out(row, symbol) stores the result.
// A symbol is the highest index m with  (span * cdf_int(m)) >> 16  <=  value - low  (index 0 always qualifies; the integerised row is strictly
// increasing: rint(cdf * scale) + m).  The kernel is bound by VALU issue -- one erfc (~100 instructions with its fp64 steps; k of them for HAC++'s
// mixtures) per candidate PASS of the wave, whatever the number of useful lanes -- and the candidates of a row do not depend on the decoder's state.
// So a pass serves FOUR rows: lane (g, c) evaluates candidate s0[g] + c of row g, a window of 16 around the element's mean (the whole row when the
// alphabet has <= 16 symbols); the serial part per symbol is then a scaled compare, a ballot over the row's 16 lanes and the range update.  Round 4
// spent a full 64-candidate pass per symbol (and, for alphabets wider than a wave, a wave-uniform binary search: seven dependent erfc per symbol).
// A window that does not bracket the value falls back to a 64-wide window of the row's own and then to the binary search: the same index either way.
template <typename CT, typename OUT>
__device__ __forceinline__ void hac_decode_chunk(const CT &cdf, const uint8_t *__restrict__ chunk_bytes, uint32_t chunk_nbytes, int64_t base, int cn, int lp,
                                                 OUT out)
{
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const float scale = (float)(65536 - (lp - 1));
    const int max_symbol = lp - 2;            // indices 0 .. lp-2 are searched
    WaveBits in;
    in.init(chunk_bytes, chunk_nbytes);
    uint32_t low = 0, high = 0xFFFFFFFFu;
    uint32_t value = in.take(32);
    typedef RowLoader<CT> RL;
    for (int j0 = 0; j0 < cn; j0 += 64) {
        const auto mine = RL::load(cdf, base + min(j0 + lane, cn - 1), lp);
        const int jn = min(64, cn - j0);
        for (int u0 = 0; u0 < jn; u0 += 4) {
            // one pass: 16 candidates of each of the next four rows (rows do not depend on decoded symbols)
            const int ug = min(u0 + g, jn - 1);
            const auto rowg = RL::get(cdf, mine, base + j0 + ug, lp, ug);
            const int s0g = max_symbol > 15 ? max(0, min(RL::centre(rowg, max_symbol) - 7, max_symbol - 15)) : 0;
            const int mg = s0g + c;
            const uint32_t preg = mg <= max_symbol ? cdf_int(rowg, mg, scale) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (u0 + u >= jn) break;
                const int64_t r = base + j0 + u0 + u;
                const uint64_t span = (uint64_t)high - (uint64_t)low + 1u;
                const uint32_t x = value - low;
                const uint32_t t = (uint32_t)((span * (uint64_t)preg) >> 16);
                const uint32_t bal = (uint32_t)(__ballot(g == u && mg <= max_symbol && (mg == 0 || t <= x)) >> (16 * u)) & 0xFFFFu;
                const int top = 31 - clz32(bal);                   // -1: no candidate qualifies
                int s = (int)lane_value((uint32_t)s0g, 16 * u) + top;
                uint32_t lo, hi;
                if (bal != 0u && (top < 15 || s == max_symbol)) {
                    lo = lane_value(t, 16 * u + top);
                    const uint32_t nxt = lane_value(t, 16 * u + min(top + 1, 15));
                    hi = s == max_symbol ? (uint32_t)span : nxt;
                } else {
                    // the narrow window does not bracket the value: a 64-wide window of this row alone, then the wave-uniform binary search
                    const auto row = RL::get(cdf, mine, r, lp, u0 + u);
                    // (centred on the quantile of value - low within the range: wide rows -- HAC's scaling attribute has sigma / Q ~ 50 -- land in it)
                    const int w0 = max_symbol > 63 ? max(0, min(RL::estimate(row, (float)x / (float)span, max_symbol) - 31, max_symbol - 63)) : 0;
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
                            const uint32_t v = uniform(cdf_int(row, mid, scale));     // (every lane computed the same number)
                            if ((uint32_t)((span * (uint64_t)v) >> 16) <= x) left = mid; else right = mid;
                        }
                        s = left;
                        lo = (uint32_t)((span * (uint64_t)uniform(cdf_int(row, s, scale))) >> 16);
                        hi = s == max_symbol ? (uint32_t)span : (uint32_t)((span * (uint64_t)uniform(cdf_int(row, s + 1, scale))) >> 16);
                    }
                }
                if (lane == 0) out(r, s);
                high = (low - 1u) + hi;
                low = low + lo;
                const int n1 = clz32(low ^ high);
                low <<= n1; high = (high << n1) | ((1u << n1) - 1u); value = (value << n1) | in.take((uint32_t)n1);
                const int n2 = min(min(clz32(~(low << 1)), clz32(high << 1)), 31);
                low = (low << n2) & (n2 ? 0x7FFFFFFFu : 0xFFFFFFFFu);
                high = (high << n2) | (n2 ? 0x80000000u : 0u) | ((1u << n2) - 1u);
                value = ((value << n2) ^ (n2 ? 0x80000000u : 0u)) | in.take((uint32_t)n2);
                // the coder's state is wave-uniform; saying so keeps it (and the arithmetic above) in scalar registers
                low = uniform(low); high = uniform(high); value = uniform(value);
            }
        }
    }
}

template <typename CT>
__global__ __launch_bounds__(64) void k_hac_decode(const CT cdf, const uint8_t *__restrict__ bytes, const int32_t *__restrict__ cnt,
                                                   const uint32_t *__restrict__ cnt_cum, int16_t *__restrict__ sym, int64_t n, int lp, int chunk)
{
    const int c = blockIdx.x;
    const int64_t base = (int64_t)c * chunk;
    hac_decode_chunk(cdf, bytes + uniform(cnt_cum[c]), uniform((uint32_t)cnt[c]), base, (int)min((int64_t)chunk, n - base), lp,
                     [&](int64_t r, int s) { sym[r] = (int16_t)s; });
}

// The same for MANY slices at once (every 3000-anchor slice of an attribute has its own symbol range [min, max], hence
// its own alphabet): one wave per chunk of any slice, CDF entries from the element's Gaussian parameters, the decoded
// value (sym + min) * Q written directly (encodings_cuda.py:431-432).
struct SliceChunk { int64_t base; int32_t n, slice; uint32_t byte_off, nbytes; };
// CT = GaussTable (HAC) or MixTable (HAC++'s mixture: the feat groups); its min_value is the slice's
template <typename CT>
__global__ __launch_bounds__(64) void k_hac_decode_slices(CT table, const SliceChunk *__restrict__ chunks, const int32_t *__restrict__ smin,
                                                          const int32_t *__restrict__ slp, const uint8_t *__restrict__ bytes, float *__restrict__ x)
{
    // (the chunk record comes in through a vector load; as scalars, the chunk's loop bounds, the bit reader and the coder's range are wave-uniform
    //  for the compiler too and run on the scalar unit)
    const SliceChunk ch = chunks[blockIdx.x];
    const int slice = (int)uniform((uint32_t)ch.slice);
    const int mn = (int)uniform((uint32_t)smin[slice]);
    table.min_value = mn;
    const float *__restrict__ q = table.q;
    hac_decode_chunk(table, bytes + uniform(ch.byte_off), uniform(ch.nbytes), uniform64(ch.base), (int)uniform((uint32_t)ch.n), (int)uniform((uint32_t)slp[slice]),
                     [&](int64_t r, int s) { x[r] = ((float)s + (float)mn) * q[r]; });
}

}  // namespace

extern "C" int gsac_calculate_cdf(gpcc_ctx *ctx, const float *mean, const float *scale, const float *Q, int64_t n, int min_value, int max_value,
                                  float *lower, void *stream)
{
    if (!ctx || !mean || !scale || !Q || !lower) return fail(GPCC_ERR_ARG, "null argument");
    if (n <= 0) return GPCC_OK;
    const int lp = max_value - min_value + 2;
    if (lp < 2) return fail(GPCC_ERR_ARG, "max_value < min_value");
    HIP_TRY(hipSetDevice(ctx->device));
    k_gaussian_cdf<<<(unsigned)cdiv(n * lp, TB), TB, 0, (hipStream_t)stream>>>(mean, scale, Q, n, min_value, lp, lower);
    LAUNCH_CHECK();
    return GPCC_OK;
}

// The tail of every encoder here, from the packed (low, high) words to the caller's pointers: lane-per-chunk coder, compaction, chunk byte counts
// and payload into the pinned buffers.  The slices encoder also gets its (min, max) table back between the two synchronisations (mm: 2 * nslices
// ints on the device; nullptr for a single stream).
// (declared in coder_tail.hpp: the latent coder of arm_codec.hip ends in it too)
int encode_tail(gpcc_ctx *ctx, hipStream_t st, const uint32_t *lohi, const RcChunk *dch, int nch, uint8_t *scratch, uint32_t sstride, uint32_t *dcnt,
                uint32_t *doff, uint8_t *payload, CoderOut out, const int32_t *mm, int nslices, float *min_out, float *max_out)
{
    GP_TRY(rc_encode_launch(st, lohi, dch, nch, scratch, sstride, dcnt));
    GP_TRY(exclusive_scan_u32(ctx, st, dcnt, doff, nch, doff + nch));
    GP_TRY(rc_compact_launch(st, scratch, sstride, dcnt, doff, nullptr, nch, payload));
    GP_TRY(ctx->hstage.reserve(4 * (size_t)nch + 8 * (size_t)nslices + 64));
    uint32_t *hcnt = reinterpret_cast<uint32_t *>(ctx->hstage.p);
    int32_t *hmm = reinterpret_cast<int32_t *>(hcnt + nch + 1);
    HIP_TRY(hipMemcpyAsync(hcnt, dcnt, 4 * (size_t)nch, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hcnt + nch, doff + nch, 4, hipMemcpyDeviceToHost, st));
    if (mm) HIP_TRY(hipMemcpyAsync(hmm, mm, 8 * (size_t)nslices, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    GP_TRY(device_error_check(ctx));
    for (int s = 0; s < nslices; ++s) {
        if (hmm[2 * s + 1] - hmm[2 * s] + 2 > 32767) return fail(GPCC_ERR_RANGE, "slice %d: quantised values span %d levels (int16 symbols)", s, hmm[2 * s + 1] - hmm[2 * s] + 1);
        min_out[s] = (float)hmm[2 * s]; max_out[s] = (float)hmm[2 * s + 1];
    }
    const size_t total = hcnt[nch];
    GP_TRY(ctx->hbytes.reserve(total + 16));
    if (total) HIP_TRY(hipMemcpyAsync(ctx->hbytes.p, payload, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out.bytes = ctx->hbytes.p; *out.nbytes = (int64_t)total;
    *out.cnt = reinterpret_cast<const int32_t *>(hcnt); *out.nchunks = nch;
    return GPCC_OK;
}

template <typename CT>
static int gsac_encode_impl(gpcc_ctx *ctx, const int16_t *sym, CT cdf, int chunk_size, int64_t n, int lp, CoderOut out, void *stream, bool keep_arena = false)
{
    if (!ctx || !sym || out.null()) return fail(GPCC_ERR_ARG, "null argument");
    if (n <= 0 || chunk_size <= 0 || lp < 2) return fail(GPCC_ERR_ARG, "bad size");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int nch = (int)cdiv(n, chunk_size);
    const uint32_t sstride = rc_scratch_stride((uint32_t)std::min<int64_t>(chunk_size, n));
    if (!keep_arena) {
        GP_TRY(ctx->arena.reserve((size_t)nch * chunk_size * 4 + 2 * (size_t)nch * sstride + (size_t)nch * 64 + ((size_t)4 << 20)));
        ctx->arena.reset();
    }
    std::vector<RcChunk> chunks((size_t)nch);
    for (int c = 0; c < nch; ++c) chunks[(size_t)c] = RcChunk{(uint32_t)c, (uint32_t)nch, (uint32_t)std::min<int64_t>(chunk_size, n - (int64_t)c * chunk_size), 0, 0, 0};
    TAKE(lohi, uint32_t, (int64_t)nch * chunk_size); TAKE(dch, RcChunk, nch); TAKE(dcnt, uint32_t, nch + 1); TAKE(doff, uint32_t, nch + 1);
    TAKE(scratch, uint8_t, (size_t)nch * sstride); TAKE(payload, uint8_t, (size_t)nch * sstride);
    HIP_TRY(hipMemcpyAsync(dch, chunks.data(), sizeof(RcChunk) * (size_t)nch, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    k_hac_pack<CT><<<(unsigned)cdiv(n, TB), TB, 0, st>>>(cdf, sym, n, lp, chunk_size, (uint32_t)nch, lohi);
    LAUNCH_CHECK();
    return encode_tail(ctx, st, lohi, dch, nch, scratch, sstride, dcnt, doff, payload, out);
}

extern "C" int gsac_encode(gpcc_ctx *ctx, const int16_t *sym, const float *cdf, int chunk_size, int64_t n, int lp, const uint8_t **bytes_out,
                           int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    if (!cdf) return fail(GPCC_ERR_ARG, "null argument");
    return gsac_encode_impl<const float *>(ctx, sym, cdf, chunk_size, n, lp, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

// the same with ONE row for all symbols (lp <= 4 entries, e.g. (0, 1 - p, 1) for a Bernoulli source): byte-identical to gsac_encode on the table that
// repeats the row n times
extern "C" int gsac_encode_const(gpcc_ctx *ctx, const int16_t *sym, const float *row_host, int chunk_size, int64_t n, int lp, const uint8_t **bytes_out,
                                 int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    if (!row_host || lp < 2 || lp > 4) return fail(GPCC_ERR_ARG, "constant-row coder: 2 <= lp <= 4");
    ConstTable t = {};
    for (int i = 0; i < lp; ++i) t.c[i] = row_host[i];
    return gsac_encode_impl<ConstTable>(ctx, sym, t, chunk_size, n, lp, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

extern "C" int gsac_encode_u16(gpcc_ctx *ctx, const int16_t *sym, const uint16_t *cdf, int chunk_size, int64_t n, int lp, const uint8_t **bytes_out,
                               int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    if (!cdf) return fail(GPCC_ERR_ARG, "null argument");
    return gsac_encode_impl<const uint16_t *>(ctx, sym, cdf, chunk_size, n, lp, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

template <typename CT>
static int gsac_decode_impl(gpcc_ctx *ctx, CT cdf, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, int64_t n, int lp,
                           int16_t *sym_out, void *stream, bool keep_arena = false)
{
    if (!ctx || !bytes || !cnt || !sym_out) return fail(GPCC_ERR_ARG, "null argument");
    if (n <= 0 || chunk_size <= 0 || lp < 2) return fail(GPCC_ERR_ARG, "bad size");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int nch = (int)cdiv(n, chunk_size);
    if (nbytes < 0 || nbytes >= ((int64_t)1 << 32)) return fail(GPCC_ERR_FORMAT, "byte stream must be shorter than 4 GiB");
    std::vector<uint32_t> cum((size_t)nch + 1, 0);
    {
        uint64_t run = 0;   // the counts come from a file: summed in 64 bits, checked chunk by chunk (a wrapped 32-bit sum would pass)
        for (int c = 0; c < nch; ++c) {
            if (cnt[c] < 0) return fail(GPCC_ERR_FORMAT, "negative chunk size");
            run += (uint64_t)cnt[c];
            if (run > (uint64_t)nbytes) return fail(GPCC_ERR_FORMAT, "chunk sizes exceed the byte stream");
            cum[(size_t)c + 1] = (uint32_t)run;
        }
    }
    if (!keep_arena) {
        GP_TRY(ctx->arena.reserve((size_t)nbytes + 8 * (size_t)nch + ((size_t)4 << 20)));
        ctx->arena.reset();
    }
    TAKE(db, uint8_t, nbytes + 16); TAKE(dcnt, int32_t, nch); TAKE(dcum, uint32_t, nch + 1);
    HIP_TRY(hipMemcpyAsync(db, bytes, (size_t)nbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dcnt, cnt, 4 * (size_t)nch, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dcum, cum.data(), 4 * ((size_t)nch + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    k_hac_decode<CT><<<(unsigned)nch, 64, 0, st>>>(cdf, db, dcnt, dcum, sym_out, n, lp, chunk_size);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}

extern "C" int gsac_decode(gpcc_ctx *ctx, const float *cdf, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, int64_t n, int lp,
                           int16_t *sym_out, void *stream)
{
    if (!cdf) return fail(GPCC_ERR_ARG, "null argument");
    return gsac_decode_impl<const float *>(ctx, cdf, bytes, nbytes, cnt, chunk_size, n, lp, sym_out, stream);
}

extern "C" int gsac_decode_const(gpcc_ctx *ctx, const float *row_host, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, int64_t n, int lp,
                                 int16_t *sym_out, void *stream)
{
    if (!row_host || lp < 2 || lp > 4) return fail(GPCC_ERR_ARG, "constant-row coder: 2 <= lp <= 4");
    ConstTable t = {};
    for (int i = 0; i < lp; ++i) t.c[i] = row_host[i];
    return gsac_decode_impl<ConstTable>(ctx, t, bytes, nbytes, cnt, chunk_size, n, lp, sym_out, stream);
}

extern "C" int gsac_decode_u16(gpcc_ctx *ctx, const uint16_t *cdf, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, int64_t n, int lp,
                               int16_t *sym_out, void *stream)
{
    if (!cdf) return fail(GPCC_ERR_ARG, "null argument");
    return gsac_decode_impl<const uint16_t *>(ctx, cdf, bytes, nbytes, cnt, chunk_size, n, lp, sym_out, stream);
}


// ------------------------------------------------------------------ fused Gaussian coder (no CDF table)
namespace {
// min / max over the block: the 64 lanes of every wave, then the waves; thread 0 hands the result to `done`
template <class F> __device__ __forceinline__ void block_minmax(int mn, int mx, F done)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { mn = min(mn, __shfl_xor(mn, d, 64)); mx = max(mx, __shfl_xor(mx, d, 64)); }
    __shared__ int red[TB / 64][2];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = mn; red[threadIdx.x >> 6][1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TB / 64; ++w) { mn = min(mn, red[w][0]); mx = max(mx, red[w][1]); }
        done(mn, mx);
    }
}
// x_int = round(x / Q) (torch.round: half to even), its min / max over the slice (encodings_cuda.py:343-345)
__global__ __launch_bounds__(TB) void k_quantise_minmax(const float *__restrict__ x, const float *__restrict__ q, int64_t n, int32_t *__restrict__ xi, int32_t *__restrict__ mm)
{
    int mn = INT32_MAX, mx = INT32_MIN;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
        const int v = (int)__builtin_rintf(x[i] / q[i]);
        xi[i] = v;
        mn = min(mn, v); mx = max(mx, v);
    }
    block_minmax(mn, mx, [&](int mn, int mx) { atomicMin(&mm[0], mn); atomicMax(&mm[1], mx); });
}
__global__ __launch_bounds__(TB) void k_to_symbols(const int32_t *__restrict__ xi, int64_t n, int min_value, int16_t *__restrict__ sym)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) sym[i] = (int16_t)(xi[i] - min_value);
}
// x = (sym + min) * Q (encodings_cuda.py:431-432)
__global__ __launch_bounds__(TB) void k_from_symbols(const int16_t *__restrict__ sym, const float *__restrict__ q, int64_t n, float min_value, float *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) x[i] = ((float)sym[i] + min_value) * q[i];
}
}  // namespace

static int mix_table(const float *const *mean, const float *const *scale, const float *const *prob, int k, const float *Q, int min_value, MixTable *t)
{
    if (!mean || !scale || !prob || !Q) return fail(GPCC_ERR_ARG, "null argument");
    if (k < 1 || k > MIX_MAX) return fail(GPCC_ERR_ARG, "a mixture has 1..%d components", MIX_MAX);
    *t = MixTable{};
    for (int i = 0; i < k; ++i) {
        if (!mean[i] || !scale[i] || !prob[i]) return fail(GPCC_ERR_ARG, "null argument");
        t->mean[i] = mean[i]; t->scale[i] = scale[i]; t->prob[i] = prob[i];
    }
    t->q = Q; t->k = k; t->min_value = min_value;
    return GPCC_OK;
}


// encoder_gaussian / HAC++'s encoder_gaussian_mixed without the (n, max - min + 2) table (encodings_cuda.py:336-371, HAC-plus/utils/
// encodings_cuda.py:205-247): quantise, min / max, symbols, then the coder on the rows of `table` (GaussTable or MixTable; its min_value is set here)
template <typename CT>
static int encode_gaussian_impl(gpcc_ctx *ctx, const float *x, CT table, const float *Q, int64_t n, int chunk_size, float *min_out, float *max_out, CoderOut out,
                                void *stream)
{
    if (!ctx || !x || !Q || !min_out || !max_out) return fail(GPCC_ERR_ARG, "null argument");
    if (n <= 0 || chunk_size <= 0) return fail(GPCC_ERR_ARG, "bad size");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int nch = (int)cdiv(n, chunk_size);
    const uint32_t sstride = rc_scratch_stride((uint32_t)std::min<int64_t>(chunk_size, n));
    GP_TRY(ctx->arena.reserve((size_t)n * 8 + (size_t)nch * chunk_size * 4 + 2 * (size_t)nch * sstride + (size_t)nch * 64 + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(xi, int32_t, n); TAKE(sym, int16_t, n); TAKE(mm, int32_t, 2);
    const int32_t init[2] = {INT32_MAX, INT32_MIN};
    HIP_TRY(hipMemcpyAsync(mm, init, 8, hipMemcpyHostToDevice, st));
    k_quantise_minmax<<<(unsigned)std::min<int64_t>(cdiv(n, TB), 512), TB, 0, st>>>(x, Q, n, xi, mm);
    LAUNCH_CHECK();
    int32_t hmm[2];
    HIP_TRY(hipMemcpyAsync(hmm, mm, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int lp = hmm[1] - hmm[0] + 2;
    // (the reference clamps the symbol to 32767, HAC-plus :227-228, and would then need a table of more than 32767 columns per element)
    if (lp > 32767) return fail(GPCC_ERR_RANGE, "quantised values span %d levels (int16 symbols)", lp - 1);
    k_to_symbols<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(xi, n, hmm[0], sym);
    LAUNCH_CHECK();
    *min_out = (float)hmm[0]; *max_out = (float)hmm[1];
    table.min_value = hmm[0];
    return gsac_encode_impl<CT>(ctx, sym, table, chunk_size, n, lp, out, stream, true);
}

// ... and decoder_gaussian / decoder_gaussian_mixed (encodings_cuda.py:399-433, HAC-plus :271-317)
template <typename CT>
static int decode_gaussian_impl(gpcc_ctx *ctx, CT table, const float *Q, int64_t n, float min_value, float max_value, const uint8_t *bytes, int64_t nbytes,
                                const int32_t *cnt, int chunk_size, float *x_out, void *stream)
{
    if (!ctx || !Q || !x_out) return fail(GPCC_ERR_ARG, "null argument");
    if (n <= 0 || chunk_size <= 0) return fail(GPCC_ERR_ARG, "bad size");
    int lp;
    GP_TRY(symbol_range(min_value, max_value, &table.min_value, &lp));
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int nch = (int)cdiv(n, chunk_size);
    GP_TRY(ctx->arena.reserve((size_t)n * 2 + (size_t)nbytes + 8 * (size_t)nch + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(sym, int16_t, n);
    GP_TRY(gsac_decode_impl<CT>(ctx, table, bytes, nbytes, cnt, chunk_size, n, lp, sym, stream, true));
    k_from_symbols<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(sym, Q, n, min_value, x_out);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}

extern "C" int gsac_encode_gaussian(gpcc_ctx *ctx, const float *x, const float *mean, const float *scale, const float *Q, int64_t n, int chunk_size,
                                    float *min_out, float *max_out, const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out,
                                    int64_t *nchunks_out, void *stream)
{
    if (!mean || !scale) return fail(GPCC_ERR_ARG, "null argument");
    return encode_gaussian_impl(ctx, x, GaussTable{mean, scale, Q, 0}, Q, n, chunk_size, min_out, max_out, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

extern "C" int gsac_decode_gaussian(gpcc_ctx *ctx, const float *mean, const float *scale, const float *Q, int64_t n, float min_value, float max_value,
                                    const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, float *x_out, void *stream)
{
    if (!mean || !scale) return fail(GPCC_ERR_ARG, "null argument");
    return decode_gaussian_impl(ctx, GaussTable{mean, scale, Q, 0}, Q, n, min_value, max_value, bytes, nbytes, cnt, chunk_size, x_out, stream);
}

extern "C" int gsac_encode_gaussian_mixed(gpcc_ctx *ctx, const float *x, const float *const *mean, const float *const *scale, const float *const *prob, int k,
                                          const float *Q, int64_t n, int chunk_size, float *min_out, float *max_out, const uint8_t **bytes_out,
                                          int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    MixTable t;
    GP_TRY(mix_table(mean, scale, prob, k, Q, 0, &t));
    return encode_gaussian_impl(ctx, x, t, Q, n, chunk_size, min_out, max_out, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

extern "C" int gsac_decode_gaussian_mixed(gpcc_ctx *ctx, const float *const *mean, const float *const *scale, const float *const *prob, int k, const float *Q,
                                          int64_t n, float min_value, float max_value, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size,
                                          float *x_out, void *stream)
{
    MixTable t;
    GP_TRY(mix_table(mean, scale, prob, k, Q, 0, &t));
    return decode_gaussian_impl(ctx, t, Q, n, min_value, max_value, bytes, nbytes, cnt, chunk_size, x_out, stream);
}

// the mixture's CDF table itself: lower (n, max - min + 2), as HAC++ builds it before arithmetic_encode (:210-225)
extern "C" int gsac_calculate_cdf_mixed(gpcc_ctx *ctx, const float *const *mean, const float *const *scale, const float *const *prob, int k, const float *Q,
                                        int64_t n, int min_value, int max_value, float *lower, void *stream)
{
    if (!ctx || !lower) return fail(GPCC_ERR_ARG, "null argument");
    const int64_t lp = (int64_t)max_value - min_value + 2;
    if (n <= 0 || lp < 2 || lp > 32767) return fail(GPCC_ERR_ARG, "bad size");
    MixTable t;
    GP_TRY(mix_table(mean, scale, prob, k, Q, min_value, &t));
    HIP_TRY(hipSetDevice(ctx->device));
    k_mixture_cdf<<<(unsigned)cdiv(n * lp, TB), TB, 0, (hipStream_t)stream>>>(t, n, (int)lp, lower);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return GPCC_OK;
}

// ------------------------------------------------------------------ all slices of an attribute in one call
namespace {
constexpr int SLICE_PARTS = 8;   // blocks per slice in the min / max pass

__device__ __forceinline__ int slice_of(const int64_t *__restrict__ start, int nslices, int64_t r)
{
    int lo = 0, hi = nslices;           // start[lo] <= r < start[hi]
    while (lo + 1 < hi) { const int m = (lo + hi) >> 1; if (start[m] <= r) lo = m; else hi = m; }
    return lo;
}

// x_int = round(x / Q) and the min / max of every slice: block (part, slice)
__global__ __launch_bounds__(TB) void k_quantise_minmax_slices(const float *__restrict__ x, const float *__restrict__ q, const int64_t *__restrict__ start,
                                                               int32_t *__restrict__ xi, int32_t *__restrict__ mm)
{
    const int s = blockIdx.y;
    const int64_t a = start[s], b = start[s + 1], len = b - a;
    const int64_t lo = a + len * blockIdx.x / SLICE_PARTS, hi = a + len * (blockIdx.x + 1) / SLICE_PARTS;
    int mn = INT32_MAX, mx = INT32_MIN;
    for (int64_t i = lo + threadIdx.x; i < hi; i += TB) {
        const int v = (int)__builtin_rintf(x[i] / q[i]);
        xi[i] = v;
        mn = min(mn, v); mx = max(mx, v);
    }
    block_minmax(mn, mx, [&](int mn, int mx) { if (hi > lo) { atomicMin(&mm[2 * s], mn); atomicMax(&mm[2 * s + 1], mx); } });
}

// (symbol, Gaussian parameters) -> the coder's two integers, in the chunk-interleaved layout of the element's slice
template <typename CT>
__global__ __launch_bounds__(TB) void k_hac_pack_slices(CT table, const int32_t *__restrict__ xi, int64_t n, const int64_t *__restrict__ start, int nslices,
                                                        const int32_t *__restrict__ mm, const int64_t *__restrict__ lohi_base,
                                                        const int32_t *__restrict__ slice_nch, int chunk, uint32_t *__restrict__ lohi)
{
    const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (r >= n) return;
    const int sl = slice_of(start, nslices, r);
    const int mn = mm[2 * sl], lp = mm[2 * sl + 1] - mn + 2;
    const float sc = (float)(65536 - (lp - 1));
    const int s = xi[r] - mn;
    table.min_value = mn;
    const auto row = row_of(table, r, lp);
    const uint32_t lo = cdf_int(row, s, sc);
    const uint32_t hi = s == lp - 2 ? 0x10000u : cdf_int(row, s + 1, sc);
    const int64_t e = r - start[sl];
    const int64_t c = e / chunk, t = e - c * chunk;
    lohi[lohi_base[sl] + t * slice_nch[sl] + c] = (lo & 0xFFFFu) | ((hi - 1u) << 16);
}
}  // namespace

// STREAM_MAX_SYMS: the longest slice of the stream form below (chunk = slice).  What depends on a chunk's length: RcChunk::n and SliceChunk::n
// (32 bits), rc_scratch_stride (2 n + 47 in 32 bits), the chunk's byte count and offset (uint32) and WaveBits::rem (int32) -- all hold below 2^30 symbols.
constexpr int64_t STREAM_MAX_SYMS = (int64_t)1 << 30;

// streams: the slice form whose unit is ONE carry-less stream per slice (TC-GS / CAT-3DGS's torchac files).  chunk_size is ignored and set to the
// longest slice, so every non-empty slice is one chunk: the packed-word buffer holds `longest` words per slice and the scratch stride is the longest
// slice's.  A slice may be empty: it gets no chunk, min = max = 0 and a byte count of 0; cnt has ONE entry per slice.
template <typename CT>
static int encode_slices_impl(gpcc_ctx *ctx, const float *x, CT table, const float *Q, const int64_t *slice_start,
                              int nslices, int chunk_size, float *min_out, float *max_out, CoderOut out, void *stream, bool streams = false)
{
    if (!ctx || !x || !Q || !slice_start || !min_out || !max_out || out.null()) return fail(GPCC_ERR_ARG, "null argument");
    if (nslices <= 0 || (!streams && chunk_size <= 0)) return fail(GPCC_ERR_ARG, "bad size");
    for (int s = 0; s < nslices; ++s)
        if (streams ? slice_start[s + 1] < slice_start[s] : slice_start[s + 1] <= slice_start[s]) return fail(GPCC_ERR_ARG, "slice %d is empty", s);
    if (slice_start[0] != 0) return fail(GPCC_ERR_ARG, "slices must start at element 0");
    const int64_t n = slice_start[nslices];
    if (streams) {
        int64_t longest = 1;
        for (int s = 0; s < nslices; ++s) longest = std::max(longest, slice_start[s + 1] - slice_start[s]);
        if (longest >= STREAM_MAX_SYMS) return fail(GPCC_ERR_ARG, "a stream of %lld symbols (at most 2^30 - 1)", (long long)longest);
        if (nslices > 65535) return fail(GPCC_ERR_ARG, "%d streams in one call (at most 65535: a grid row per slice): split the call", nslices);
        // the payload's offsets are uint32 (exclusive_scan_u32, RcChunk): a call whose streams could exceed 4 GiB is split by the caller
        // (gauspcc_amd.torchac_encodings.encoder_gaussian_slices cuts the slice list); 3 000 streams of 50 000 symbols are bounded by 0.3 GB
        if ((uint64_t)nslices * rc_scratch_stride((uint32_t)longest) >= ((uint64_t)1 << 32))
            return fail(GPCC_ERR_ARG, "%d streams of up to %lld symbols may exceed 4 GiB: split the call", nslices, (long long)longest);
        chunk_size = (int)longest;
        if (n == 0) {   // nothing but empty slices
            ctx->stream_cnt.assign((size_t)nslices, 0);
            for (int s = 0; s < nslices; ++s) min_out[s] = max_out[s] = 0.0f;
            GP_TRY(ctx->hbytes.reserve(16));
            *out.bytes = ctx->hbytes.p; *out.nbytes = 0; *out.cnt = ctx->stream_cnt.data(); *out.nchunks = nslices;
            return GPCC_OK;
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // chunk descriptors: slice by slice, the chunks of a slice interleaved among themselves
    std::vector<RcChunk> chunks;
    std::vector<int64_t> lbase((size_t)nslices);
    std::vector<int32_t> snch((size_t)nslices);
    int64_t slots = 0;
    uint32_t max_syms = 1;
    for (int s = 0; s < nslices; ++s) {
        const int64_t len = slice_start[s + 1] - slice_start[s];
        const int nch = (int)cdiv(len, chunk_size);
        lbase[(size_t)s] = slots; snch[(size_t)s] = nch;
        for (int c = 0; c < nch; ++c) {
            const uint32_t cn = (uint32_t)std::min<int64_t>(chunk_size, len - (int64_t)c * chunk_size);
            chunks.push_back(RcChunk{(uint32_t)(slots + c), (uint32_t)nch, cn, 0, 0, 0});
            max_syms = std::max(max_syms, cn);
        }
        slots += (int64_t)nch * chunk_size;
    }
    if (slots >= ((int64_t)1 << 32)) return fail(GPCC_ERR_ARG, "too many symbols in one call");
    const int nch = (int)chunks.size();
    const uint32_t sstride = rc_scratch_stride(max_syms);
    GP_TRY(ctx->arena.reserve((size_t)n * 4 + (size_t)slots * 4 + 2 * (size_t)nch * sstride + (size_t)nch * 64 + (size_t)nslices * 32 + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(xi, int32_t, n); TAKE(mm, int32_t, 2 * nslices); TAKE(dstart, int64_t, nslices + 1); TAKE(dlbase, int64_t, nslices); TAKE(dsnch, int32_t, nslices);
    TAKE(lohi, uint32_t, slots); TAKE(dch, RcChunk, nch); TAKE(dcnt, uint32_t, nch + 1); TAKE(doff, uint32_t, nch + 1);
    TAKE(scratch, uint8_t, (size_t)nch * sstride); TAKE(payload, uint8_t, (size_t)nch * sstride);
    std::vector<int32_t> init((size_t)2 * nslices);
    for (int s = 0; s < nslices; ++s) {
        const bool empty = slice_start[s + 1] == slice_start[s];    // (stream form only) no element touches the pair: min = max = 0
        init[(size_t)2 * s] = empty ? 0 : INT32_MAX; init[(size_t)2 * s + 1] = empty ? 0 : INT32_MIN;
    }
    HIP_TRY(hipMemcpyAsync(mm, init.data(), 8 * (size_t)nslices, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dstart, slice_start, 8 * ((size_t)nslices + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dlbase, lbase.data(), 8 * (size_t)nslices, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dsnch, snch.data(), 4 * (size_t)nslices, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dch, chunks.data(), sizeof(RcChunk) * (size_t)nch, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope before the stream drains otherwise
    k_quantise_minmax_slices<<<dim3(SLICE_PARTS, (unsigned)nslices), TB, 0, st>>>(x, Q, dstart, xi, mm);
    LAUNCH_CHECK();
    k_hac_pack_slices<CT><<<(unsigned)cdiv(n, TB), TB, 0, st>>>(table, xi, n, dstart, nslices, mm, dlbase, dsnch, chunk_size, lohi);
    LAUNCH_CHECK();
    if (!streams) return encode_tail(ctx, st, lohi, dch, nch, scratch, sstride, dcnt, doff, payload, out, mm, nslices, min_out, max_out);
    // the tail counts the chunks, that is the non-empty slices; one count per SLICE goes into a buffer of the context's own
    GP_TRY(encode_tail(ctx, st, lohi, dch, nch, scratch, sstride, dcnt, doff, payload, out, mm, nslices, min_out, max_out));
    const int32_t *per_chunk = *out.cnt;
    ctx->stream_cnt.resize((size_t)nslices);
    for (int s = 0, c = 0; s < nslices; ++s) ctx->stream_cnt[(size_t)s] = slice_start[s + 1] > slice_start[s] ? per_chunk[c++] : 0;
    *out.cnt = ctx->stream_cnt.data(); *out.nchunks = nslices;
    return GPCC_OK;
}

extern "C" int gsac_encode_gaussian_slices(gpcc_ctx *ctx, const float *x, const float *mean, const float *scale, const float *Q, const int64_t *slice_start,
                                           int nslices, int chunk_size, float *min_out, float *max_out, const uint8_t **bytes_out, int64_t *nbytes_out,
                                           const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    if (!mean || !scale) return fail(GPCC_ERR_ARG, "null argument");
    return encode_slices_impl(ctx, x, GaussTable{mean, scale, Q, 0}, Q, slice_start, nslices, chunk_size, min_out, max_out, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

// HAC++: the slices of ONE channel group of `feat` under the two-component mixture (HAC-plus/scene/gaussian_model.py:1306-1321)
extern "C" int gsac_encode_gaussian_mixed_slices(gpcc_ctx *ctx, const float *x, const float *const *mean, const float *const *scale, const float *const *prob, int k,
                                                 const float *Q, const int64_t *slice_start, int nslices, int chunk_size, float *min_out, float *max_out,
                                                 const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    MixTable t;
    GP_TRY(mix_table(mean, scale, prob, k, Q, 0, &t));
    return encode_slices_impl(ctx, x, t, Q, slice_start, nslices, chunk_size, min_out, max_out, CoderOut{bytes_out, nbytes_out, cnt_out, nchunks_out}, stream);
}

template <typename CT>
static int decode_slices_impl(gpcc_ctx *ctx, CT table, const float *Q, const int64_t *slice_start, int nslices,
                              const float *min_value, const float *max_value, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt,
                              int chunk_size, float *x_out, void *stream, bool streams = false)
{
    // (streams: one chunk per slice whatever its length, ONE count per slice, empty slices allowed -- see encode_slices_impl; the bytes may be empty)
    if (!ctx || !Q || !slice_start || !min_value || !max_value || (!bytes && !(streams && nbytes == 0)) || !cnt || !x_out) return fail(GPCC_ERR_ARG, "null argument");
    if (nslices <= 0 || (!streams && chunk_size <= 0) || slice_start[0] != 0 || nbytes < 0) return fail(GPCC_ERR_ARG, "bad size");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<SliceChunk> chunks;
    std::vector<int32_t> smin((size_t)nslices), slp((size_t)nslices);
    uint64_t off = 0;
    for (int s = 0; s < nslices; ++s) {
        const int64_t len = slice_start[s + 1] - slice_start[s];
        if (streams) {
            if (len < 0 || len >= STREAM_MAX_SYMS) return fail(GPCC_ERR_ARG, "slice %d: %lld symbols", s, (long long)len);
            if (cnt[s] < 0) return fail(GPCC_ERR_FORMAT, "negative stream size");
            smin[(size_t)s] = 0; slp[(size_t)s] = 2;
            if (len > 0) {
                if (symbol_range(min_value[s], max_value[s], &smin[(size_t)s], &slp[(size_t)s]) != GPCC_OK) return fail(GPCC_ERR_FORMAT, "slice %d: bad symbol range", s);
                chunks.push_back(SliceChunk{slice_start[s], (int32_t)len, s, (uint32_t)off, (uint32_t)cnt[s]});
            }
            off += (uint32_t)cnt[s];
            if ((int64_t)off > nbytes || off >= ((uint64_t)1 << 32)) return fail(GPCC_ERR_FORMAT, "stream sizes exceed the byte stream");
            continue;
        }
        if (len <= 0) return fail(GPCC_ERR_ARG, "slice %d is empty", s);
        if (symbol_range(min_value[s], max_value[s], &smin[(size_t)s], &slp[(size_t)s]) != GPCC_OK) return fail(GPCC_ERR_FORMAT, "slice %d: bad symbol range", s);
        const int nch = (int)cdiv(len, chunk_size);
        for (int c = 0; c < nch; ++c) {
            const int32_t cb = cnt[chunks.size()];
            if (cb < 0) return fail(GPCC_ERR_FORMAT, "negative chunk size");
            chunks.push_back(SliceChunk{slice_start[s] + (int64_t)c * chunk_size, (int32_t)std::min<int64_t>(chunk_size, len - (int64_t)c * chunk_size), s,
                                        (uint32_t)off, (uint32_t)cb});
            off += (uint32_t)cb;
            if ((int64_t)off > nbytes || off >= ((uint64_t)1 << 32)) return fail(GPCC_ERR_FORMAT, "chunk sizes exceed the byte stream");
        }
    }
    const size_t nch = chunks.size();
    if (nch == 0) return GPCC_OK;   // (stream form: nothing but empty slices)
    GP_TRY(ctx->arena.reserve((size_t)nbytes + sizeof(SliceChunk) * nch + 8 * (size_t)nslices + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(db, uint8_t, nbytes + 16); TAKE(dch, SliceChunk, nch); TAKE(dmin, int32_t, nslices); TAKE(dlp, int32_t, nslices);
    if (nbytes) HIP_TRY(hipMemcpyAsync(db, bytes, (size_t)nbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dch, chunks.data(), sizeof(SliceChunk) * nch, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dmin, smin.data(), 4 * (size_t)nslices, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dlp, slp.data(), 4 * (size_t)nslices, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    k_hac_decode_slices<CT><<<(unsigned)nch, 64, 0, st>>>(table, dch, dmin, dlp, db, x_out);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}

extern "C" int gsac_decode_gaussian_slices(gpcc_ctx *ctx, const float *mean, const float *scale, const float *Q, const int64_t *slice_start, int nslices,
                                           const float *min_value, const float *max_value, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt,
                                           int chunk_size, float *x_out, void *stream)
{
    if (!mean || !scale) return fail(GPCC_ERR_ARG, "null argument");
    return decode_slices_impl(ctx, GaussTable{mean, scale, Q, 0}, Q, slice_start, nslices, min_value, max_value, bytes, nbytes, cnt, chunk_size, x_out, stream);
}

extern "C" int gsac_decode_gaussian_mixed_slices(gpcc_ctx *ctx, const float *const *mean, const float *const *scale, const float *const *prob, int k, const float *Q,
                                                 const int64_t *slice_start, int nslices, const float *min_value, const float *max_value, const uint8_t *bytes,
                                                 int64_t nbytes, const int32_t *cnt, int chunk_size, float *x_out, void *stream)
{
    MixTable t;
    GP_TRY(mix_table(mean, scale, prob, k, Q, 0, &t));
    return decode_slices_impl(ctx, t, Q, slice_start, nslices, min_value, max_value, bytes, nbytes, cnt, chunk_size, x_out, stream);
}

// ------------------------------------------------------------------ TC-GS / CAT-3DGS: one torchac stream per slice, no table
namespace {
// the integer rows themselves: torchac's _convert_to_int_and_normalize of the float table, all lp entries (the coder never reads the last one)
__global__ __launch_bounds__(TB) void k_normal_rows(NormalTable t, int64_t n, int lp, uint16_t *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n * lp) return;
    const int64_t idx = i / lp;
    rows[i] = (uint16_t)cdf_int(row_of(t, idx, lp), (int)(i - idx * lp), (float)(65536 - (lp - 1)));
}
// parameters no Normal takes: bit 0 a mean that is not finite, bit 1 a scale that is not finite or not positive, bit 2 a step that is not finite or zero
__global__ __launch_bounds__(TB) void k_normal_check(NormalTable t, int64_t n, uint32_t *__restrict__ flags)
{
    uint32_t f = 0u;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
        const float m = t.mean[i], s = t.scale[i], q = t.q[i];
        f |= (isfinite(m) ? 0u : 1u) | (isfinite(s) && s > 0.0f ? 0u : 2u) | (isfinite(q) && q != 0.0f ? 0u : 4u);
    }
    if (f) atomicOr(flags, f);
}
}  // namespace

extern "C" int gsac_normal_cdf_rows(gpcc_ctx *ctx, const float *mean, const float *scale, const float *Q, int64_t n, int min_value, int max_value,
                                    uint16_t *rows, void *stream)
{
    if (!ctx || !mean || !scale || !Q || !rows) return fail(GPCC_ERR_ARG, "null argument");
    const int64_t lp = (int64_t)max_value - min_value + 2;
    if (n < 0 || lp < 2 || lp > 32767) return fail(GPCC_ERR_ARG, "bad size");
    if (n == 0) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    k_normal_rows<<<(unsigned)cdiv(n * lp, TB), TB, 0, (hipStream_t)stream>>>(NormalTable{mean, scale, Q, min_value}, n, (int)lp, rows);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return GPCC_OK;
}

extern "C" int gsac_encode_normal_streams(gpcc_ctx *ctx, const float *x, const float *mean, const float *scale, const float *Q, const int64_t *slice_start,
                                          int nslices, float *min_out, float *max_out, const uint8_t **bytes_out, int64_t *nbytes_out,
                                          const int32_t **cnt_out, void *stream)
{
    if (!ctx || !mean || !scale || !Q || !slice_start || !cnt_out) return fail(GPCC_ERR_ARG, "null argument");
    if (nslices <= 0 || slice_start[0] != 0 || slice_start[nslices] < 0) return fail(GPCC_ERR_ARG, "bad size");
    const int64_t n = slice_start[nslices];
    const NormalTable t{mean, scale, Q, 0};
    if (n > 0) {
        // the entry function divides by scale and the quantiser by Q: what they cannot take is refused here, before any kernel computes with it
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t st = (hipStream_t)stream;
        GP_TRY(ctx->arena.reserve((size_t)4 << 20));
        ctx->arena.reset();
        TAKE(dflags, uint32_t, 1);
        GP_TRY(ctx->hstage.reserve(64));
        uint32_t *hflags = reinterpret_cast<uint32_t *>(ctx->hstage.p);
        HIP_TRY(hipMemsetAsync(dflags, 0, 4, st));
        k_normal_check<<<(unsigned)std::min<int64_t>(cdiv(n, TB), 1024), TB, 0, st>>>(t, n, dflags);
        LAUNCH_CHECK();
        HIP_TRY(hipMemcpyAsync(hflags, dflags, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (*hflags) return fail(GPCC_ERR_ARG, "normal streams:%s%s%s", (*hflags & 1u) ? " a mean is not finite;" : "", (*hflags & 2u) ? " a scale is not finite or not positive;" : "",
                                 (*hflags & 4u) ? " a step Q is not finite or zero;" : "");
    }
    int64_t nstreams = 0;
    return encode_slices_impl(ctx, x, t, Q, slice_start, nslices, 0, min_out, max_out, CoderOut{bytes_out, nbytes_out, cnt_out, &nstreams}, stream, true);
}

extern "C" int gsac_decode_normal_streams(gpcc_ctx *ctx, const float *mean, const float *scale, const float *Q, const int64_t *slice_start, int nslices,
                                          const float *min_value, const float *max_value, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt,
                                          float *x_out, void *stream)
{
    if (!mean || !scale) return fail(GPCC_ERR_ARG, "null argument");
    return decode_slices_impl(ctx, NormalTable{mean, scale, Q, 0}, Q, slice_start, nslices, min_value, max_value, bytes, nbytes, cnt, 0, x_out, stream, true);
}
