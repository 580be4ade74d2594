// densify.hip -- densification bookkeeping of the HAC family (e.g. HAC/scene/gaussian_model.py:758-775, 914-968):
//   gpcc_densify_stats   one iteration of training_statis, in place, no host synchronisation
//   gpcc_densify_front   adjust_anchor's head: grads_norm = |accum / denom| (NaN -> 0) and offset_mask
//   gpcc_densify_finish  adjust_anchor's tail: the prune mask and the four accumulators of the survivors
//   gpcc_compact_rows    the kept rows of up to 32 float32 matrices, one scan and one launch
//   gpcc_expand_rows     its transpose (the backward of the gather): kept rows back at their positions, zero rows elsewhere, no synchronisation
// The contracts are in include/gauspcc.h.  No float atomics: every destination has exactly one source lane.
//
// gpcc_densify_stats.  The torch sequence finds its destinations with four boolean-mask index operations, each a nonzero() and a wait for the
// host.  Here the two ranks they stand for come from one pair of scans of M + 1 words, M = max(n, v):
//   rv[a] = visible anchors before a, rv[M] = their count;   rs[r] = set selection entries before row r of the (v, k) table, rs[M] = their count
// (k_stats_flags writes the flags and the per-row counts, the scan runs in place, the appended zero turns its last word into the total).
// k_stats_update first compares both totals with v and s.  Only when they agree is any index formed -- then rv[a] < v
// and every filter / grad row is below s by construction -- and otherwise nothing is written but the caller's sticky error words.
//
// Traffic per anchor (K offsets, a fraction p visible, q of the entries selected and passing the filter): 1 B visible + 28 + 4 p B of rank words
// (8 written by k_stats_flags, 8 read and 8 written by the scans, rv[a] and, for a visible anchor, rs[row] read by the update) + p (5 K B opacity
// and selection, the selection read a second time for the row counts, 16 B anchor accumulators read and written) + p q K (1 B filter + 8 B of the
// 12 B grad row + 16 B offset accumulators read and written).  DESIGN.md 4.5 has the bound and what was measured.
#include "primitives.hpp"

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int MAX_MATS = 32;
enum { E_FLAGS = 0, E_NVIS = 1, E_V = 2, E_NSEL = 3, E_S = 4 };   // the sticky error words (gpcc_densify_stats, include/gauspcc.h)

// ------------------------------------------------------------------ gpcc_densify_stats
__global__ __launch_bounds__(TB) void k_stats_flags(const uint8_t *__restrict__ visible, int64_t n, const uint8_t *__restrict__ selection, int64_t v, int k,
                                                    int64_t m1, uint32_t *__restrict__ rv, uint32_t *__restrict__ rs)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= m1) return;
    rv[i] = i < n ? (visible ? visible[i] != 0 : 1u) : 0u;
    uint32_t c = 0;
    if (i < v) {
        const uint8_t *row = selection + i * k;
        for (int j = 0; j < k; ++j) c += row[j] != 0;
    }
    rs[i] = c;
}

// A lane per (anchor, offset): a block holds TB / k whole anchors, so that an anchor's k lanes meet in LDS.  The reads of opacity and selection
// and the read-modify-writes of the offset accumulators are coalesced along the flat index; the lane of offset 0 adds the row's clamped
// opacities in ascending order from LDS, and a selected lane counts the set entries of its row before it there.
__global__ __launch_bounds__(TB) void k_stats_update(const uint8_t *__restrict__ visible, int64_t n, int k, const float *__restrict__ opacity, int64_t v,
                                                     const uint8_t *__restrict__ selection, const uint8_t *__restrict__ filter, int64_t s,
                                                     const float *__restrict__ grad, int64_t gstride, const uint32_t *__restrict__ rv,
                                                     const uint32_t *__restrict__ rs, int64_t m, float *__restrict__ opacity_accum,
                                                     float *__restrict__ anchor_demon, float *__restrict__ grad_accum, float *__restrict__ denom,
                                                     unsigned int *__restrict__ err)
{
    __shared__ float clamped[TB];
    __shared__ uint8_t chosen[TB];
    const int tid = threadIdx.x, rpb = TB / k;
    const int la = tid / k, j = tid - la * k;
    const int64_t a = (int64_t)blockIdx.x * rpb + la;
    const uint32_t nvis = rv[m], nsel = rs[m];
    const bool bad_v = (int64_t)nvis != v, bad_s = (int64_t)nsel != s;
    if (bad_v || bad_s) {   // ill-formed (the same for every lane of the launch): nothing is written, no rank is used
        if (blockIdx.x == 0 && tid == 0) {
            atomicOr(&err[E_FLAGS], (bad_v ? 1u : 0u) | (bad_s ? 2u : 0u));
            err[E_NVIS] = nvis; err[E_V] = (unsigned int)v; err[E_NSEL] = nsel; err[E_S] = (unsigned int)s;
        }
        return;
    }
    const bool act = la < rpb && a < n && (!visible || visible[a]);
    int64_t r = 0;
    float o = 0.0f;
    bool sel = false;
    if (act) {
        r = rv[a];                         // < v: the totals agree
        o = opacity[r * k + j];
        sel = selection[r * k + j] != 0;
    }
    clamped[tid] = o < 0.0f ? 0.0f : o;    // temp_opacity[temp_opacity < 0] = 0: a NaN stays
    chosen[tid] = sel;
    __syncthreads();
    if (!act) return;
    if (sel) {
        int64_t f = rs[r];                 // < s for every set entry of the row
        for (int t = tid - j; t < tid; ++t) f += chosen[t];
        if (filter[f]) {
            const float gx = grad[f * gstride], gy = grad[f * gstride + 1];
            grad_accum[a * k + j] += sqrtf(gx * gx + gy * gy);
            denom[a * k + j] += 1.0f;
        }
    }
    if (j == 0) {
        float sum = 0.0f;
        for (int t = 0; t < k; ++t) sum += clamped[tid + t];
        opacity_accum[a] += sum;
        anchor_demon[a] += 1.0f;
    }
}

// ------------------------------------------------------------------ gpcc_densify_front
__global__ __launch_bounds__(TB) void k_front(const float *__restrict__ grad_accum, const float *__restrict__ denom, int64_t total, float thr,
                                              float *__restrict__ grads_norm, uint8_t *__restrict__ offset_mask)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= total) return;
    const float d = denom[i];
    const float g = grad_accum[i] / d;
    grads_norm[i] = g != g ? 0.0f : fabsf(g);
    offset_mask[i] = d > thr;
}

// ------------------------------------------------------------------ gpcc_densify_finish
__global__ __launch_bounds__(TB) void k_finish_flags(const float *__restrict__ opacity_accum, const float *__restrict__ anchor_demon, int64_t n1, float anchor_thr,
                                                     float min_opacity, uint8_t *__restrict__ prune, uint32_t *__restrict__ rank)
{
    const int64_t a = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (a > n1) return;
    uint32_t keep = 0;
    if (a < n1) {
        const float d = anchor_demon[a];
        const bool p = opacity_accum[a] < min_opacity * d && d > anchor_thr;
        prune[a] = p;
        keep = !p;
    }
    rank[a] = keep;   // rank[n1] = 0: the scan leaves the survivors' count there
}

// a lane per (anchor, offset) of the grown model; the lane of offset 0 also moves the anchor's two words
__global__ __launch_bounds__(TB) void k_finish_gather(const float *__restrict__ grad_accum, const float *__restrict__ denom, const uint8_t *__restrict__ offset_mask,
                                                      int64_t n0, const float *__restrict__ opacity_accum, const float *__restrict__ anchor_demon, int64_t n1,
                                                      int k, float anchor_thr, const uint8_t *__restrict__ prune, const uint32_t *__restrict__ rank,
                                                      float *__restrict__ out_grad_accum, float *__restrict__ out_denom, float *__restrict__ out_opacity_accum,
                                                      float *__restrict__ out_anchor_demon)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n1 * k) return;
    const int64_t a = (uint32_t)i / (uint32_t)k;   // n1 k < 2^31
    const int j = (int)(i - a * k);
    if (prune[a]) return;
    const int64_t o = rank[a];
    const bool live = a < n0 && !offset_mask[i];
    out_grad_accum[o * k + j] = live ? grad_accum[i] : 0.0f;
    out_denom[o * k + j] = live ? denom[i] : 0.0f;
    if (j == 0) {
        const float d = anchor_demon[a];
        const bool reset = d > anchor_thr;
        out_opacity_accum[o] = reset ? 0.0f : opacity_accum[a];
        out_anchor_demon[o] = reset ? 0.0f : d;
    }
}

// ------------------------------------------------------------------ gpcc_compact_rows
struct Mats {
    const float *src[MAX_MATS];
    float *dst[MAX_MATS];
    uint32_t width[MAX_MATS];
};

__global__ __launch_bounds__(TB) void k_keep_flags(const uint8_t *__restrict__ keep, int64_t n, uint32_t *__restrict__ rank)
{
    const int64_t a = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (a <= n) rank[a] = a < n ? keep[a] != 0 : 0u;
}

// blockIdx.y = the matrix, a lane per element of it
__global__ __launch_bounds__(TB) void k_compact(Mats mats, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ rank, uint32_t n)
{
    const uint32_t w = mats.width[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= (uint64_t)n * w) return;
    const uint32_t row = (uint32_t)i / w, col = (uint32_t)i - row * w;   // n w < 2^31 (checked by the host)
    if (!keep[row]) return;
    mats.dst[blockIdx.y][(uint64_t)rank[row] * w + col] = mats.src[blockIdx.y][i];
}

// The transpose of k_compact: blockIdx.y = the matrix, a lane per element of the n-row destination.  rank == nullptr: no row is kept.
// A kept row whose rank is not below m (a mask that does not count m rows) reads nothing and gets zeros.
__global__ __launch_bounds__(TB) void k_expand(Mats mats, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ rank, uint32_t n, uint32_t m)
{
    const uint32_t w = mats.width[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= (uint64_t)n * w) return;
    const uint32_t row = (uint32_t)i / w, col = (uint32_t)i - row * w;   // n w < 2^31 (checked by the host)
    float v = 0.0f;
    if (rank && keep[row]) {
        const uint32_t r = rank[row];
        if (r < m) v = mats.src[blockIdx.y][(uint64_t)r * w + col];
    }
    mats.dst[blockIdx.y][i] = v;
}

// the survivors' count, the call's one synchronisation
int read_count(gpcc_ctx *ctx, hipStream_t st, const uint32_t *word, int64_t *count)
{
    GP_TRY(ctx->hstage.reserve(64));
    uint32_t *h = reinterpret_cast<uint32_t *>(ctx->hstage.p);
    HIP_TRY(hipMemcpyAsync(h, word, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    GP_TRY(device_error_check(ctx));
    *count = h[0];
    return GPCC_OK;
}

constexpr int64_t ROWS_MAX = (int64_t)1 << 28;   // the look-back scan's reach (65536 tiles of 4096) with room for the appended word

}  // namespace

extern "C" int gpcc_densify_stats(gpcc_ctx *ctx, int64_t n, int k, const uint8_t *visible, const float *opacity, int64_t v, const uint8_t *selection,
                                  const uint8_t *update_filter, int64_t s, const float *grad, int64_t grad_stride, float *opacity_accum, float *anchor_demon,
                                  float *offset_gradient_accum, float *offset_denom, uint32_t *err, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gpcc_densify_stats: null context");
    if (n < 0 || n >= ROWS_MAX || v < 0 || v >= ROWS_MAX || k < 1 || k > TB || n * k >= ((int64_t)1 << 31) || v * k >= ((int64_t)1 << 31))
        return fail(GPCC_ERR_ARG, "gpcc_densify_stats: n = %lld, v = %lld, k = %d (n, v < 2^28, 1 <= k <= 256, n k and v k < 2^31)", (long long)n, (long long)v, k);
    if (s < 0 || s > v * k || grad_stride < 2) return fail(GPCC_ERR_ARG, "gpcc_densify_stats: s = %lld for %lld entries, grad stride %lld", (long long)s, (long long)(v * k), (long long)grad_stride);
    if (!visible && v != n) return fail(GPCC_ERR_ARG, "gpcc_densify_stats: no visible mask but opacity has %lld rows for %lld anchors", (long long)v, (long long)n);
    if (!err || !alloc || (n > 0 && (!opacity_accum || !anchor_demon || !offset_gradient_accum || !offset_denom)) || (v > 0 && (!opacity || !selection)) ||
        (s > 0 && (!update_filter || !grad)))
        return fail(GPCC_ERR_ARG, "gpcc_densify_stats: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t m = n > v ? n : v, m1 = m + 1;
    uint32_t *rv, *rs;
    GP_TRY(caller_block(alloc, alloc_user, "gpcc_densify_stats", [&](Carver &c) { rv = c.take<uint32_t>(m1); rs = c.take<uint32_t>(m1); }));
    k_stats_flags<<<(unsigned)cdiv(m1, TB), TB, 0, st>>>(visible, n, selection, v, k, m1, rv, rs);
    LAUNCH_CHECK();
    GP_TRY(exclusive_scan_pair_u32(ctx, st, rv, rv, rs, rs, m1));
    k_stats_update<<<(unsigned)cdiv(n > 0 ? n : 1, TB / k), TB, 0, st>>>(visible, n, k, opacity, v, selection, update_filter, s, grad, grad_stride, rv, rs, m, opacity_accum,
                                                                     anchor_demon, offset_gradient_accum, offset_denom, err);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gpcc_densify_front(gpcc_ctx *ctx, const float *offset_gradient_accum, const float *offset_denom, int64_t total, float offset_thr,
                                  float *grads_norm_out, uint8_t *offset_mask_out, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gpcc_densify_front: null context");
    if (total < 0) return fail(GPCC_ERR_ARG, "gpcc_densify_front: %lld entries", (long long)total);
    if (total == 0) return GPCC_OK;
    if (!offset_gradient_accum || !offset_denom || !grads_norm_out || !offset_mask_out) return fail(GPCC_ERR_ARG, "gpcc_densify_front: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    k_front<<<(unsigned)cdiv(total, TB), TB, 0, (hipStream_t)stream>>>(offset_gradient_accum, offset_denom, total, offset_thr, grads_norm_out, offset_mask_out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gpcc_densify_finish(gpcc_ctx *ctx, const float *offset_gradient_accum, const float *offset_denom, const uint8_t *offset_mask, int64_t n0, int k,
                                   const float *opacity_accum, const float *anchor_demon, int64_t n1, float anchor_thr, float min_opacity, uint8_t *prune_out,
                                   int64_t *count_out, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx || !count_out) return fail(GPCC_ERR_ARG, "gpcc_densify_finish: null context or count");
    *count_out = 0;
    if (n0 < 0 || n1 < n0 || n1 >= ROWS_MAX || k < 1 || k > 1024 || n1 * k >= ((int64_t)1 << 31))
        return fail(GPCC_ERR_ARG, "gpcc_densify_finish: n0 = %lld, n1 = %lld, k = %d (n0 <= n1 < 2^28, 1 <= k <= 1024, n1 k < 2^31)", (long long)n0, (long long)n1, k);
    if (n1 == 0) return GPCC_OK;
    if (!alloc || !opacity_accum || !anchor_demon || !prune_out || (n0 > 0 && (!offset_gradient_accum || !offset_denom || !offset_mask)))
        return fail(GPCC_ERR_ARG, "gpcc_densify_finish: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t *rank;
    GP_TRY(caller_alloc(alloc, alloc_user, sizeof(uint32_t) * (size_t)(n1 + 1), &rank, "gpcc_densify_finish: ranks"));
    k_finish_flags<<<(unsigned)cdiv(n1 + 1, TB), TB, 0, st>>>(opacity_accum, anchor_demon, n1, anchor_thr, min_opacity, prune_out, rank);
    LAUNCH_CHECK();
    GP_TRY(exclusive_scan_u32(ctx, st, rank, rank, n1 + 1, nullptr));
    int64_t n2 = 0;
    GP_TRY(read_count(ctx, st, rank + n1, &n2));
    *count_out = n2;
    if (n2 == 0) return GPCC_OK;
    float *out[4];
    for (int t = 0; t < 4; ++t) GP_TRY(caller_alloc(alloc, alloc_user, sizeof(float) * (size_t)(n2 * (t < 2 ? k : 1)), &out[t], "gpcc_densify_finish: outputs"));
    k_finish_gather<<<(unsigned)cdiv(n1 * k, TB), TB, 0, st>>>(offset_gradient_accum, offset_denom, offset_mask, n0, opacity_accum, anchor_demon, n1, k, anchor_thr,
                                                               prune_out, rank, out[0], out[1], out[2], out[3]);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gpcc_compact_rows(gpcc_ctx *ctx, const uint8_t *keep, int64_t n, int nmats, const float *const *src, const int64_t *widths, int64_t *count_out,
                                 gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx || !count_out) return fail(GPCC_ERR_ARG, "gpcc_compact_rows: null context or count");
    *count_out = 0;
    if (n < 0 || n >= ROWS_MAX || nmats < 0 || nmats > MAX_MATS) return fail(GPCC_ERR_ARG, "gpcc_compact_rows: n = %lld (< 2^28), %d matrices (<= %d)", (long long)n, nmats, MAX_MATS);
    if (nmats > 0 && (!src || !widths)) return fail(GPCC_ERR_ARG, "gpcc_compact_rows: null argument");
    Mats mats = {};
    int64_t wmax = 0;
    for (int t = 0; t < nmats; ++t) {
        if (widths[t] < 0 || (n > 0 && widths[t] > (((int64_t)1 << 31) - 1) / n) || (n > 0 && widths[t] > 0 && !src[t]))
            return fail(GPCC_ERR_ARG, "gpcc_compact_rows: matrix %d of width %lld (n width < 2^31)", t, (long long)widths[t]);
        mats.src[t] = src[t];
        mats.width[t] = (uint32_t)widths[t];
        wmax = widths[t] > wmax ? widths[t] : wmax;
    }
    if (n == 0) return GPCC_OK;
    if (!keep || !alloc) return fail(GPCC_ERR_ARG, "gpcc_compact_rows: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t *rank;
    GP_TRY(caller_alloc(alloc, alloc_user, sizeof(uint32_t) * (size_t)(n + 1), &rank, "gpcc_compact_rows: ranks"));
    k_keep_flags<<<(unsigned)cdiv(n + 1, TB), TB, 0, st>>>(keep, n, rank);
    LAUNCH_CHECK();
    GP_TRY(exclusive_scan_u32(ctx, st, rank, rank, n + 1, nullptr));
    int64_t n2 = 0;
    GP_TRY(read_count(ctx, st, rank + n, &n2));
    *count_out = n2;
    if (n2 == 0 || nmats == 0) return GPCC_OK;
    for (int t = 0; t < nmats; ++t) GP_TRY(caller_alloc(alloc, alloc_user, sizeof(float) * (size_t)(n2 * widths[t]), &mats.dst[t], "gpcc_compact_rows: outputs"));
    if (wmax == 0) return GPCC_OK;
    k_compact<<<dim3((unsigned)cdiv(n * wmax, TB), (unsigned)nmats), TB, 0, st>>>(mats, keep, rank, (uint32_t)n);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gpcc_expand_rows(gpcc_ctx *ctx, const uint8_t *keep, int64_t n, int64_t m, int nmats, const float *const *src, const int64_t *widths, float *const *dst,
                                gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gpcc_expand_rows: null context");
    if (n < 0 || n >= ROWS_MAX || m < 0 || m > n || nmats < 0 || nmats > MAX_MATS)
        return fail(GPCC_ERR_ARG, "gpcc_expand_rows: n = %lld (< 2^28), m = %lld (0..n), %d matrices (<= %d)", (long long)n, (long long)m, nmats, MAX_MATS);
    if (nmats > 0 && (!src || !widths || !dst)) return fail(GPCC_ERR_ARG, "gpcc_expand_rows: null argument");
    Mats mats = {};
    int64_t wmax = 0;
    for (int t = 0; t < nmats; ++t) {
        if (widths[t] < 0 || (n > 0 && widths[t] > (((int64_t)1 << 31) - 1) / n) || (n > 0 && widths[t] > 0 && (!dst[t] || (m > 0 && !src[t]))))
            return fail(GPCC_ERR_ARG, "gpcc_expand_rows: matrix %d of width %lld (n width < 2^31, non-null)", t, (long long)widths[t]);
        mats.src[t] = src[t];
        mats.dst[t] = dst[t];
        mats.width[t] = (uint32_t)widths[t];
        wmax = widths[t] > wmax ? widths[t] : wmax;
    }
    if (n == 0 || nmats == 0 || wmax == 0) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t *rank = nullptr;
    if (m > 0) {   // m == 0: every row is zero, no scan
        if (!keep || !alloc) return fail(GPCC_ERR_ARG, "gpcc_expand_rows: null argument");
        GP_TRY(caller_alloc(alloc, alloc_user, sizeof(uint32_t) * (size_t)(n + 1), &rank, "gpcc_expand_rows: ranks"));
        k_keep_flags<<<(unsigned)cdiv(n + 1, TB), TB, 0, st>>>(keep, n, rank);
        LAUNCH_CHECK();
        GP_TRY(exclusive_scan_u32(ctx, st, rank, rank, n + 1, nullptr));
    }
    k_expand<<<dim3((unsigned)cdiv(n * wmax, TB), (unsigned)nmats), TB, 0, st>>>(mats, keep, rank, (uint32_t)n, (uint32_t)m);
    LAUNCH_CHECK();
    return GPCC_OK;
}
