// gridencoder.hip -- HAC's hash-grid encoder, forward and backward:
//   gsge_forward         _gridencoder.grid_encode_forward   gridencoder.zip!gridencoder/src/gridencoder.cu:46-361
//   gsge_forward_train   the same plus dy_dx                ...:363-657
//   gsge_backward        _gridencoder.grid_encode_backward  ...:663-881, store-and-sum instead of atomicAdd
// (the tri-plane sampler gsge_plane_* is triplane.hip)
#include "common.hpp"
#include "primitives.hpp"
#include "sorted_sum.hpp"

using namespace gpcc;

namespace {

constexpr int TB = 256;

// ------------------------------------------------------------------ hash-grid forward
__device__ __forceinline__ uint32_t grid_index(int D, uint32_t F, uint32_t hashmap_size, uint32_t res, const uint32_t *pg)
{
    uint32_t stride = 1, index = 0;
    for (int d = 0; d < D && stride <= hashmap_size; ++d) { index += pg[d] * stride; stride *= res; }
    if (stride > hashmap_size) {  // gridencoder.cu:46-60: xor of coordinate * prime
        const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
        uint32_t h = 0;
        for (int d = 0; d < D; ++d) h ^= pg[d] * primes[d];
        index = h;
    }
    return (index % hashmap_size) * F;
}

// The corners of point x at one level (gridencoder.cu:180-330), shared by the forward and the backward's key pass: per corner its
// weight, whether it is used (no coordinate at 0 or res - 1, and an occupied voxel in its binary_vxl footprint) and, when used, its
// element offset (index % hashmap_size) * F in the level's table.  Returns wn_re = 1 / (sum of the used weights, 1e-9 when none).
template <int D>
__device__ __forceinline__ float grid_corners(const float *x, uint32_t res, uint32_t hashmap_size, uint32_t F, uint32_t Rb, const uint8_t *__restrict__ binary_vxl,
                                              float *w_list, uint32_t *idx_list, bool *use)
{
    float pos[D];
    uint32_t pg[D];
    for (int d = 0; d < D; ++d) {
        const float t = x[d] * (float)(res - 2);
        pos[d] = t + 0.5f;                           // (float)((double)t + 0.5): identical rounding
        pg[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pg[d];
    }
    float wn = 0.0f;
    for (int c = 0; c < (1 << D); ++c) {
        float w = 1.0f;
        uint32_t pl[D];
        for (int d = 0; d < D; ++d) {
            if ((c & (1 << d)) == 0) { w *= 1.0f - pos[d]; pl[d] = pg[d]; }
            else { w *= pos[d]; pl[d] = min(pg[d] + 1u, res - 1u); }
        }
        bool zero = false;
        for (int d = 0; d < D; ++d) zero |= (pl[d] == 0u || pl[d] == res - 1u);
        bool m = true;
        if (binary_vxl) {  // gridencoder.cu:262-317: any occupied voxel in the corner's footprint
            m = false;
            const float scale_re = (float)(1.0 / ((double)(float)res - 2.0));
            int g0[D], g1[D];
            for (int d = 0; d < D; ++d) {
                const float pn = (float)(((double)(float)pl[d] - 0.5) * (double)scale_re);
                float a = (pn - scale_re) * (float)Rb;
                a = a < 0.0f ? 0.0f : a; a = a > (float)(Rb - 1) ? (float)(Rb - 1) : a;
                g0[d] = (int)a;
                float bb = (pn + scale_re) * (float)Rb;
                bb = bb < 0.0f ? 0.0f : bb; bb = bb > (float)(Rb - 1) ? (float)(Rb - 1) : bb;
                g1[d] = (int)bb;
            }
            if (D == 2) {
                for (int ia = g0[0]; ia <= g1[0] && !m; ++ia)
                    for (int ib = g0[1]; ib <= g1[1] && !m; ++ib) m = binary_vxl[(size_t)ia * Rb + ib] != 0;
            } else if (D == 3) {
                for (int ia = g0[0]; ia <= g1[0] && !m; ++ia)
                    for (int ib = g0[1]; ib <= g1[1] && !m; ++ib)
                        for (int ic = g0[D - 1]; ic <= g1[D - 1] && !m; ++ic) m = binary_vxl[((size_t)ia * Rb + ib) * Rb + ic] != 0;
            } else {
                for (int ia = g0[0]; ia <= g1[0] && !m; ++ia) m = binary_vxl[ia] != 0;
            }
        }
        w_list[c] = w;
        use[c] = !zero && m;
        idx_list[c] = 0;
        if (use[c]) { idx_list[c] = grid_index(D, F, hashmap_size, res, pl); wn += w; }
    }
    if (wn == 0.0f) wn = (float)((double)wn + 1e-9);
    return (float)(1.0 / (double)wn);
}

template <int D, int F>
__global__ __launch_bounds__(TB) void k_grid_forward(const float *__restrict__ inputs, const float *__restrict__ grid, const int *__restrict__ offsets,
                                                     const int *__restrict__ resolutions, float *__restrict__ outputs, uint32_t N, uint32_t Rb,
                                                     const uint8_t *__restrict__ binary_vxl, const int *__restrict__ min_level_id)
{
    const uint32_t b = blockIdx.x * TB + threadIdx.x;
    if (b >= N) return;
    const uint32_t level = min_level_id ? (uint32_t)min_level_id[b] + blockIdx.y : blockIdx.y;
    grid += (size_t)(uint32_t)offsets[level] * F;
    const float *x = inputs + (size_t)b * D;
    float *out = outputs + ((size_t)blockIdx.y * N + b) * F;
    bool oob = false;
    for (int d = 0; d < D; ++d) oob |= (x[d] < 0.0f || x[d] > 1.0f);
    if (oob) { for (int ch = 0; ch < F; ++ch) out[ch] = 0.0f; return; }
    const uint32_t hashmap_size = (uint32_t)(offsets[level + 1] - offsets[level]);
    const uint32_t res = (uint32_t)resolutions[level];
    float w_list[1 << D];
    uint32_t idx_list[1 << D];
    bool use[1 << D];
    const float wn_re = grid_corners<D>(x, res, hashmap_size, F, Rb, binary_vxl, w_list, idx_list, use);
    float r[F];
    for (int ch = 0; ch < F; ++ch) r[ch] = 0.0f;
    for (int c = 0; c < (1 << D); ++c)
        if (use[c]) {
            const float ww = w_list[c] * wn_re;
            for (int ch = 0; ch < F; ++ch) r[ch] = __builtin_fmaf(ww, grid[idx_list[c] + ch], r[ch]);  // nvcc contracts mul+add (fmad) here
        }
    for (int ch = 0; ch < F; ++ch) out[ch] = r[ch];
}

template <int D>
int grid_launch_f(hipStream_t st, int F, dim3 g, const float *in, const float *emb, const int *off, const int *res, float *out, uint32_t N, uint32_t Rb,
                  const uint8_t *bv, const int *ml)
{
    switch (F) {
    case 1: k_grid_forward<D, 1><<<g, TB, 0, st>>>(in, emb, off, res, out, N, Rb, bv, ml); break;
    case 2: k_grid_forward<D, 2><<<g, TB, 0, st>>>(in, emb, off, res, out, N, Rb, bv, ml); break;
    case 4: k_grid_forward<D, 4><<<g, TB, 0, st>>>(in, emb, off, res, out, N, Rb, bv, ml); break;
    case 8: k_grid_forward<D, 8><<<g, TB, 0, st>>>(in, emb, off, res, out, N, Rb, bv, ml); break;
    default: return fail(GPCC_ERR_ARG, "GridEncoding: n_features must be 1, 2, 4 or 8");
    }
    LAUNCH_CHECK();
    return GPCC_OK;
}

// ------------------------------------------------------------------ hash-grid training: dy_dx and backward
// dy_dx[gd][ch] of one point at one level as gridencoder.cu:363-657 writes it: per axis gd, over the 2^(D-1) edges along gd in ascending
// edge index, w = (res - 2) * prod_{d != gd} (1 - pos[d] or pos[d]) times (g_right - g_left), the two corners at pg[gd] and
// min(pg[gd] + 1, res - 1); a corner with a coordinate at 0 or res - 1 reads as 0.  No wn normalisation and no binary_vxl mask (the
// reference's formula: the exact derivative only inside the grid with all corners used).
template <int D, int F>
__device__ __forceinline__ void grid_dydx(const float *x, const float *__restrict__ grid, uint32_t res, uint32_t hashmap_size, float (&g)[D][F])
{
    float pos[D];
    uint32_t pg[D];
    for (int d = 0; d < D; ++d) {
        const float t = x[d] * (float)(res - 2);
        pos[d] = t + 0.5f;
        pg[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pg[d];
    }
    for (int gd = 0; gd < D; ++gd) {
        for (int ch = 0; ch < F; ++ch) g[gd][ch] = 0.0f;
        for (int e = 0; e < (1 << (D - 1)); ++e) {
            float w = (float)(res - 2);
            uint32_t pl[D];
            for (int nd = 0; nd < D - 1; ++nd) {
                const int d = nd >= gd ? nd + 1 : nd;
                if ((e & (1 << nd)) == 0) { w *= 1.0f - pos[d]; pl[d] = pg[d]; }
                else { w *= pos[d]; pl[d] = min(pg[d] + 1u, res - 1u); }
            }
            bool zl = false, zr = false;
            pl[gd] = pg[gd];
            for (int d = 0; d < D; ++d) zl |= (pl[d] == 0u || pl[d] == res - 1u);
            const uint32_t il = zl ? 0u : grid_index(D, F, hashmap_size, res, pl);
            pl[gd] = min(pg[gd] + 1u, res - 1u);
            for (int d = 0; d < D; ++d) zr |= (pl[d] == 0u || pl[d] == res - 1u);
            const uint32_t ir = zr ? 0u : grid_index(D, F, hashmap_size, res, pl);
            for (int ch = 0; ch < F; ++ch) {
                const float gl = zl ? 0.0f : grid[il + ch], gr = zr ? 0.0f : grid[ir + ch];
                g[gd][ch] = __builtin_fmaf(w, gr - gl, g[gd][ch]);
            }
        }
    }
}

__device__ __forceinline__ bool grid_oob(const float *x, int D)
{
    bool oob = false;
    for (int d = 0; d < D; ++d) oob |= (x[d] < 0.0f || x[d] > 1.0f);
    return oob;
}

// dy_dx (N, L, D, F) of the training forward: one thread per (point, level), beside the unchanged k_grid_forward
template <int D, int F>
__global__ __launch_bounds__(TB) void k_grid_dydx(const float *__restrict__ inputs, const float *__restrict__ grid, const int *__restrict__ offsets,
                                                  const int *__restrict__ resolutions, float *__restrict__ dy_dx, uint32_t N, const int *__restrict__ min_level_id)
{
    const uint32_t b = blockIdx.x * TB + threadIdx.x;
    if (b >= N) return;
    const uint32_t level = min_level_id ? (uint32_t)min_level_id[b] + blockIdx.y : blockIdx.y;
    const float *x = inputs + (size_t)b * D;
    float *out = dy_dx + ((size_t)b * gridDim.y + blockIdx.y) * D * F;
    float g[D][F];
    if (grid_oob(x, D)) {
        for (int d = 0; d < D; ++d)
            for (int ch = 0; ch < F; ++ch) g[d][ch] = 0.0f;
    } else {
        grid_dydx<D, F>(x, grid + (size_t)(uint32_t)offsets[level] * F, (uint32_t)resolutions[level], (uint32_t)(offsets[level + 1] - offsets[level]), g);
    }
    for (int d = 0; d < D; ++d)
        for (int ch = 0; ch < F; ++ch) out[d * F + ch] = g[d][ch];
}

// Backward, embedding gradient: store and sum, no float atomics.
//   key pass   one thread per (point b, level l): corner c's contribution lives at slot s = (b L + l) 2^D + c; the key is its table row
//              offsets[level] + idx / F (the sentinel n_rows when the corner is unused or the point out of range), the value the slot,
//              and wts[s] = w_c wn_re.
//   sort       stable LSD radix sort on the key: each row's contributions become one run in ascending slot order.
//   sum, combine   sorted_sum.hpp (shared with the tri-plane's backward): one thread per chunk of GB_CHUNK sorted entries sums each run it
//              holds in order (fmaf(w, grad[l, b, ch], acc)); runs that cross chunks are finished by their first chunk's thread.
// Every row is written by exactly one thread and summed in an order fixed by the sorted keys alone: bitwise reproducible.
constexpr int GB_CHUNK = 32;

template <int D>
__global__ __launch_bounds__(TB) void k_grid_bwd_keys(const float *__restrict__ inputs, const int *__restrict__ offsets, const int *__restrict__ resolutions,
                                                      uint32_t N, uint32_t F, uint32_t Rb, const uint8_t *__restrict__ binary_vxl,
                                                      const int *__restrict__ min_level_id, uint32_t n_rows, uint64_t *__restrict__ keys,
                                                      uint32_t *__restrict__ slots, float *__restrict__ wts)
{
    const uint32_t b = blockIdx.x * TB + threadIdx.x;
    if (b >= N) return;
    const uint32_t level = min_level_id ? (uint32_t)min_level_id[b] + blockIdx.y : blockIdx.y;
    const uint32_t s0 = (b * gridDim.y + blockIdx.y) << D;
    const float *x = inputs + (size_t)b * D;
    float w_list[1 << D];
    uint32_t idx_list[1 << D];
    bool use[1 << D];
    float wn_re = 0.0f;
    const bool oob = grid_oob(x, D);
    const uint32_t off = (uint32_t)offsets[level];
    if (!oob) wn_re = grid_corners<D>(x, (uint32_t)resolutions[level], (uint32_t)(offsets[level + 1] - offsets[level]), F, Rb, binary_vxl, w_list, idx_list, use);
    for (int c = 0; c < (1 << D); ++c) {
        uint32_t row = n_rows;
        if (!oob && use[c]) {
            row = off + idx_list[c] / F;
            if (row >= n_rows) row = n_rows;     // offsets beyond the caller's table: dropped, never written out of bounds
            else wts[s0 + c] = w_list[c] * wn_re;
        }
        keys[s0 + c] = row;
        slots[s0 + c] = s0 + c;
    }
}

template <int F>
__device__ __forceinline__ void gb_add(float (&acc)[F], const float *__restrict__ grad, const uint32_t *__restrict__ slots, const float *__restrict__ wts,
                                       int64_t i, int D, uint32_t N, uint32_t L)
{
    const uint32_t s = slots[i], q = s >> D, b = q / L, l = q - b * L;
    const float w = wts[s];
    const float *g = grad + ((size_t)l * N + b) * F;
    for (int ch = 0; ch < F; ++ch) acc[ch] = __builtin_fmaf(w, g[ch], acc[ch]);
}

template <int F> struct GridRowSum {
    const float *__restrict__ grad;
    const uint32_t *__restrict__ slots;
    const float *__restrict__ wts;
    int D;
    uint32_t N, L;
    float *__restrict__ grad_emb, *__restrict__ head, *__restrict__ tail;
    float acc[F];
    __device__ __forceinline__ void zero() { for (int ch = 0; ch < F; ++ch) acc[ch] = 0.0f; }
    __device__ __forceinline__ void add(int64_t i) { gb_add<F>(acc, grad, slots, wts, i, D, N, L); }
    __device__ __forceinline__ void to_head(int64_t t) { for (int ch = 0; ch < F; ++ch) head[t * F + ch] = acc[ch]; }
    __device__ __forceinline__ void to_tail(int64_t t) { for (int ch = 0; ch < F; ++ch) tail[t * F + ch] = acc[ch]; }
    __device__ __forceinline__ void to_row(uint32_t row) { for (int ch = 0; ch < F; ++ch) grad_emb[(size_t)row * F + ch] += acc[ch]; }
};

template <int F>
__global__ __launch_bounds__(TB) void k_grid_bwd_sum(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slots, const float *__restrict__ wts,
                                                     const float *__restrict__ grad, int D, uint32_t N, uint32_t L, int64_t E, uint32_t n_rows,
                                                     float *__restrict__ grad_emb, float *__restrict__ head, float *__restrict__ tail, uint8_t *__restrict__ own)
{
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t * GB_CHUNK >= E) return;
    GridRowSum<F> a{grad, slots, wts, D, N, L, grad_emb, head, tail, {}};
    sorted_chunk_sum<GB_CHUNK>(keys, t, E, n_rows, a, own);
}

// the owners' walk: partials are read GB_WALK chunks at a time
constexpr int GB_WALK = 8;

template <int F>
__global__ __launch_bounds__(TB) void k_grid_bwd_combine(const uint64_t *__restrict__ keys, int64_t E, int64_t nchunks, const float *__restrict__ head,
                                                         const float *__restrict__ tail, const uint8_t *__restrict__ own, float *__restrict__ grad_emb)
{
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    sorted_combine<GB_CHUNK, F, GB_WALK>(keys, E, nchunks, t, head, tail, F, own, [&](uint32_t row, const float (&s)[F]) {
        for (int ch = 0; ch < F; ++ch) grad_emb[(size_t)row * F + ch] += s[ch];
    });
}

// Backward, input gradient: one thread per point, dy_dx recomputed; levels outer, channels inner (gridencoder.cu:857-881)
template <int D, int F>
__global__ __launch_bounds__(TB) void k_grid_bwd_inputs(const float *__restrict__ inputs, const float *__restrict__ grid, const int *__restrict__ offsets,
                                                        const int *__restrict__ resolutions, const float *__restrict__ grad, uint32_t N, uint32_t L,
                                                        const int *__restrict__ min_level_id, float *__restrict__ grad_inputs)
{
    const uint32_t b = blockIdx.x * TB + threadIdx.x;
    if (b >= N) return;
    const float *x = inputs + (size_t)b * D;
    float r[D];
    for (int d = 0; d < D; ++d) r[d] = 0.0f;
    if (!grid_oob(x, D)) {
        const uint32_t ml = min_level_id ? (uint32_t)min_level_id[b] : 0u;
        for (uint32_t l = 0; l < L; ++l) {
            const uint32_t level = ml + l;
            float g[D][F];
            grid_dydx<D, F>(x, grid + (size_t)(uint32_t)offsets[level] * F, (uint32_t)resolutions[level], (uint32_t)(offsets[level + 1] - offsets[level]), g);
            const float *gp = grad + ((size_t)l * N + b) * F;
            for (int ch = 0; ch < F; ++ch)
                for (int d = 0; d < D; ++d) r[d] = __builtin_fmaf(gp[ch], g[d][ch], r[d]);
        }
    }
    for (int d = 0; d < D; ++d) grad_inputs[(size_t)b * D + d] = r[d];
}

template <int D>
int grid_dydx_launch(hipStream_t st, int F, dim3 g, const float *in, const float *emb, const int *off, const int *res, float *dy_dx, uint32_t N, const int *ml)
{
    switch (F) {
    case 1: k_grid_dydx<D, 1><<<g, TB, 0, st>>>(in, emb, off, res, dy_dx, N, ml); break;
    case 2: k_grid_dydx<D, 2><<<g, TB, 0, st>>>(in, emb, off, res, dy_dx, N, ml); break;
    case 4: k_grid_dydx<D, 4><<<g, TB, 0, st>>>(in, emb, off, res, dy_dx, N, ml); break;
    case 8: k_grid_dydx<D, 8><<<g, TB, 0, st>>>(in, emb, off, res, dy_dx, N, ml); break;
    default: return fail(GPCC_ERR_ARG, "GridEncoding: n_features must be 1, 2, 4 or 8");
    }
    LAUNCH_CHECK();
    return GPCC_OK;
}

template <int D, int F>
void grid_bwd_inputs_launch(hipStream_t st, const float *in, const float *emb, const int *off, const int *res, const float *grad, uint32_t N, uint32_t L,
                            const int *ml, float *gi)
{
    k_grid_bwd_inputs<D, F><<<(unsigned)cdiv(N, TB), TB, 0, st>>>(in, emb, off, res, grad, N, L, ml, gi);
}

template <int F>
void grid_bwd_sum_launch(hipStream_t st, const uint64_t *keys, const uint32_t *slots, const float *wts, const float *grad, int D, uint32_t N, uint32_t L,
                         int64_t E, uint32_t n_rows, float *grad_emb, float *head, float *tail, uint8_t *own, int64_t nchunks)
{
    k_grid_bwd_sum<F><<<(unsigned)cdiv(nchunks, TB), TB, 0, st>>>(keys, slots, wts, grad, D, N, L, E, n_rows, grad_emb, head, tail, own);
    k_grid_bwd_combine<F><<<(unsigned)cdiv(nchunks, TB), TB, 0, st>>>(keys, E, nchunks, head, tail, own, grad_emb);
}

}  // namespace

extern "C" int gsge_forward(gpcc_ctx *ctx, const float *inputs, const float *embeddings, const int32_t *offsets, const int32_t *resolutions,
                            float *outputs, int64_t N, int num_dim, int n_features, int n_levels, int Rb, const uint8_t *binary_vxl,
                            const int32_t *min_level_id, void *stream)
{
    if (!ctx || !inputs || !embeddings || !offsets || !resolutions || !outputs) return fail(GPCC_ERR_ARG, "null argument");
    if (N <= 0 || n_levels <= 0) return GPCC_OK;
    if (N >= ((int64_t)1 << 31)) return fail(GPCC_ERR_ARG, "too many points");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    dim3 g((unsigned)cdiv(N, TB), (unsigned)n_levels);
    switch (num_dim) {
    case 1: return grid_launch_f<1>(st, n_features, g, inputs, embeddings, offsets, resolutions, outputs, (uint32_t)N, (uint32_t)Rb, binary_vxl, min_level_id);
    case 2: return grid_launch_f<2>(st, n_features, g, inputs, embeddings, offsets, resolutions, outputs, (uint32_t)N, (uint32_t)Rb, binary_vxl, min_level_id);
    case 3: return grid_launch_f<3>(st, n_features, g, inputs, embeddings, offsets, resolutions, outputs, (uint32_t)N, (uint32_t)Rb, binary_vxl, min_level_id);
    default: return fail(GPCC_ERR_ARG, "GridEncoding: num_dim must be 1, 2 or 3");
    }
}

// gsge_forward plus dy_dx (N, L, D, F) for the input gradient of _gridencoder's caller (NULL: outputs only).  outputs come from the same
// k_grid_forward launch as gsge_forward's.
extern "C" int gsge_forward_train(gpcc_ctx *ctx, const float *inputs, const float *embeddings, const int32_t *offsets, const int32_t *resolutions,
                                  float *outputs, int64_t N, int num_dim, int n_features, int n_levels, int Rb, const uint8_t *binary_vxl,
                                  const int32_t *min_level_id, float *dy_dx, void *stream)
{
    GP_TRY(gsge_forward(ctx, inputs, embeddings, offsets, resolutions, outputs, N, num_dim, n_features, n_levels, Rb, binary_vxl, min_level_id, stream));
    if (!dy_dx || N <= 0 || n_levels <= 0) return GPCC_OK;
    hipStream_t st = (hipStream_t)stream;
    dim3 g((unsigned)cdiv(N, TB), (unsigned)n_levels);
    switch (num_dim) {
    case 1: return grid_dydx_launch<1>(st, n_features, g, inputs, embeddings, offsets, resolutions, dy_dx, (uint32_t)N, min_level_id);
    case 2: return grid_dydx_launch<2>(st, n_features, g, inputs, embeddings, offsets, resolutions, dy_dx, (uint32_t)N, min_level_id);
    default: return grid_dydx_launch<3>(st, n_features, g, inputs, embeddings, offsets, resolutions, dy_dx, (uint32_t)N, min_level_id);
    }
}

// _gridencoder.grid_encode_backward without float atomics (see k_grid_bwd_keys): adds into grad_embeddings (n_rows, F), overwrites grad_inputs
// (N, D) when given.  Workspace (about 28 bytes per (point, level, corner)) through `alloc`; no synchronisation.
extern "C" int gsge_backward(gpcc_ctx *ctx, const float *grad, const float *inputs, const float *embeddings, const int32_t *offsets, const int32_t *resolutions,
                             int64_t n_rows, float *grad_embeddings, float *grad_inputs, int64_t N, int num_dim, int n_features, int n_levels, int Rb,
                             const uint8_t *binary_vxl, const int32_t *min_level_id, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx || !grad || !inputs || !embeddings || !offsets || !resolutions || !grad_embeddings || !alloc) return fail(GPCC_ERR_ARG, "null argument");
    if (num_dim < 1 || num_dim > 3) return fail(GPCC_ERR_ARG, "GridEncoding: num_dim must be 1, 2 or 3");
    if (n_features != 1 && n_features != 2 && n_features != 4 && n_features != 8) return fail(GPCC_ERR_ARG, "GridEncoding: n_features must be 1, 2, 4 or 8");
    if (N <= 0 || n_levels <= 0) {
        if (grad_inputs && N > 0) HIP_TRY(hipMemsetAsync(grad_inputs, 0, (size_t)N * num_dim * sizeof(float), (hipStream_t)stream));
        return GPCC_OK;
    }
    if (n_rows <= 0 || n_rows >= ((int64_t)1 << 31) - 1) return fail(GPCC_ERR_ARG, "bad embedding row count");
    const int64_t E = (N * n_levels) << num_dim;
    if (E >= ((int64_t)1 << 32)) return fail(GPCC_ERR_ARG, "too many (point, level, corner) slots for 32-bit slot ids");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int F = n_features;
    const int64_t nchunks = cdiv(E, GB_CHUNK);
    uint64_t *ka, *kb;
    uint32_t *va, *vb, *hist;
    float *wts, *head, *tail;
    uint8_t *own;
    GP_TRY(caller_block(alloc, alloc_user, "gsge_backward", [&](Carver &c) {
        ka = c.take<uint64_t>(E); kb = c.take<uint64_t>(E); va = c.take<uint32_t>(E); vb = c.take<uint32_t>(E); wts = c.take<float>(E);
        hist = c.take<uint32_t>(radix_sort_hist_words(E)); head = c.take<float>(nchunks * F); tail = c.take<float>(nchunks * F);
        own = c.take<uint8_t>(nchunks);
    }));
    const uint32_t n = (uint32_t)N, L = (uint32_t)n_levels, nr = (uint32_t)n_rows;
    dim3 g((unsigned)cdiv(N, TB), L);
    switch (num_dim) {
    case 1: k_grid_bwd_keys<1><<<g, TB, 0, st>>>(inputs, offsets, resolutions, n, (uint32_t)F, (uint32_t)Rb, binary_vxl, min_level_id, nr, ka, va, wts); break;
    case 2: k_grid_bwd_keys<2><<<g, TB, 0, st>>>(inputs, offsets, resolutions, n, (uint32_t)F, (uint32_t)Rb, binary_vxl, min_level_id, nr, ka, va, wts); break;
    default: k_grid_bwd_keys<3><<<g, TB, 0, st>>>(inputs, offsets, resolutions, n, (uint32_t)F, (uint32_t)Rb, binary_vxl, min_level_id, nr, ka, va, wts); break;
    }
    LAUNCH_CHECK();
    int bits = 1;
    while (((int64_t)1 << bits) <= n_rows) ++bits;    // the sentinel n_rows sorts last
    uint64_t *k0 = ka, *k1 = kb;
    uint32_t *v0 = va, *v1 = vb;
    GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, E, bits, hist));
    switch (F) {
    case 1: grid_bwd_sum_launch<1>(st, k0, v0, wts, grad, num_dim, n, L, E, nr, grad_embeddings, head, tail, own, nchunks); break;
    case 2: grid_bwd_sum_launch<2>(st, k0, v0, wts, grad, num_dim, n, L, E, nr, grad_embeddings, head, tail, own, nchunks); break;
    case 4: grid_bwd_sum_launch<4>(st, k0, v0, wts, grad, num_dim, n, L, E, nr, grad_embeddings, head, tail, own, nchunks); break;
    default: grid_bwd_sum_launch<8>(st, k0, v0, wts, grad, num_dim, n, L, E, nr, grad_embeddings, head, tail, own, nchunks); break;
    }
    LAUNCH_CHECK();
    if (grad_inputs) {
#define GB_IN(D, F) grid_bwd_inputs_launch<D, F>(st, inputs, embeddings, offsets, resolutions, grad, n, L, min_level_id, grad_inputs)
#define GB_IN_F(D) switch (F) { case 1: GB_IN(D, 1); break; case 2: GB_IN(D, 2); break; case 4: GB_IN(D, 4); break; default: GB_IN(D, 8); break; }
        switch (num_dim) {
        case 1: GB_IN_F(1); break;
        case 2: GB_IN_F(2); break;
        default: GB_IN_F(3); break;
        }
#undef GB_IN_F
#undef GB_IN
        LAUNCH_CHECK();
    }
    return GPCC_OK;
}
