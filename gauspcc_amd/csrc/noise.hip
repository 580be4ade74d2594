// noise.hip -- the adaptive-step quantisation noise of the HAC family's training branch (HAC-plus/gaussian_renderer/__init__.py:47-51,
// 64-69, 91-99): x + U(-0.5, 0.5) * Q0 * (1 + tanh(adj)) on up to three row-aligned attributes (feat, scaling, offsets) in one launch.
//   gsnn_noise_forward    y_j = x_j + u_j * Q_j, Q_j[r] = Q0_j * (1 + tanh(adj[r, col_j])), and the (n, nattr) table of the Q_j[r]
//   gsnn_noise_forward_b / _backward_b   the same with the step rule's base as an argument: Q0 * (base + tanh(adj)), CAT-3DGS's 1.1
//   gsnn_noise_backward   d_adj[r, j] = (sum_c g_j[r, c] u_j[r, c] + gQ[r, j]) * Q0_j * (1 - tanh^2); dx_j is g_j itself, nothing is copied
//   gsnn_quantise        the evaluation side, STE_multistep on the same attributes in one launch: y_j = rint(clamp(x_j, m_j -+ 15000 Q_j) / Q_j) Q_j with
//                        the means m_j device scalars; gsnn_mean forms them (x_j.mean()) by a fixed-order double sum when the caller has none
// The contract is in include/gauspcc.h.  Per element, in float32 and in torch's expression order (no contraction): t = tanhf(adj),
// Q = Q0 * (1 + t), y = x + u * Q.  The noise u is the caller's: which random numbers a seeded run consumes does not change.
//
// Both kernels move bytes and do little else.  Forward: a lane per vector of V floats of the flat (n, w_j) matrix, V chosen per attribute
// from the width and the three base addresses (w = 50, 30 or 6: rows start at 8-byte boundaries at best, V = 2; w = 32: V = 4; w = 3:
// V = 1); a vector never straddles a row because V divides w.  adj is read in place from the context MLP's output (a row stride of e.g. 225
// floats): one 4-byte read per lane, the same address for the lanes of a row.  The lane of column 0 writes the row's Q.
// Backward: L lanes per row (16, or 4 for w <= 8), lane l adds g u over the columns l, l + L, ... in ascending order, then the L partial
// sums meet in a butterfly (xor 1, 2, 4, 8): every lane forms the same sum in the same order, so the result is bitwise reproducible.  No atomics.
#include "common.hpp"

#include <math.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int MAX_ATTR = 3;

struct Attr {
    const float *x, *u;       // backward: g, u
    float *y;
    uint32_t width;
    int col;                  // the column of adj
    int vec;                  // forward: floats per lane (1, 2, 4); backward: lanes per row (4, 16)
    float q0;
};

struct Args {
    Attr a[MAX_ATTR];
    const float *adj;         // NULL: the constant step Q0
    int64_t adj_stride;
    int nattr;
    uint32_t n;
    float base;               // Q = Q0 * (base + tanh(adj)): 1 for the HAC family, 1.1 for CAT-3DGS
};

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<2> { typedef float2 type; };
template <> struct Vec<4> { typedef float4 type; };

template <int V> __device__ __forceinline__ void noise_vec(const Attr &A, uint64_t e, float q)
{
    typedef typename Vec<V>::type T;
    const T xv = *reinterpret_cast<const T *>(A.x + e), uv = *reinterpret_cast<const T *>(A.u + e);
    T yv;
    const float *xs = reinterpret_cast<const float *>(&xv), *us = reinterpret_cast<const float *>(&uv);
    float *ys = reinterpret_cast<float *>(&yv);
#pragma unroll
    for (int i = 0; i < V; ++i) ys[i] = xs[i] + us[i] * q;
    *reinterpret_cast<T *>(A.y + e) = yv;
}

// blockIdx.y = the attribute, a lane per vector of it
__global__ __launch_bounds__(TB) void k_noise_fwd(Args P, float *__restrict__ q_out)
{
    const int j = blockIdx.y;
    const Attr &A = P.a[j];
    const uint32_t w = A.width;
    const uint64_t e = ((uint64_t)blockIdx.x * TB + threadIdx.x) * (uint32_t)A.vec;
    if (e >= (uint64_t)P.n * w) return;
    const uint32_t row = (uint32_t)e / w, col = (uint32_t)e - row * w;      // n w < 2^31 (checked by the host)
    float q = A.q0;
    if (P.adj) q = A.q0 * (P.base + tanhf(P.adj[(int64_t)row * P.adj_stride + A.col]));
    if (col == 0) q_out[(uint64_t)row * P.nattr + j] = q;
    if (A.vec == 4) noise_vec<4>(A, e, q);
    else if (A.vec == 2) noise_vec<2>(A, e, q);
    else noise_vec<1>(A, e, q);
}

// blockIdx.y = the attribute, A.vec lanes per row
__global__ __launch_bounds__(TB) void k_noise_bwd(Args P, const float *__restrict__ gq, float *__restrict__ d_adj)
{
    const int j = blockIdx.y;
    const Attr &A = P.a[j];
    const int L = A.vec;
    const uint32_t w = A.width;
    const uint64_t t = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const uint64_t row = t / (uint32_t)L;
    const uint32_t l = (uint32_t)(t - row * (uint32_t)L);
    const bool live = row < P.n;      // a row's L lanes are live together (L divides the wave); dead lanes still take part in the shuffles
    float s = 0.0f;
    if (live) {
        const float *g = A.x + row * w, *u = A.u + row * w;
        for (uint32_t c = l; c < w; c += L) s = s + g[c] * u[c];
    }
    for (int d = 1; d < L; d <<= 1) s = s + __shfl_xor(s, d, L);
    if (!live || l != 0) return;
    const float th = tanhf(P.adj[(int64_t)row * P.adj_stride + A.col]);
    if (gq) s = s + gq[row * P.nattr + j];
    d_adj[row * P.nattr + j] = (s * A.q0) * fmaf(-th, th, 1.0f);      // autograd's order: the step's gradient, then tanh's, 1 - t t rounded once
}

bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks the two entry points share; fills everything of P but the per-attribute pointers' roles
int make_args(const char *who, int64_t n, int nattr, const float *const *a, const float *const *b, const int64_t *widths, const double *q0, const float *adj,
              int64_t adj_stride, const int *adj_cols, double base, Args &P)
{
    if (n < 0 || nattr < 1 || nattr > MAX_ATTR) return fail(GPCC_ERR_ARG, "%s: n = %lld, %d attributes (1..%d)", who, (long long)n, nattr, MAX_ATTR);
    if (!a || !b || !widths || !q0) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    memset(&P, 0, sizeof(P));
    P.nattr = nattr;
    P.n = (uint32_t)n;
    P.adj = adj;
    P.adj_stride = adj_stride;
    P.base = (float)base;
    for (int j = 0; j < nattr; ++j) {
        if (widths[j] < 1 || (n > 0 && widths[j] > (((int64_t)1 << 31) - 1) / n))
            return fail(GPCC_ERR_ARG, "%s: attribute %d of width %lld (>= 1, n width < 2^31)", who, j, (long long)widths[j]);
        if (n > 0 && (!a[j] || !b[j])) return fail(GPCC_ERR_ARG, "%s: null tensor of attribute %d", who, j);
        P.a[j].x = a[j];
        P.a[j].u = b[j];
        P.a[j].width = (uint32_t)widths[j];
        P.a[j].q0 = (float)q0[j];
        if (adj) {
            if (!adj_cols || adj_cols[j] < 0 || adj_cols[j] >= adj_stride)
                return fail(GPCC_ERR_ARG, "%s: adj column of attribute %d outside the row stride %lld", who, j, (long long)adj_stride);
            P.a[j].col = adj_cols[j];
        }
    }
    if (n >= ((int64_t)1 << 31)) return fail(GPCC_ERR_ARG, "%s: n = %lld (< 2^31)", who, (long long)n);
    return GPCC_OK;
}

// ------------------------------------------------------------------ the quantiser (STE_multistep's forward; no backward: every caller detaches)
struct QArgs {
    Args P;
    const float *means;       // nattr device scalars
    int clamp;
};

template <int V> __device__ __forceinline__ void quant_vec(const Attr &A, uint64_t e, float q, float lo, float hi, bool clamp)
{
    typedef typename Vec<V>::type T;
    const T xv = *reinterpret_cast<const T *>(A.x + e);
    T yv;
    const float *xs = reinterpret_cast<const float *>(&xv);
    float *ys = reinterpret_cast<float *>(&yv);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float v = xs[i];
        if (clamp) {            // torch.clamp: a NaN element stays NaN
            v = v < lo ? lo : v;
            v = v > hi ? hi : v;
        }
        ys[i] = rintf(v / q) * q;      // IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt), half to even, no contraction
    }
    *reinterpret_cast<T *>(A.y + e) = yv;
}

// blockIdx.y = the attribute, a lane per vector of it
__global__ __launch_bounds__(TB) void k_quantise(QArgs Q, float *__restrict__ q_out)
{
    const Args &P = Q.P;
    const int j = blockIdx.y;
    const Attr &A = P.a[j];
    const uint32_t w = A.width;
    const uint64_t e = ((uint64_t)blockIdx.x * TB + threadIdx.x) * (uint32_t)A.vec;
    if (e >= (uint64_t)P.n * w) return;
    const uint32_t row = (uint32_t)e / w, col = (uint32_t)e - row * w;      // n w < 2^31 (checked by the host)
    float q = A.q0;
    if (P.adj) q = A.q0 * (P.base + tanhf(P.adj[(int64_t)row * P.adj_stride + A.col]));
    if (col == 0) q_out[(uint64_t)row * P.nattr + j] = q;
    const float m = Q.means[j], r = 15000.0f * q, lo = m - r, hi = m + r;
    if (A.vec == 4) quant_vec<4>(A, e, q, lo, hi, Q.clamp);
    else if (A.vec == 2) quant_vec<2>(A, e, q, lo, hi, Q.clamp);
    else quant_vec<1>(A, e, q, lo, hi, Q.clamp);
}

// ------------------------------------------------------------------ the means: MEAN_PARTS workgroups per tensor, then one
constexpr int MEAN_PARTS = 256;

struct MeanArgs {
    const float *x[MAX_ATTR];
    int64_t count[MAX_ATTR];
};

// the workgroup's TB doubles to one, a fixed tree
__device__ __forceinline__ double block_sum(double s, double *sh)
{
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = TB / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    return sh[0];
}

// thread t of workgroup b adds the elements b TB + t, + MEAN_PARTS TB, ... in ascending order
__global__ __launch_bounds__(TB) void k_mean_partial(MeanArgs M, double *__restrict__ partials)
{
    __shared__ double sh[TB];
    const int j = blockIdx.y;
    const float *x = M.x[j];
    const int64_t n = M.count[j];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)MEAN_PARTS * TB) s += (double)x[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partials[j * MEAN_PARTS + blockIdx.x] = s;
}

__global__ __launch_bounds__(TB) void k_mean_final(MeanArgs M, const double *__restrict__ partials, float *__restrict__ means)
{
    __shared__ double sh[TB];
    static_assert(MEAN_PARTS == TB, "one partial per thread");
    const int j = blockIdx.x;
    const double s = block_sum(partials[j * MEAN_PARTS + threadIdx.x], sh);
    if (threadIdx.x == 0) means[j] = (float)(s / (double)M.count[j]);
}

}  // namespace

extern "C" int gsnn_mean(gpcc_ctx *ctx, int nattr, const float *const *x, const int64_t *counts, double *partials, float *means, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsnn_mean: null context");
    if (nattr < 1 || nattr > MAX_ATTR || !x || !counts || !partials || !means) return fail(GPCC_ERR_ARG, "gsnn_mean: %d tensors (1..%d) or a null argument", nattr, MAX_ATTR);
    MeanArgs M;
    for (int j = 0; j < nattr; ++j) {
        if (counts[j] < 0 || (counts[j] > 0 && !x[j])) return fail(GPCC_ERR_ARG, "gsnn_mean: tensor %d of %lld elements", j, (long long)counts[j]);
        M.x[j] = x[j];
        M.count[j] = counts[j];      // an empty tensor's mean is 0 / 0 = NaN, as torch's
    }
    HIP_TRY(hipSetDevice(ctx->device));
    k_mean_partial<<<dim3(MEAN_PARTS, (unsigned)nattr), TB, 0, (hipStream_t)stream>>>(M, partials);
    LAUNCH_CHECK();
    k_mean_final<<<(unsigned)nattr, TB, 0, (hipStream_t)stream>>>(M, partials, means);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsnn_quantise(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *x, const int64_t *widths, const double *q0, const float *adj,
                             int64_t adj_stride, const int *adj_cols, double base, const float *means, int use_clamp, float *const *y, float *q_out,
                             void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsnn_quantise: null context");
    QArgs Q;
    GP_TRY(make_args("gsnn_quantise", n, nattr, x, x, widths, q0, adj, adj_stride, adj_cols, base, Q.P));
    if (n == 0) return GPCC_OK;
    if (!y || !q_out || !means) return fail(GPCC_ERR_ARG, "gsnn_quantise: null output or means");
    Q.means = means;
    Q.clamp = use_clamp != 0;
    int64_t lanes = 0;
    for (int j = 0; j < nattr; ++j) {
        if (!y[j]) return fail(GPCC_ERR_ARG, "gsnn_quantise: null output of attribute %d", j);
        Attr &A = Q.P.a[j];
        A.y = y[j];
        A.u = nullptr;
        const uint32_t w = A.width;
        A.vec = (w % 4 == 0 && aligned(A.x, 16) && aligned(A.y, 16)) ? 4 : (w % 2 == 0 && aligned(A.x, 8) && aligned(A.y, 8)) ? 2 : 1;
        const int64_t v = n * w / A.vec;
        lanes = v > lanes ? v : lanes;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    k_quantise<<<dim3((unsigned)cdiv(lanes, TB), (unsigned)nattr), TB, 0, (hipStream_t)stream>>>(Q, q_out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsnn_noise_forward_b(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *x, const float *const *u, const int64_t *widths, const double *q0,
                                    const float *adj, int64_t adj_stride, const int *adj_cols, double base, float *const *y, float *q_out, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsnn_noise_forward: null context");
    Args P;
    GP_TRY(make_args("gsnn_noise_forward", n, nattr, x, u, widths, q0, adj, adj_stride, adj_cols, base, P));
    if (n == 0) return GPCC_OK;
    if (!y || !q_out) return fail(GPCC_ERR_ARG, "gsnn_noise_forward: null output");
    int64_t lanes = 0;
    for (int j = 0; j < nattr; ++j) {
        if (!y[j]) return fail(GPCC_ERR_ARG, "gsnn_noise_forward: null output of attribute %d", j);
        Attr &A = P.a[j];
        A.y = y[j];
        const uint32_t w = A.width;
        A.vec = (w % 4 == 0 && aligned(A.x, 16) && aligned(A.u, 16) && aligned(A.y, 16)) ? 4 : (w % 2 == 0 && aligned(A.x, 8) && aligned(A.u, 8) && aligned(A.y, 8)) ? 2 : 1;
        const int64_t v = n * w / A.vec;
        lanes = v > lanes ? v : lanes;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    k_noise_fwd<<<dim3((unsigned)cdiv(lanes, TB), (unsigned)nattr), TB, 0, (hipStream_t)stream>>>(P, q_out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsnn_noise_forward(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *x, const float *const *u, const int64_t *widths, const double *q0,
                                  const float *adj, int64_t adj_stride, const int *adj_cols, float *const *y, float *q_out, void *stream)
{
    return gsnn_noise_forward_b(ctx, n, nattr, x, u, widths, q0, adj, adj_stride, adj_cols, 1.0, y, q_out, stream);
}

// base shifts the step, not its slope: the gradient of adj is the same for every base
extern "C" int gsnn_noise_backward_b(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *g, const float *const *u, const int64_t *widths, const double *q0,
                                     const float *adj, int64_t adj_stride, const int *adj_cols, double base, const float *grad_q, float *d_adj, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsnn_noise_backward: null context");
    Args P;
    GP_TRY(make_args("gsnn_noise_backward", n, nattr, g, u, widths, q0, adj, adj_stride, adj_cols, base, P));
    if (n == 0) return GPCC_OK;
    if (!adj || !d_adj) return fail(GPCC_ERR_ARG, "gsnn_noise_backward: null adj or output (a constant step has no gradient)");
    int lmax = 4;
    for (int j = 0; j < nattr; ++j) {
        P.a[j].vec = P.a[j].width <= 8 ? 4 : 16;
        lmax = P.a[j].vec > lmax ? P.a[j].vec : lmax;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    k_noise_bwd<<<dim3((unsigned)cdiv(n * lmax, TB), (unsigned)nattr), TB, 0, (hipStream_t)stream>>>(P, grad_q, d_adj);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsnn_noise_backward(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *g, const float *const *u, const int64_t *widths, const double *q0,
                                   const float *adj, int64_t adj_stride, const int *adj_cols, const float *grad_q, float *d_adj, void *stream)
{
    return gsnn_noise_backward_b(ctx, n, nattr, g, u, widths, q0, adj, adj_stride, adj_cols, 1.0, grad_q, d_adj, stream);
}
