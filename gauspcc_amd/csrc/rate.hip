// rate.hip -- the rate half of the 3DGS compressors' rate-distortion loss (HAC-plus/utils/entropy_models.py: Entropy_gaussian,
// Entropy_gaussian_clamp, Entropy_gaussian_mix_prob_2 / _3, Low_bound; the same code in HAC, CAT-3DGS and TC-GS's utils/entropy.py):
//   gsac_rate_forward   bits = -log2(max(L, 1e-6)) per element (or max(L, 1e-6) itself), L the Gaussian (mixture) likelihood of the bin
//   gsac_rate_backward  the analytic gradients for x, every mean_i, scale_i, prob_i and Q
//
// Per element, in float32, in the reference's expression order (torch's Normal.cdf as its CUDA kernels evaluate it):
//   Q  = max(Q, q_floor)                                          (CAT-3DGS only)
//   x' = min(max(x, xm - 15000 Q), xm + 15000 Q)                  (use_clamp; the bounds are detached)
//   s_i = max(scale_i, 1e-9), r_i = 1 / s_i
//   Phi_i(v) = 0.5 (1 + erf(((v - mean_i) r_i) * (1 / sqrt 2)))   (torch divides by the host scalar sqrt(2) as a multiply by its float32
//                                                                  reciprocal; the 1 + erf form saturates where the reference's does)
//   L = |Phi(x' + Q/2) - Phi(x' - Q/2)|, or sum_i prob_i |Phi_i(x' + Q/2) - Phi_i(x' - Q/2)| in list order (a product, then a sum: no fma)
//   L' = max(L, 1e-6), bits = -log2(L')
//
// Backward: dPhi_i/dv = K e r_i, K = 1/sqrt(2 pi), e = exp(-z^2).  Gates at the kinks are autograd's: clamp passes where lo <= x <= hi,
// where scale_i >= 1e-9, and where Q >= q_floor; abs has gradient 0 at 0; Low_bound passes iff L >= 1e-6.
//
// Operands mean_i, scale_i, prob_i and Q are each full (n, c), per-row (n) or one device value; Q may also be a host value.  Gradients of
// full operands are written per element.  Per-row gradients are summed in LDS by one thread per row, columns in order; one-value
// gradients add those row sums in row order per workgroup (double) and k_rate_reduce adds the workgroup partials in a fixed order.  No
// atomics: results are bitwise reproducible.  Nothing is read back to the host.
#include "common.hpp"

#include <math.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int KMAX = 3;
constexpr int NOPS = 1 + 3 * KMAX;        // Q, mean_i, scale_i, prob_i: the operands whose gradients may need reducing
constexpr float LOW = 1e-6f;              // Low_bound
constexpr float SCALE_FLOOR = 1e-9f;      // torch.clamp(scale, min=1e-9)
constexpr float RSQRT2 = 0.70710677f;     // float32(1.0f / float32(sqrt(2))): torch's multiply for a division by a host scalar
constexpr float KPDF = 0.3989422804014327f;   // 1 / sqrt(2 pi) = (2 / sqrt(pi)) * 0.5 * (1 / sqrt(2))
constexpr float LN2 = 0.6931471805599453f;    // torch's log2 backward: grad / (x * ln 2)

enum Kind { FULL = 0, ROW = 1, ONE = 2, HOST = 3 };

struct Op {
    const float *p;
    int kind;
};

struct Args {
    const float *x, *xm;
    Op mean[KMAX], scale[KMAX], prob[KMAX], q;
    float q_host, hw_host;                // HOST Q: its float32 value and float32(15000 Q) formed in double, as torch forms a host scalar
    float q_floor;                        // > 0: CAT-3DGS's floor
    int lkl;
    int64_t n, c;
};

__device__ __forceinline__ float load(const Op &o, int64_t e, int64_t r)
{
    return o.p[o.kind == FULL ? e : o.kind == ROW ? r : 0];
}

// the per-element inputs of one evaluation: the clamped x, half bin, and whether x, Q pass their clamps
struct Elem {
    float xc, hq;
    bool x_in, q_in;
};

// CAT-3DGS's torch.clamp(Q, min=q_floor): passes where Q >= q_floor
__device__ __forceinline__ bool floor_q(float &q, float q_floor)
{
    if (!(q_floor > 0.f)) return true;
    const bool in = q >= q_floor;
    q = q < q_floor ? q_floor : q;
    return in;
}

// x against x_mean +- hw (hw = 15000 Q), and the half bin
__device__ __forceinline__ Elem clamped(float x, float xm, float q, float hw, bool q_in)
{
    Elem E;
    E.q_in = q_in;
    const float lo = xm - hw, hi = xm + hw;
    E.x_in = x >= lo && x <= hi;
    E.xc = fminf(fmaxf(x, lo), hi);
    E.xc = x != x ? x : E.xc;             // torch.clamp keeps a NaN
    E.hq = 0.5f * q;
    return E;
}

__device__ __forceinline__ Elem element(const Args &A, int64_t e, int64_t r)
{
    if (A.q.kind == HOST) return clamped(A.x[e], A.xm[0], A.q_host, A.hw_host, true);
    float q = load(A.q, e, r);
    const bool q_in = floor_q(q, A.q_floor);
    return clamped(A.x[e], A.xm[0], q, 15000.f * q, q_in);
}

// one component: its two CDF values, their erf arguments and the reciprocal scale
struct Comp {
    float u, l, zu, zl, r, du, dl;        // du, dl = v -/+ mean at the bin's two edges
};

__device__ __forceinline__ Comp component(float xc, float hq, float mean, float scale)
{
    Comp C;
    const float s = scale < SCALE_FLOOR ? SCALE_FLOOR : scale;
    C.r = 1.f / s;
    C.du = (xc + hq) - mean;
    C.dl = (xc - hq) - mean;
    C.zu = (C.du * C.r) * RSQRT2;
    C.zl = (C.dl * C.r) * RSQRT2;
    C.u = 0.5f * (1.f + erff(C.zu));
    C.l = 0.5f * (1.f + erff(C.zl));
    return C;
}

template <int K>
__global__ __launch_bounds__(TB) void k_rate_fwd(Args A, float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= A.n * A.c) return;
    const int64_t r = e / A.c;
    const Elem E = element(A, e, r);
    float L;
    if (K == 1) {
        const Comp C = component(E.xc, E.hq, load(A.mean[0], e, r), load(A.scale[0], e, r));
        L = fabsf(C.u - C.l);
    } else {
        L = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const Comp C = component(E.xc, E.hq, load(A.mean[i], e, r), load(A.scale[i], e, r));
            const float t = load(A.prob[i], e, r) * fabsf(C.u - C.l);
            L = i == 0 ? t : L + t;
        }
    }
    const float Lb = L < LOW ? LOW : L;   // Low_bound's clamp (a NaN stays NaN)
    out[e] = A.lkl ? Lb : -log2f(Lb);
}

struct Grads {
    float *x;
    float *op[NOPS];                      // Q, mean_0..K-1, scale_0..K-1, prob_0..K-1 (slots KMAX apart); NULL: not wanted
    int kind[NOPS];
    double *part[NOPS];                   // ONE kind: a double per workgroup
};

template <int K>
__global__ __launch_bounds__(TB) void k_rate_bwd(Args A, const float *__restrict__ g, Grads G, int rows_per_block)
{
    __shared__ float red[NOPS][TB];
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t rows = min((int64_t)rows_per_block, A.n - r0);
    const int64_t span = rows * A.c;      // elements of this workgroup, contiguous from r0 * c
    const int64_t e0 = r0 * A.c;
    const int t = threadIdx.x;
    float acc[NOPS];                      // per-row sums of the row this thread owns (t < rows)
#pragma unroll
    for (int o = 0; o < NOPS; ++o) acc[o] = 0.f;

    for (int64_t c0 = 0; c0 < span; c0 += TB) {
        const int64_t le = c0 + t;
        float gv[NOPS];
#pragma unroll
        for (int o = 0; o < NOPS; ++o) gv[o] = 0.f;
        if (le < span) {
            const int64_t e = e0 + le, r = e / A.c;
            const Elem E = element(A, e, r);
            Comp C[K];
            float p[K], Li[K];
            float L = 0.f;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                C[i] = component(E.xc, E.hq, load(A.mean[i], e, r), load(A.scale[i], e, r));
                Li[i] = fabsf(C[i].u - C[i].l);
                if (K == 1) {
                    L = Li[i];
                } else {
                    p[i] = load(A.prob[i], e, r);
                    const float tt = p[i] * Li[i];
                    L = i == 0 ? tt : L + tt;
                }
            }
            // Low_bound passes iff L >= 1e-6.  The reference also passes where g < 0 (np.logical_or(x >= 1e-6, g < 0)), but it
            // multiplies that mask into a copy of g already zeroed where x < 1e-6, so the extra pass-through never changes a value.
            // For a mixture the second Low_bound sees max(L, 1e-6) >= 1e-6 and always passes.
            float gl = 0.f;
            if (L >= LOW) {
                const float go = g[e];
                gl = A.lkl ? go : (-go) / (L * LN2);
            }
            float gx = 0.f, gq = 0.f;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const float diff = C[i].u - C[i].l;
                const float sg = (float)(diff > 0.f) - (float)(diff < 0.f);   // abs: sign, 0 at 0
                const float a = (K == 1 ? gl : gl * p[i]) * sg;
                const float eu = expf(-(C[i].zu * C[i].zu)), el = expf(-(C[i].zl * C[i].zl));
                const float ak = a * KPDF;
                const float dvu = (ak * eu) * C[i].r, dvl = -((ak * el) * C[i].r);   // dbits / d(x' +- Q/2)
                gx += dvu + dvl;
                gq += 0.5f * (dvu - dvl);
                gv[1 + i] = -(dvu + dvl);                                           // mean_i
                const float dr = ak * (eu * C[i].du - el * C[i].dl);                // d / d(1 / s_i)
                const float sc = load(A.scale[i], e, r);
                gv[1 + KMAX + i] = sc >= SCALE_FLOOR ? -(dr * (C[i].r * C[i].r)) : 0.f;
                if (K > 1) gv[1 + 2 * KMAX + i] = gl * Li[i];                      // prob_i
            }
            gv[0] = E.q_in ? gq : 0.f;
            if (G.x) G.x[e] = E.x_in ? gx : 0.f;
#pragma unroll
            for (int o = 0; o < NOPS; ++o)
                if (G.op[o] && G.kind[o] == FULL) G.op[o][e] = gv[o];
        }
        // reduced operands: this chunk's values in LDS, then each row's owner adds its columns in order
#pragma unroll
        for (int o = 0; o < NOPS; ++o)
            if (G.op[o] && G.kind[o] != FULL) red[o][t] = gv[o];
        __syncthreads();
        if (t < rows) {
            const int64_t a = max((int64_t)t * A.c, c0), b = min((int64_t)(t + 1) * A.c, c0 + TB);
            for (int64_t j = a; j < b; ++j)
#pragma unroll
                for (int o = 0; o < NOPS; ++o)
                    if (G.op[o] && G.kind[o] != FULL) acc[o] += red[o][j - c0];
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 0; o < NOPS; ++o) {
        if (!G.op[o] || G.kind[o] == FULL) continue;
        if (G.kind[o] == ROW) {
            if (t < rows) G.op[o][r0 + t] = acc[o];
        } else {
            if (t < rows) red[o][t] = acc[o];   // the last chunk's reads finished at the barrier above
        }
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int o = 0; o < NOPS; ++o) {
            if (!G.op[o] || G.kind[o] != ONE) continue;
            double s = 0.0;
            for (int64_t j = 0; j < rows; ++j) s += (double)red[o][j];
            G.part[o][blockIdx.x] = s;
        }
    }
}

// one workgroup per one-value gradient: the workgroup partials in a fixed order (thread-strided, then a fixed tree)
struct Partials {
    const double *p[NOPS];
    float *out[NOPS];
};

__global__ __launch_bounds__(TB) void k_rate_reduce(Partials P, int64_t blocks)
{
    __shared__ double s[TB];
    const double *p = P.p[blockIdx.x];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < blocks; i += TB) a += p[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) P.out[blockIdx.x][0] = (float)s[0];
}

int make_args(const char *who, int k, int64_t n, int64_t c, const float *x, const float *x_mean, const float *const *mean,
              const float *const *scale, const float *const *prob, const int *kinds, const float *q, int q_kind, double q_host,
              double q_floor, int lkl, Args &A)
{
    if (k < 1 || k > KMAX) return fail(GPCC_ERR_ARG, "%s: k = %d not in [1, %d]", who, k, KMAX);
    if (n < 0 || c < 1 || n > ((int64_t)1 << 38) / c) return fail(GPCC_ERR_ARG, "%s: shape (%lld, %lld)", who, (long long)n, (long long)c);
    if (!x || !x_mean || !mean || !scale || !kinds || (k > 1 && !prob)) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    if (q_kind < FULL || q_kind > HOST || (q_kind != HOST && !q)) return fail(GPCC_ERR_ARG, "%s: Q kind %d", who, q_kind);
    memset(&A, 0, sizeof(A));
    A.x = x;
    A.xm = x_mean;
    A.n = n;
    A.c = c;
    A.lkl = lkl ? 1 : 0;
    A.q_floor = q_floor > 0.0 ? (float)q_floor : 0.f;
    A.q = Op{q, q_kind};
    if (q_kind == HOST) {
        const double qh = q_floor > 0.0 && q_host < q_floor ? q_floor : q_host;
        A.q_host = (float)qh;
        A.hw_host = (float)(15000.0 * qh);
    }
    for (int i = 0; i < k; ++i) {
        const int km = kinds[i], ks = kinds[k + i], kp = k > 1 ? kinds[2 * k + i] : ONE;
        if (km < FULL || km > ONE || ks < FULL || ks > ONE || kp < FULL || kp > ONE)
            return fail(GPCC_ERR_ARG, "%s: component %d operand kinds (%d, %d, %d)", who, i, km, ks, kp);
        if (!mean[i] || !scale[i] || (k > 1 && !prob[i])) return fail(GPCC_ERR_ARG, "%s: component %d null operand", who, i);
        A.mean[i] = Op{mean[i], km};
        A.scale[i] = Op{scale[i], ks};
        A.prob[i] = Op{k > 1 ? prob[i] : nullptr, kp};
    }
    return GPCC_OK;
}

}  // namespace

extern "C" int gsac_rate_forward(gpcc_ctx *ctx, int k, int64_t n, int64_t c, const float *x, const float *x_mean, const float *const *mean,
                                 const float *const *scale, const float *const *prob, const int *kinds, const float *q, int q_kind, double q_host,
                                 double q_floor, int return_lkl, float *out, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsac_rate_forward: null context");
    Args A;
    GP_TRY(make_args("gsac_rate_forward", k, n, c, x, x_mean, mean, scale, prob, kinds, q, q_kind, q_host, q_floor, return_lkl, A));
    if (!out) return fail(GPCC_ERR_ARG, "gsac_rate_forward: null output");
    if (n == 0) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)cdiv(n * c, TB);
    switch (k) {
    case 1: k_rate_fwd<1><<<blocks, TB, 0, st>>>(A, out); break;
    case 2: k_rate_fwd<2><<<blocks, TB, 0, st>>>(A, out); break;
    default: k_rate_fwd<3><<<blocks, TB, 0, st>>>(A, out); break;
    }
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsac_rate_backward(gpcc_ctx *ctx, int k, int64_t n, int64_t c, const float *x, const float *x_mean, const float *const *mean,
                                  const float *const *scale, const float *const *prob, const int *kinds, const float *q, int q_kind, double q_host,
                                  double q_floor, int return_lkl, const float *grad_out, float *grad_x, float *const *grad_mean,
                                  float *const *grad_scale, float *const *grad_prob, float *grad_q, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsac_rate_backward: null context");
    Args A;
    GP_TRY(make_args("gsac_rate_backward", k, n, c, x, x_mean, mean, scale, prob, kinds, q, q_kind, q_host, q_floor, return_lkl, A));
    if (!grad_out) return fail(GPCC_ERR_ARG, "gsac_rate_backward: null upstream gradient");
    if (grad_q && q_kind == HOST) return fail(GPCC_ERR_ARG, "gsac_rate_backward: a host Q has no gradient");
    Grads G;
    memset(&G, 0, sizeof(G));
    G.x = grad_x;
    G.op[0] = grad_q;
    G.kind[0] = q_kind;
    for (int i = 0; i < k; ++i) {
        G.op[1 + i] = grad_mean ? grad_mean[i] : nullptr;
        G.kind[1 + i] = A.mean[i].kind;
        G.op[1 + KMAX + i] = grad_scale ? grad_scale[i] : nullptr;
        G.kind[1 + KMAX + i] = A.scale[i].kind;
        G.op[1 + 2 * KMAX + i] = k > 1 && grad_prob ? grad_prob[i] : nullptr;
        G.kind[1 + 2 * KMAX + i] = A.prob[i].kind;
    }
    bool any = G.x != nullptr;
    int nones = 0;
    for (int o = 0; o < NOPS; ++o) {
        any = any || G.op[o];
        nones += G.op[o] && G.kind[o] == ONE;
    }
    if (!any) return GPCC_OK;
    if (n == 0) {                         // the one-value gradients are empty sums
        HIP_TRY(hipSetDevice(ctx->device));
        for (int o = 0; o < NOPS; ++o)
            if (G.op[o] && G.kind[o] == ONE) HIP_TRY(hipMemsetAsync(G.op[o], 0, sizeof(float), (hipStream_t)stream));
        return GPCC_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int rows_per_block = c >= TB ? 1 : (int)(TB / c);
    const int64_t blocks = cdiv(n, (int64_t)rows_per_block);
    if (blocks > INT32_MAX) return fail(GPCC_ERR_ARG, "gsac_rate_backward: %lld rows", (long long)n);
    Partials P;
    memset(&P, 0, sizeof(P));
    if (nones) {
        if (!alloc) return fail(GPCC_ERR_ARG, "gsac_rate_backward: a one-value gradient needs the workspace allocator");
        double *ws;
        GP_TRY(caller_alloc(alloc, alloc_user, (size_t)nones * (size_t)blocks * sizeof(double), &ws, "gsac_rate_backward"));
        int j = 0;
        for (int o = 0; o < NOPS; ++o)
            if (G.op[o] && G.kind[o] == ONE) {
                G.part[o] = ws + (int64_t)j * blocks;
                P.p[j] = G.part[o];
                P.out[j] = G.op[o];
                ++j;
            }
    }
    switch (k) {
    case 1: k_rate_bwd<1><<<(unsigned)blocks, TB, 0, st>>>(A, grad_out, G, rows_per_block); break;
    case 2: k_rate_bwd<2><<<(unsigned)blocks, TB, 0, st>>>(A, grad_out, G, rows_per_block); break;
    default: k_rate_bwd<3><<<(unsigned)blocks, TB, 0, st>>>(A, grad_out, G, rows_per_block); break;
    }
    LAUNCH_CHECK();
    if (nones) {
        k_rate_reduce<<<nones, TB, 0, st>>>(P, blocks);
        LAUNCH_CHECK();
    }
    return GPCC_OK;
}

// ---- the channel-wise context chain of CAT-3DGS's training branch (CAT-3DGS/gaussian_renderer/__init__.py:92-123) ------------------------
// Every stage of the chain -- the feat groups, scaling, offsets -- priced in one launch and differentiated in one: in training the "decoded"
// channels a stage's MLP reads are the noisy feat itself, so once the MLPs have run the stages do not depend on one another.  Per element
// the math is element() / component() above with k = 1 and a per-row Q: mean = ctx + dmean and scale = ctx + dscale are one rounded add
// each, the offsets' bits are multiplied by the anchor's offset mask.  The contract is in include/gauspcc.h.
namespace {

constexpr int CR_STAGES = 8;
constexpr int CR_CH = 64;
constexpr int CR_COLS = CR_STAGES * CR_CH;            // the widest bits row
constexpr int CR_WIDTH = 2 * CR_COLS + 64;            // the widest ctx row
constexpr int CR_WORDS = (CR_WIDTH + 31) / 32;

struct CStage {
    const float *res;         // (m, 2 ch) or NULL
    float *d_res;             // backward: (m, 2 ch) or NULL
    int out0;                 // first column of bits
    int attr, col, ch, mean_col, scale_col;
};

struct CArgs {
    const float *ctx, *x[3], *q, *xm, *mask;
    int64_t ctx_stride, m;
    int width[3];             // F, 6, 3 K
    int W, C, K, S;
    float q_floor;
    CStage st[CR_STAGES];
};

struct CGrads {
    float *x[3], *ctx, *q, *mask;
    uint32_t covered[CR_WORDS];   // the columns of ctx some stage reads
};

// what one element of bits reads
struct CElem {
    int s, a, j, ca;          // stage, attribute, column in the stage, column in the attribute
    float mean, scale, mk;    // mk: the offsets mask (1 elsewhere)
    bool masked;
    Elem E;
    Comp P;
};

__device__ __forceinline__ CElem chain_element(const CArgs &A, int64_t r, int c)
{
    CElem X;
    X.s = 0;
    for (int s = 1; s < A.S; ++s)
        if (c >= A.st[s].out0 && c < A.st[s].out0 + A.st[s].ch) X.s = s;
    const CStage &T = A.st[X.s];
    X.a = T.attr;
    X.j = c - T.out0;
    X.ca = T.col + X.j;
    const float *row = A.ctx + r * A.ctx_stride;
    X.mean = row[T.mean_col + X.j];
    X.scale = row[T.scale_col + X.j];
    if (T.res) {
        const float *d = T.res + r * (2 * T.ch);
        X.mean = X.mean + d[X.j];
        X.scale = X.scale + d[T.ch + X.j];
    }
    float q = A.q[r * 3 + X.a];
    const bool q_in = floor_q(q, A.q_floor);
    X.E = clamped(A.x[X.a][r * A.width[X.a] + X.ca], A.xm[X.a], q, 15000.f * q, q_in);
    X.P = component(X.E.xc, X.E.hq, X.mean, X.scale);
    X.masked = X.a == 2 && A.mask;
    X.mk = X.masked ? A.mask[r * A.K + X.ca / 3] : 1.f;
    return X;
}

__global__ __launch_bounds__(TB) void k_chain_fwd(CArgs A, float *__restrict__ bits)
{
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= A.m * A.C) return;
    const int64_t r = e / A.C;
    const CElem X = chain_element(A, r, (int)(e - r * A.C));
    const float L = fabsf(X.P.u - X.P.l);
    const float Lb = L < LOW ? LOW : L;
    const float b = -log2f(Lb);
    bits[e] = X.masked ? b * X.mk : b;
}

// a workgroup per `rows` rows (rows C <= max(TB, C) <= CR_COLS elements): per-element gradients are written as they are formed, the
// per-row sums wait in LDS for their owner, which adds them with columns ascending
__global__ __launch_bounds__(TB) void k_chain_bwd(CArgs A, const float *__restrict__ g, CGrads G, int rows_per_block)
{
    __shared__ float sq[CR_COLS], sm[CR_COLS];
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int rows = (int)min((int64_t)rows_per_block, A.m - r0);
    const int span = rows * A.C;
    const int t = threadIdx.x;
    const int K3 = 3 * A.K;
    for (int le = t; le < span; le += TB) {
        const int rl = le / A.C, c = le - rl * A.C;
        const int64_t r = r0 + rl, e = r * A.C + c;
        const CElem X = chain_element(A, r, c);
        const CStage &T = A.st[X.s];
        const Comp &P = X.P;
        const float diff = P.u - P.l;
        const float L = fabsf(diff);
        float go = g[e];
        if (X.masked) {
            const float Lb = L < LOW ? LOW : L;
            sm[rl * K3 + X.ca] = go * -log2f(Lb);
            go = go * X.mk;
        }
        const float gl = L >= LOW ? (-go) / (L * LN2) : 0.f;      // Low_bound passes iff L >= 1e-6
        const float sg = (float)(diff > 0.f) - (float)(diff < 0.f);
        const float a = gl * sg;
        const float eu = expf(-(P.zu * P.zu)), el = expf(-(P.zl * P.zl));
        const float ak = a * KPDF;
        const float dvu = (ak * eu) * P.r, dvl = -((ak * el) * P.r);
        const float gx = dvu + dvl;
        const float gq = 0.5f * (dvu - dvl);
        const float gmean = -(dvu + dvl);
        const float dr = ak * (eu * P.du - el * P.dl);
        const float gscale = X.scale >= SCALE_FLOOR ? -(dr * (P.r * P.r)) : 0.f;   // the gate tests the sum scale + dscale
        sq[le] = X.E.q_in ? gq : 0.f;
        if (G.x[X.a]) G.x[X.a][r * A.width[X.a] + X.ca] = X.E.x_in ? gx : 0.f;
        if (G.ctx) {
            float *row = G.ctx + r * A.W;
            row[T.mean_col + X.j] = gmean;
            row[T.scale_col + X.j] = gscale;
        }
        if (T.d_res) {
            float *d = T.d_res + r * (2 * T.ch);
            d[X.j] = gmean;
            d[T.ch + X.j] = gscale;
        }
    }
    __syncthreads();
    if (G.q && t < rows * 3) {
        const int rl = t / 3, a = t - rl * 3;
        const int c0 = a == 0 ? 0 : a == 1 ? A.width[0] : A.width[0] + A.width[1];
        const float *v = sq + rl * A.C + c0;
        float s = 0.f;
        for (int j = 0; j < A.width[a]; ++j) s += v[j];
        G.q[(r0 + rl) * 3 + a] = s;
    }
    if (G.mask) {
        for (int i = t; i < rows * A.K; i += TB) {
            const float *v = sm + i * 3;      // (row, k): rows are K3 = 3 K apart
            G.mask[r0 * A.K + i] = (v[0] + v[1]) + v[2];
        }
    }
    if (G.ctx) {
        for (int i = t; i < rows * A.W; i += TB) {
            const int rl = i / A.W, c = i - rl * A.W;
            if (!((G.covered[c >> 5] >> (c & 31)) & 1u)) G.ctx[(r0 + rl) * A.W + c] = 0.f;
        }
    }
}

int chain_args(const char *who, int64_t m, int feat_dim, int n_offsets, const float *ctxp, int64_t ctx_stride, int ctx_width, const float *feat,
               const float *scaling, const float *offsets, const float *q, const float *x_mean, double q_floor, const float *mask,
               const gsac_rate_stage *stages, int nstages, CArgs &A, uint32_t *covered)
{
    if (m < 0 || feat_dim < 1 || feat_dim > CR_COLS || n_offsets < 1 || 3 * n_offsets > CR_COLS)
        return fail(GPCC_ERR_ARG, "%s: m = %lld, feat_dim %d, %d offsets", who, (long long)m, feat_dim, n_offsets);
    if (!stages || nstages < 1 || nstages > CR_STAGES) return fail(GPCC_ERR_ARG, "%s: %d stages (1..%d)", who, nstages, CR_STAGES);
    if (ctx_width < 1 || ctx_width > CR_WIDTH || ctx_stride < ctx_width)
        return fail(GPCC_ERR_ARG, "%s: ctx of width %d (1..%d) with row stride %lld", who, ctx_width, CR_WIDTH, (long long)ctx_stride);
    if (m > 0 && (!ctxp || !feat || !scaling || !offsets || !q || !x_mean)) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    memset(&A, 0, sizeof(A));
    A.ctx = ctxp; A.ctx_stride = ctx_stride; A.W = ctx_width; A.m = m;
    A.x[0] = feat; A.x[1] = scaling; A.x[2] = offsets;
    A.width[0] = feat_dim; A.width[1] = 6; A.width[2] = 3 * n_offsets;
    A.q = q; A.xm = x_mean; A.mask = mask;
    A.K = n_offsets; A.S = nstages;
    A.C = feat_dim + 6 + 3 * n_offsets;
    A.q_floor = q_floor > 0.0 ? (float)q_floor : 0.f;
    if (A.C > CR_COLS) return fail(GPCC_ERR_ARG, "%s: %d columns of bits (<= %d)", who, A.C, CR_COLS);
    if (m > ((int64_t)1 << 38) / A.C) return fail(GPCC_ERR_ARG, "%s: m = %lld", who, (long long)m);
    const int base[3] = {0, feat_dim, feat_dim + 6};
    uint32_t out_seen[(CR_COLS + 31) / 32];
    memset(out_seen, 0, sizeof(out_seen));
    memset(covered, 0, CR_WORDS * sizeof(uint32_t));
    int total = 0;
    for (int s = 0; s < nstages; ++s) {
        const gsac_rate_stage &T = stages[s];
        if (T.attr < 0 || T.attr > 2 || T.ch < 1 || T.ch > CR_CH || T.col < 0 || T.col + T.ch > A.width[T.attr] || T.mean_col < 0 ||
            T.mean_col + T.ch > ctx_width || T.scale_col < 0 || T.scale_col + T.ch > ctx_width)
            return fail(GPCC_ERR_ARG, "%s: stage %d (attribute %d, columns %d + %d, mean_col %d, scale_col %d) outside its tensors", who, s, T.attr,
                        T.col, T.ch, T.mean_col, T.scale_col);
        CStage &D = A.st[s];
        D.res = T.res; D.attr = T.attr; D.col = T.col; D.ch = T.ch; D.mean_col = T.mean_col; D.scale_col = T.scale_col;
        D.out0 = base[T.attr] + T.col;
        for (int j = 0; j < T.ch; ++j) {
            const int o = D.out0 + j, cs[2] = {T.mean_col + j, T.scale_col + j};
            if ((out_seen[o >> 5] >> (o & 31)) & 1u) return fail(GPCC_ERR_ARG, "%s: stage %d prices a column another stage prices", who, s);
            out_seen[o >> 5] |= 1u << (o & 31);
            for (int c : cs) {
                if ((covered[c >> 5] >> (c & 31)) & 1u) return fail(GPCC_ERR_ARG, "%s: stage %d reads a ctx column twice read", who, s);
                covered[c >> 5] |= 1u << (c & 31);
            }
        }
        total += T.ch;
    }
    if (total != A.C) return fail(GPCC_ERR_ARG, "%s: the stages price %d of the %d columns", who, total, A.C);
    return GPCC_OK;
}

}  // namespace

extern "C" int gsac_chain_rate_forward(gpcc_ctx *ctx, int64_t m, int feat_dim, int n_offsets, const float *ctx_dev, int64_t ctx_stride, int ctx_width,
                                       const float *feat, const float *scaling, const float *offsets, const float *q, const float *x_mean, double q_floor,
                                       const float *mask, const gsac_rate_stage *stages, int nstages, float *bits, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsac_chain_rate_forward: null context");
    CArgs A;
    uint32_t covered[CR_WORDS];
    GP_TRY(chain_args("gsac_chain_rate_forward", m, feat_dim, n_offsets, ctx_dev, ctx_stride, ctx_width, feat, scaling, offsets, q, x_mean, q_floor, mask,
                      stages, nstages, A, covered));
    if (m == 0) return GPCC_OK;
    if (!bits) return fail(GPCC_ERR_ARG, "gsac_chain_rate_forward: null output");
    const int64_t blocks = cdiv(m * A.C, TB);
    if (blocks > INT32_MAX) return fail(GPCC_ERR_ARG, "gsac_chain_rate_forward: %lld rows", (long long)m);
    HIP_TRY(hipSetDevice(ctx->device));
    k_chain_fwd<<<(unsigned)blocks, TB, 0, (hipStream_t)stream>>>(A, bits);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsac_chain_rate_backward(gpcc_ctx *ctx, int64_t m, int feat_dim, int n_offsets, const float *ctx_dev, int64_t ctx_stride, int ctx_width,
                                        const float *feat, const float *scaling, const float *offsets, const float *q, const float *x_mean, double q_floor,
                                        const float *mask, const gsac_rate_stage *stages, int nstages, const float *grad_bits, float *d_feat,
                                        float *d_scaling, float *d_offsets, float *d_ctx, float *const *d_res, float *d_q, float *d_mask, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsac_chain_rate_backward: null context");
    CArgs A;
    CGrads G;
    memset(&G, 0, sizeof(G));
    GP_TRY(chain_args("gsac_chain_rate_backward", m, feat_dim, n_offsets, ctx_dev, ctx_stride, ctx_width, feat, scaling, offsets, q, x_mean, q_floor, mask,
                      stages, nstages, A, G.covered));
    if (d_mask && !mask) return fail(GPCC_ERR_ARG, "gsac_chain_rate_backward: d_mask without a mask");
    if (m == 0) return GPCC_OK;
    if (!grad_bits) return fail(GPCC_ERR_ARG, "gsac_chain_rate_backward: null upstream gradient");
    G.x[0] = d_feat; G.x[1] = d_scaling; G.x[2] = d_offsets;
    G.ctx = d_ctx; G.q = d_q; G.mask = d_mask;
    bool any = d_feat || d_scaling || d_offsets || d_ctx || d_q || d_mask;
    for (int s = 0; s < nstages; ++s) {
        A.st[s].d_res = d_res && A.st[s].res ? d_res[s] : nullptr;
        any = any || A.st[s].d_res;
    }
    if (!any) return GPCC_OK;
    const int rows_per_block = A.C >= TB ? 1 : TB / A.C;
    const int64_t blocks = cdiv(m, (int64_t)rows_per_block);
    if (blocks > INT32_MAX) return fail(GPCC_ERR_ARG, "gsac_chain_rate_backward: %lld rows", (long long)m);
    HIP_TRY(hipSetDevice(ctx->device));
    k_chain_bwd<<<(unsigned)blocks, TB, 0, (hipStream_t)stream>>>(A, grad_bits, G, rows_per_block);
    LAUNCH_CHECK();
    return GPCC_OK;
}
