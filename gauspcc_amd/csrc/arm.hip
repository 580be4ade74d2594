// arm.hip -- the rate of CAT-3DGS's quantised tri-plane latents under its Cool-Chic style auto-regressive model (scene/arm.py: get_neighbor,
// ArmMLP, get_mu_scale, compute_rate; scene/triplane.py: get_density):
//   gsarm_rate_forward   per latent: rate = -log2 p, its fixed-order sum, and the (mu, scale) maps the entropy coder reads
//   gsarm_rate_backward  the analytic gradients for every latent and every w and b of the MLP
//
// Per latent y[c, h, w] of a level [C, H, W], in float32, one lane per latent:
//   ctx_i = y[c, h - 2 + i / 5, w - 2 + i % 5], i = 0..11, zero outside the plane: the causal half of a 5 x 5 window inside channel c
//   a layer is x W^T + b, plus x where its input and output widths agree (hidden layers only), a ReLU behind every hidden layer;
//   a sum is an fmaf chain over the inputs in order, then + b (then + x)
//   (mu, ls) = MLP(ctx), s = exp(-0.5 clamp(ls, -10, 13.8155))
//   F(t) = 0.5 - 0.5 sign(t - mu) expm1(-|t - mu| / s), p0 = F(x + 0.5) - F(x - 0.5), rate = -log2(max(p0, 2^-16))
// The weights are wave-uniform operands read straight from the parameter buffer (about 4 KB: it stays in the scalar cache).
//
// Backward: nothing but the latent is saved; each lane recomputes its hidden layers and walks them backwards in registers.  Gates
// are autograd's: the floor passes iff p0 >= 2^-16 (a latent on it contributes exactly 0 everywhere), the clamp passes iff
// -10 <= ls <= 13.8155, a ReLU passes where its output is > 0.
//   parameters: per layer the workgroup stages (dz, x) of its latents in LDS, transposed, and forms dW = dz^T x and db over the tile
//     in float32 -- the reference's shape on the fp32 matrix pipe (every layer is one 16 x 16 tile, the latents are k), any other
//     shape with thread (j, i) adding dz_j x_i -- then adds the tile to its sum in double.  Workgroups are persistent (a fixed grid
//     strides over the tiles, and carries its sums from one level to the next), so the partials are grid x parameters doubles
//     whatever the latent count; k_arm_reduce adds them in a fixed order.
//   latents: the direct part through x is written at once; the 12 context gradients of every latent go to a scratch of 12 planes
//     of the level, and k_arm_gather gives each latent its own plus those of the 12 later latents whose context holds it, in
//     context order.  No atomics anywhere: bitwise reproducible.  Nothing is read back to the host.
#include "arm_dev.hpp"

using namespace gpcc;
using namespace gpcc::armdev;

namespace {

constexpr int GRID_MAX = 1024;            // persistent workgroups per launch
constexpr float P_FLOOR = 1.52587890625e-05f;       // 2^-16
constexpr float LN2 = 0.6931471805599453f;          // torch's log2 backward: grad / (x * ln 2)

// (the network's description, load_ctx, mlp_fwd and the scale formula: arm_dev.hpp, shared with the latent coder)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Rate {
    float s, p0, rate, du, dl;
    bool ls_in;
};

__device__ __forceinline__ Rate rate_of(float x, float mu, float ls)
{
    Rate R;
    R.ls_in = ls >= LS_MIN && ls <= LS_MAX;
    R.s = scale_of(ls);
    R.du = (x + 0.5f) - mu;
    R.dl = (x - 0.5f) - mu;
    const float fu = 0.5f - (0.5f * sgn(R.du)) * expm1f(-fabsf(R.du) / R.s);
    const float fl = 0.5f - (0.5f * sgn(R.dl)) * expm1f(-fabsf(R.dl) / R.s);
    R.p0 = fu - fl;
    const float p = R.p0 < P_FLOOR ? P_FLOOR : R.p0;      // clamp_min (a NaN stays NaN)
    R.rate = -log2f(p);
    return R;
}

template <class N>
__global__ __launch_bounds__(N::TB) void k_arm_fwd(Net net, const float *__restrict__ P, const float *__restrict__ y, int H, int W, int n,
                                                   float *__restrict__ rate, float *__restrict__ mu, float *__restrict__ scale,
                                                   double *__restrict__ part)
{
    constexpr int TB = N::TB;
    __shared__ double red[TB];
    const int t = threadIdx.x, ntiles = (n + TB - 1) / TB, nl = N::nl(net);
    double acc = 0.0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int e = tile * TB + t;
        if (e >= n) continue;
        float h[N::NL + 1][N::W];
        const float x = load_ctx(y, e, true, H, W, h[0]);
        mlp_fwd<N>(net, P, h);
        const Rate R = rate_of(x, h[nl][0], h[nl][1]);
        if (rate) rate[e] = R.rate;
        if (mu) mu[e] = h[nl][0];
        if (scale) scale[e] = R.s;
        acc += (double)R.rate;
    }
    if (!part) return;
    red[t] = acc;                         // a lane's tiles in order, then a fixed tree
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_arm_sum(const double *__restrict__ part, int count, float *__restrict__ out)
{
    __shared__ double s[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) a += part[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)s[0];
}

template <class N>
__global__ __launch_bounds__(N::TB) void k_arm_bwd(Net net, const float *__restrict__ P, const float *__restrict__ y, int H, int W, int n,
                                                   const float *__restrict__ g, int g_each, float *__restrict__ gy, float *__restrict__ gctx,
                                                   double *__restrict__ part, int carry)
{
    constexpr int TB = N::TB, LD = TB + 4, KPT = N::KPT;   // rows of LD floats: 16-byte aligned, and rows 4 banks apart
    __shared__ __attribute__((aligned(16))) float sx[N::W][LD];
    __shared__ __attribute__((aligned(16))) float sdz[N::W][LD];
    const int t = threadIdx.x, ntiles = (n + TB - 1) / TB, nl = N::nl(net);
    double *mine = part ? part + (int64_t)blockIdx.x * net.np : nullptr;
    // a tile's sums are float32, the tiles add up in double.  Vector path: thread q owns element q of a layer's w (four chains of every
    // fourth latent) and thread j < nout its b.  Matrix path: wave v takes latents 64 v .. 64 v + 63 of the tile; dW = dz^T x is a
    // 16 x 16 x 4 product per four latents (A = dz^T: lane (j, k) reads dz_j of latent k; B = x: lane (i, k) reads x_i), db the same
    // product against ones; lane (i = lane & 15, g = lane >> 4) holds rows j = 4 g .. 4 g + 3 of column i.  Rows and columns beyond
    // the layer's widths read stale LDS and are never used.
    constexpr bool MF = N::MFMA;
    constexpr int NA = MF ? 4 : KPT, NB = MF ? 4 : 1;
    double aw[N::NL][NA], ab[N::NL][NB];
#pragma unroll N::UL
    for (int l = 0; l < N::NL; ++l) {
        const int nin = l < nl ? N::dim(net, l) : 0, nout = l < nl ? N::dim(net, l + 1) : 0;
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int q = t + k * TB;
            aw[l][k] = !MF && mine && carry && q < nout * nin ? mine[net.wo[l] + q] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) ab[l][k] = !MF && mine && carry && t < nout ? mine[net.bo[l] + t] : 0.0;
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int e = tile * TB + t;
        const bool live = e < n;
        float h[N::NL + 1][N::W], dz[N::W];
        const float x = load_ctx(y, e, live, H, W, h[0]);
        mlp_fwd<N>(net, P, h);
        const Rate R = rate_of(x, h[nl][0], h[nl][1]);
        // d rate / d p0 through -log2 and the floor; everything below is a multiple of it
        const float go = live ? g[g_each ? e : 0] : 0.f;
        const float gp = live && R.p0 >= P_FLOOR ? (-go) / (R.p0 * LN2) : 0.f;
        const float eu = expf(-fabsf(R.du) / R.s), el = expf(-fabsf(R.dl) / R.s);
        const float su = sgn(R.du), sl = sgn(R.dl);
        const float gx = gp * ((0.5f * (su * su) * eu - 0.5f * (sl * sl) * el) / R.s);
#pragma unroll N::UW
        for (int j = 0; j < N::W; ++j) dz[j] = 0.f;
        dz[0] = -gx;
        dz[1] = R.ls_in ? gp * ((0.25f * (R.du * eu - R.dl * el)) / R.s) : 0.f;
        if (gy && live) gy[e] = gx;
#pragma unroll N::UL
        for (int l = N::NL - 1; l >= 0; --l) {
            if (l >= nl) continue;
            const int nin = N::dim(net, l), nout = N::dim(net, l + 1);
            const bool res = l < nl - 1 && nin == nout;
            if (mine) {
                __syncthreads();          // the layer before has been read
#pragma unroll N::UW
                for (int i = 0; i < nin; ++i) sx[i][t] = h[l][i];
#pragma unroll N::UW
                for (int j = 0; j < nout; ++j) sdz[j][t] = dz[j];
                __syncthreads();
                if constexpr (MF) {
                    const int lane = t & 63, r = lane & 15;
                    const float *pa = &sdz[r][(t & ~63) + (lane >> 4)], *pb = &sx[r][(t & ~63) + (lane >> 4)];
                    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, d0 = c0, d1 = c0;   // two accumulators each: the dependent latency is 40 cycles
#pragma unroll
                    for (int m = 0; m < 64; m += 8) {
                        const float a0 = pa[m], b0 = pb[m], a1 = pa[m + 4], b1 = pb[m + 4];
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c0, 0, 0, 0);
                        d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, 1.f, d0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c1, 0, 0, 0);
                        d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, 1.f, d1, 0, 0, 0);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        aw[l][k] += (double)(c0[k] + c1[k]);
                        ab[l][k] += (double)(d0[k] + d1[k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < KPT; ++k) {
                        const int q = t + k * TB;
                        if (q >= nout * nin) continue;
                        const int j = q / nin, i = q - j * nin;
                        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                        for (int m = 0; m < TB; m += 4) {
                            const float4 u = *reinterpret_cast<const float4 *>(&sdz[j][m]), v = *reinterpret_cast<const float4 *>(&sx[i][m]);
                            a0 = __builtin_fmaf(u.x, v.x, a0);
                            a1 = __builtin_fmaf(u.y, v.y, a1);
                            a2 = __builtin_fmaf(u.z, v.z, a2);
                            a3 = __builtin_fmaf(u.w, v.w, a3);
                        }
                        aw[l][k] += (double)((a0 + a1) + (a2 + a3));
                    }
                    if (t < nout) {
                        double a = ab[l][0];      // a handful of threads: the bias sums afford double throughout
                        for (int m = 0; m < TB; m += 4) {
                            const float4 u = *reinterpret_cast<const float4 *>(&sdz[t][m]);
                            a += ((double)u.x + (double)u.y) + ((double)u.z + (double)u.w);
                        }
                        ab[l][0] = a;
                    }
                }
            }
            if (l == 0 && !gctx) continue;
            const float *w = P + net.wo[l];
            float dx[N::W];
            // row by row of w (contiguous wave-uniform loads), nin independent chains: dx_i = sum over j in order, then + dz_i
#pragma unroll N::UW
            for (int i = 0; i < nin; ++i) dx[i] = w[i] * dz[0];
#pragma unroll N::UW
            for (int j = 1; j < nout; ++j)
#pragma unroll N::UW
                for (int i = 0; i < nin; ++i) dx[i] = __builtin_fmaf(w[j * nin + i], dz[j], dx[i]);
            if (res)
#pragma unroll N::UW
                for (int i = 0; i < nin; ++i) dx[i] += dz[i];
            if (l > 0) {
#pragma unroll N::UW
                for (int i = 0; i < nin; ++i) dz[i] = h[l][i] > 0.f ? dx[i] : 0.f;
            } else if (live) {
#pragma unroll N::UW
                for (int i = 0; i < nin; ++i) gctx[(int64_t)i * n + e] = dx[i];
            }
        }
    }
    if (!mine) return;
    if constexpr (MF) {
        // the four waves add their sums to the workgroup's partial one after the other: a fixed order
        const int lane = t & 63, r = lane & 15, g4 = (lane >> 4) * 4;
        for (int v = 0; v < TB / 64; ++v) {
            if ((t >> 6) == v) {
#pragma unroll
                for (int l = 0; l < N::NL; ++l) {
                    const int nin = N::dim(net, l), nout = N::dim(net, l + 1);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = g4 + k;
                        if (j >= nout) continue;
                        if (r < nin) {
                            double *p = mine + net.wo[l] + j * nin + r;
                            *p = (v > 0 || carry ? *p : 0.0) + aw[l][k];
                        }
                        if (r == 0) {
                            double *p = mine + net.bo[l] + j;
                            *p = (v > 0 || carry ? *p : 0.0) + ab[l][k];
                        }
                    }
                }
            }
            __syncthreads();
        }
    } else {
#pragma unroll N::UL
        for (int l = 0; l < N::NL; ++l) {
            const int nin = l < nl ? N::dim(net, l) : 0, nout = l < nl ? N::dim(net, l + 1) : 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                const int q = t + k * TB;
                if (q < nout * nin) mine[net.wo[l] + q] = aw[l][k];
            }
            if (t < nout) mine[net.bo[l] + t] = ab[l][0];
        }
    }
}

// the latent at (h, w) is context entry i of the latent at (h + 2 - i / 5, w + 2 - i % 5)
__global__ __launch_bounds__(256) void k_arm_gather(const float *__restrict__ gctx, int H, int W, int n, float *__restrict__ gy)
{
    const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e64 >= n) return;
    const int e = (int)e64, w = e % W, h = (e / W) % H;
    float a = gy[e];
#pragma unroll
    for (int i = 0; i < NCTX; ++i) {
        const int dh = 2 - i / MASK, dw = 2 - i % MASK;
        if (h + dh < H && w + dw >= 0 && w + dw < W) a += gctx[(int64_t)i * n + (e + dh * W + dw)];
    }
    gy[e] = a;
}

__global__ __launch_bounds__(256) void k_arm_reduce(const double *__restrict__ part, int blocks, int np, float *__restrict__ out)
{
    __shared__ double s[256];             // one workgroup per parameter: the partials thread-strided, then a fixed tree
    const int p = blockIdx.x;
    double a = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) a += part[(int64_t)b * np + p];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[p] = (float)s[0];
}

template <class N> int grid_of(const Levels &L)
{
    const int64_t tiles = cdiv(L.largest, N::TB);
    return (int)(tiles < 1 ? 1 : tiles > GRID_MAX ? GRID_MAX : tiles);
}

}  // namespace

extern "C" int gsarm_rate_forward(gpcc_ctx *ctx, int n_levels, const float *const *y, const int *channels, const int *heights, const int *widths,
                                  const float *params, int n_layers, const int *dims, float *rate, float *rate_sum, float *mu, float *scale,
                                  gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsarm_rate_forward: null context");
    Net net;
    bool spec;
    Levels L;
    GP_TRY(make_net("gsarm_rate_forward", n_layers, dims, net, spec));
    GP_TRY(make_levels("gsarm_rate_forward", n_levels, y, channels, heights, widths, L));
    if (!params) return fail(GPCC_ERR_ARG, "gsarm_rate_forward: null parameters");
    if (!rate && !rate_sum && !mu && !scale) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (L.total == 0) {
        if (rate_sum) HIP_TRY(hipMemsetAsync(rate_sum, 0, sizeof(float), st));
        return GPCC_OK;
    }
    const int grid = spec ? grid_of<Spec>(L) : grid_of<Any>(L);
    double *part = nullptr;
    if (rate_sum) {
        if (!alloc) return fail(GPCC_ERR_ARG, "gsarm_rate_forward: the sum needs the workspace allocator");
        GP_TRY(caller_alloc(alloc, alloc_user, (size_t)n_levels * grid * sizeof(double), &part, "gsarm_rate_forward"));
    }
    int64_t off = 0;
    for (int v = 0; v < n_levels; ++v) {
        const int n = (int)L.n[v];
        float *r = rate ? rate + off : nullptr, *m = mu ? mu + off : nullptr, *s = scale ? scale + off : nullptr;
        double *p = part ? part + (int64_t)v * grid : nullptr;
        if (spec) k_arm_fwd<Spec><<<grid, Spec::TB, 0, st>>>(net, params, y[v], heights[v], widths[v], n, r, m, s, p);
        else k_arm_fwd<Any><<<grid, Any::TB, 0, st>>>(net, params, y[v], heights[v], widths[v], n, r, m, s, p);
        LAUNCH_CHECK();
        off += L.n[v];
    }
    if (rate_sum) {
        k_arm_sum<<<1, 256, 0, st>>>(part, n_levels * grid, rate_sum);
        LAUNCH_CHECK();
    }
    return GPCC_OK;
}

extern "C" int gsarm_rate_backward(gpcc_ctx *ctx, int n_levels, const float *const *y, const int *channels, const int *heights, const int *widths,
                                   const float *params, int n_layers, const int *dims, const float *grad_rate, int grad_is_scalar,
                                   float *const *grad_y, float *grad_params, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsarm_rate_backward: null context");
    Net net;
    bool spec;
    Levels L;
    GP_TRY(make_net("gsarm_rate_backward", n_layers, dims, net, spec));
    GP_TRY(make_levels("gsarm_rate_backward", n_levels, y, channels, heights, widths, L));
    if (!params || !grad_rate) return fail(GPCC_ERR_ARG, "gsarm_rate_backward: null argument");
    bool any_y = false;
    for (int v = 0; v < n_levels; ++v) any_y = any_y || (grad_y && grad_y[v]);
    if (!any_y && !grad_params) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (L.total == 0) {
        if (grad_params) HIP_TRY(hipMemsetAsync(grad_params, 0, (size_t)net.np * sizeof(float), st));
        return GPCC_OK;
    }
    if (!alloc) return fail(GPCC_ERR_ARG, "gsarm_rate_backward: null workspace allocator");
    const int grid = spec ? grid_of<Spec>(L) : grid_of<Any>(L);
    float *gctx = nullptr;
    double *part = nullptr;
    GP_TRY(caller_block(alloc, alloc_user, "gsarm_rate_backward", [&](Carver &c) {
        if (any_y) gctx = c.take<float>((size_t)NCTX * L.largest);
        if (grad_params) part = c.take<double>((size_t)grid * net.np);
    }));
    int64_t off = 0;
    for (int v = 0; v < n_levels; ++v) {
        const int n = (int)L.n[v], H = heights[v], W = widths[v];
        float *gy = grad_y ? grad_y[v] : nullptr;
        const float *g = grad_is_scalar ? grad_rate : grad_rate + off;
        if (spec) k_arm_bwd<Spec><<<grid, Spec::TB, 0, st>>>(net, params, y[v], H, W, n, g, !grad_is_scalar, gy, gy ? gctx : nullptr, part, v > 0);
        else k_arm_bwd<Any><<<grid, Any::TB, 0, st>>>(net, params, y[v], H, W, n, g, !grad_is_scalar, gy, gy ? gctx : nullptr, part, v > 0);
        LAUNCH_CHECK();
        if (gy) {
            k_arm_gather<<<(unsigned)cdiv(n, 256), 256, 0, st>>>(gctx, H, W, n, gy);
            LAUNCH_CHECK();
        }
        off += L.n[v];
    }
    if (grad_params) {
        k_arm_reduce<<<net.np, 256, 0, st>>>(part, grid, net.np, grad_params);
        LAUNCH_CHECK();
    }
    return GPCC_OK;
}
