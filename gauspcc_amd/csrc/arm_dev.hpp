// arm_dev.hpp -- what the rate term (arm.hip) and the latent coder (arm_codec.hip) of CAT-3DGS's auto-regressive model share: the network's
// description, a lane's causal context, the MLP forward and the scale formula.  ONE definition each, so that the (mu, scale) a decoder
// evaluates are bit for bit those the encoder coded under and those gsarm_rate_forward returns.
#pragma once
#include "common.hpp"

#include <math.h>

namespace gpcc {
namespace armdev {

constexpr int NCTX = 12;                  // (5 * 5 - 1) / 2
constexpr int MASK = 5;
constexpr int MAXL = 9;                   // layers: up to eight hidden ones and the output
constexpr int MAXW = 32;
constexpr int MAX_LEVELS = 64;
constexpr int64_t MAX_LATENTS = (int64_t)1 << 30;   // per level: 32-bit latent indices
constexpr float LS_MIN = -10.f, LS_MAX = 13.8155f;

struct Net {
    int nl;                               // layers, the output layer included
    int d[MAXL + 1];                      // widths: 12, the hidden layers, 2
    int wo[MAXL], bo[MAXL];               // offsets of w (out, in) and b in the flat parameter buffer
    int np;
};

// the reference's shape, every width a compile-time constant: activations and sums live in registers
struct Spec {
    static constexpr int NL = 5, W = 16, TB = 256, KPT = 1, UL = NL, UW = W;
    static constexpr bool MFMA = true;    // parameter gradients on the fp32 matrix pipe: every layer is one 16 x 16 tile
    __device__ static constexpr int nl(const Net &) { return NL; }
    __device__ static constexpr int dim(const Net &, int l) { return l == 0 ? NCTX : l == NL ? 2 : 16; }
};
// any other shape: widths are run-time values and the per-lane arrays are private memory
struct Any {
    static constexpr int NL = MAXL, W = MAXW, TB = 128, KPT = MAXW * MAXW / TB, UL = 1, UW = 1;
    static constexpr bool MFMA = false;
    __device__ static int nl(const Net &n) { return n.nl; }
    __device__ static int dim(const Net &n, int l) { return n.d[l]; }
};

// a lane's latent and its causal context; a lane beyond the level reads zeros
__device__ __forceinline__ float load_ctx(const float *__restrict__ y, int e, bool live, int H, int W, float *ctx)
{
    const int w = live ? e % W : 0, h = live ? (e / W) % H : 0;
    const float *row = y + ((int64_t)e - w);
#pragma unroll
    for (int i = 0; i < NCTX; ++i) {
        const int dh = i / MASK - 2, ww = w + i % MASK - 2;
        const bool ok = live && h + dh >= 0 && ww >= 0 && ww < W;
        ctx[i] = ok ? row[dh * W + ww] : 0.f;
    }
    return live ? y[e] : 0.f;
}

template <class N>
__device__ __forceinline__ void mlp_fwd(const Net &net, const float *__restrict__ P, float (&h)[N::NL + 1][N::W])
{
    const int nl = N::nl(net);
#pragma unroll N::UL
    for (int l = 0; l < N::NL; ++l) {
        if (l >= nl) continue;
        const int nin = N::dim(net, l), nout = N::dim(net, l + 1);
        const bool hidden = l < nl - 1, res = hidden && nin == nout;
        const float *w = P + net.wo[l], *b = P + net.bo[l];
#pragma unroll N::UW
        for (int j = 0; j < nout; ++j) {
            float a = w[j * nin] * h[l][0];   // the products first, then the bias (and x): a large bias is rounded into the sum once
#pragma unroll N::UW
            for (int i = 1; i < nin; ++i) a = __builtin_fmaf(w[j * nin + i], h[l][i], a);
            a += b[j];
            if (res) a += h[l][j];
            h[l + 1][j] = hidden && a < 0.f ? 0.f : a;    // a NaN stays NaN, as torch's relu keeps it
        }
    }
}

__device__ __forceinline__ float sgn(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }

// get_mu_scale: s = exp(-0.5 clamp(ls, -10, 13.8155))
__device__ __forceinline__ float scale_of(float ls)
{
    float lc = fminf(fmaxf(ls, LS_MIN), LS_MAX);
    lc = ls != ls ? ls : lc;              // torch.clamp keeps a NaN
    return expf(-0.5f * lc);
}

// the Laplace CDF at t - mu = d: F = 0.5 - 0.5 sign(d) expm1(-|d| / s)
__device__ __forceinline__ float laplace_cdf(float d, float s) { return 0.5f - (0.5f * sgn(d)) * expm1f(-fabsf(d) / s); }

struct Levels {
    int count;
    int64_t n[MAX_LEVELS], total, largest;
};

inline int make_net(const char *who, int n_layers, const int *dims, Net &net, bool &spec)
{
    if (!dims || n_layers < 2 || n_layers > MAXL) return fail(GPCC_ERR_ARG, "%s: %d layers outside [2, %d]", who, n_layers, MAXL);
    if (dims[0] != NCTX || dims[n_layers] != 2) return fail(GPCC_ERR_ARG, "%s: %d inputs, %d outputs (12 and 2 supported)", who, dims[0], dims[n_layers]);
    memset(&net, 0, sizeof(net));
    net.nl = n_layers;
    int off = 0;
    for (int l = 0; l <= n_layers; ++l) {
        if (l > 0 && l < n_layers && (dims[l] < 1 || dims[l] > MAXW)) return fail(GPCC_ERR_ARG, "%s: hidden width %d outside [1, %d]", who, dims[l], MAXW);
        net.d[l] = dims[l];
    }
    for (int l = 0; l < n_layers; ++l) {
        net.wo[l] = off;
        off += net.d[l] * net.d[l + 1];
        net.bo[l] = off;
        off += net.d[l + 1];
    }
    net.np = off;
    spec = n_layers == Spec::NL;
    for (int l = 1; spec && l < n_layers; ++l) spec = dims[l] == 16;
    return GPCC_OK;
}

inline int make_levels(const char *who, int n_levels, const float *const *y, const int *C, const int *H, const int *W, Levels &L)
{
    if (n_levels < 0 || n_levels > MAX_LEVELS) return fail(GPCC_ERR_ARG, "%s: %d levels outside [0, %d]", who, n_levels, MAX_LEVELS);
    if (n_levels && (!y || !C || !H || !W)) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    L.count = n_levels;
    L.total = L.largest = 0;
    for (int v = 0; v < n_levels; ++v) {
        if (C[v] < 1 || H[v] < 1 || W[v] < 1 || (int64_t)C[v] * H[v] > MAX_LATENTS || (int64_t)C[v] * H[v] * W[v] > MAX_LATENTS)
            return fail(GPCC_ERR_ARG, "%s: level %d of %d x %d x %d", who, v, C[v], H[v], W[v]);
        if (!y[v]) return fail(GPCC_ERR_ARG, "%s: level %d is null", who, v);
        L.n[v] = (int64_t)C[v] * H[v] * W[v];
        L.total += L.n[v];
        L.largest = L.n[v] > L.largest ? L.n[v] : L.largest;
    }
    return GPCC_OK;
}

}  // namespace armdev
}  // namespace gpcc
