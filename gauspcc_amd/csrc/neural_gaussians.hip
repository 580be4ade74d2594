// neural_gaussians.hip -- generate_neural_gaussians on gfx950 (inference path; the training path at the end of the file): SURVEY.md 8(f) row 2.
//
// Reference: src/gs_compress/HAC/gaussian_renderer/__init__.py:25-172 (the same function in HAC-plus / TC-GS / CAT-3DGS):
// per visible anchor the view direction and distance, the optional feature bank, three two-layer MLPs (opacity / colour /
// covariance) on [feat | view | dist], masking by neural opacity, and the assembly of the surviving Gaussians' position,
// colour, opacity, scale and rotation.  In PyTorch that is ~40 small kernels and an (n K, 22) concatenation that is
// written, masked and split again; here
//   k_anchor_mlps   one lane per anchor: inputs and hidden activations in registers, weights through the scalar cache
//                   (every lane of a wave reads the same weight -> SGPR operands), the K x (1 + 3 + 7) head outputs and
//                   the per-Gaussian keep flag written once;
//   scan            exclusive scan of the flags;
//   k_assemble      one lane per kept Gaussian writes its 14 output floats.
// fp32 throughout; RD evaluation tolerates rounding differences (PSNR within 0.01 dB), so unlike the codec kernels this
// arithmetic is not pinned to an order -- the test compares against the same operations in PyTorch fp32 with a tolerance.
#include "primitives.hpp"

using namespace gpcc;

namespace {

constexpr int TB = 256;

struct Mlp { const float *w1, *b1, *w2, *b2; };   // Linear(din, F) - ReLU - Linear(F, dout); nn.Linear layouts

struct NGArgs {
    const float *anchor, *feat, *offsets, *scaling, *mask;   // (n,3) (n,F) (n,K,3) (n,6) (n,K)
    const int32_t *rows;                                      // anchors of the model this call is about (visible_mask as an index list), or null: rows 0 .. n - 1
    int64_t n;
    int K;
    const float *cam;                // camera centre (3), device memory: read by the kernels, no copy to the host in front of the call
    Mlp bank, opacity, cov, color;   // bank.w1 == nullptr: no feature bank
    float *nopa;                     // (n K)     neural opacity * mask
    float *dense;                    // (n K, 10) colour (3) | scale_rot (7)
    uint32_t *keep;                  // (n K)     neural opacity > 0
    int mafter;                      // training path (TR): HAC++'s order -- keep = tanh > 0, the mask applied to the kept rows' opacity and scale
    uint8_t *keep8;                  // training path (TR): the keep flags as bool (n K)
};

template <int F, int DIN>
__device__ __forceinline__ void hidden_layer(const float (&x)[DIN], const Mlp &m, float (&h)[F])
{
#pragma unroll 2
    for (int c = 0; c < F; ++c) {
        float a = m.b1[c];
        const float *w = m.w1 + c * DIN;
#pragma unroll
        for (int k = 0; k < DIN; ++k) a = __builtin_fmaf(x[k], w[k], a);
        h[c] = a > 0.0f ? a : 0.0f;
    }
}

template <int F>
__device__ __forceinline__ float out_unit(const float (&h)[F], const Mlp &m, int j)
{
    float a = m.b2[j];
    const float *w = m.w2 + j * F;
#pragma unroll
    for (int k = 0; k < F; ++k) a = __builtin_fmaf(h[k], w[k], a);
    return a;
}

template <int F, bool TR = false>
__global__ __launch_bounds__(TB) void k_anchor_mlps(NGArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= a.n) return;
    const int64_t src = a.rows ? a.rows[i] : i;     // row of the model's tensors; outputs are indexed by i
    constexpr int DIN = F + 4;
    float x[DIN];
    // ob_view / ob_dist (:116-118)
    const float vx = a.anchor[3 * src] - a.cam[0], vy = a.anchor[3 * src + 1] - a.cam[1], vz = a.anchor[3 * src + 2] - a.cam[2];
    const float dist = sqrtf(vx * vx + vy * vy + vz * vz);
    x[F] = vx / dist; x[F + 1] = vy / dist; x[F + 2] = vz / dist; x[F + 3] = dist;
#pragma unroll
    for (int k = 0; k < F; ++k) x[k] = a.feat[src * F + k];
    if (a.bank.w1) {   // view-adaptive feature (:121-132): softmax-weighted mix of the feature at strides 4 / 2 / 1
        float hb[F];
        const float cv[4] = {x[F], x[F + 1], x[F + 2], x[F + 3]};
        hidden_layer<F, 4>(cv, a.bank, hb);
        float z0 = out_unit<F>(hb, a.bank, 0), z1 = out_unit<F>(hb, a.bank, 1), z2 = out_unit<F>(hb, a.bank, 2);
        const float zm = fmaxf(z0, fmaxf(z1, z2));
        z0 = expf(z0 - zm); z1 = expf(z1 - zm); z2 = expf(z2 - zm);
        const float zs = z0 + z1 + z2;
        z0 /= zs; z1 /= zs; z2 /= zs;
        float y[F];
#pragma unroll
        for (int k = 0; k < F; ++k) y[k] = x[(k % (F / 4)) * 4] * z0 + x[(k % (F / 2)) * 2] * z1 + x[k] * z2;
#pragma unroll
        for (int k = 0; k < F; ++k) x[k] = y[k];
    }
    float h[F];
    const int K = a.K;
    // opacity: tanh head, times the binary grid mask; a Gaussian survives when the product is positive (:136-141)
    hidden_layer<F, DIN>(x, a.opacity, h);
    for (int j = 0; j < K; ++j) {
        const float t = tanhf(out_unit<F>(h, a.opacity, j));
        const float o = TR && a.mafter ? t : t * a.mask[src * K + j];
        a.nopa[i * K + j] = o;
        a.keep[i * K + j] = o > 0.0f ? 1u : 0u;
        if (TR) a.keep8[i * K + j] = o > 0.0f ? 1 : 0;
    }
    // colour: sigmoid head (:147-148)
    hidden_layer<F, DIN>(x, a.color, h);
    for (int j = 0; j < 3 * K; ++j) {
        const float v = out_unit<F>(h, a.color, j);
        a.dense[(i * K + j / 3) * 10 + j % 3] = 1.0f / (1.0f + expf(-v));
    }
    // covariance: linear head, 7 per Gaussian (:151-152)
    hidden_layer<F, DIN>(x, a.cov, h);
    for (int j = 0; j < 7 * K; ++j) a.dense[(i * K + j / 7) * 10 + 3 + j % 7] = out_unit<F>(h, a.cov, j);
}

struct AsmArgs {
    const float *anchor, *offsets, *scaling, *nopa, *dense;
    const int32_t *rows;
    const uint32_t *keep, *pos;
    int64_t nk;
    int K;
    float *xyz, *color, *opacity, *scale, *rot;
    const float *mask;               // TR with HAC++'s order: (n K) multiplies the kept rows' opacity and scale; otherwise null
};

template <bool TR = false>
__global__ __launch_bounds__(TB) void k_assemble(AsmArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (g >= a.nk || !a.keep[g]) return;
    const int64_t i = a.rows ? (int64_t)a.rows[g / a.K] : g / a.K;
    const int64_t gs = i * a.K + g % a.K;      // the candidate's row in the model's (n, K, 3) offsets
    const uint32_t p = a.pos[g];
    const float *d = a.dense + g * 10, *sc = a.scaling + i * 6;
    const float mk = TR && a.mask ? a.mask[gs] : 1.0f;
    a.opacity[p] = TR ? a.nopa[g] * mk : a.nopa[g];
    a.color[3 * p] = d[0]; a.color[3 * p + 1] = d[1]; a.color[3 * p + 2] = d[2];
    // scaling = scaling[3:] * sigmoid(scale_rot[:3]); rot = normalize(scale_rot[3:7]) (:166-168)
#pragma unroll
    for (int k = 0; k < 3; ++k) a.scale[3 * p + k] = TR ? sc[3 + k] * (1.0f / (1.0f + expf(-d[3 + k]))) * mk : sc[3 + k] * (1.0f / (1.0f + expf(-d[3 + k])));
    const float q0 = d[6], q1 = d[7], q2 = d[8], q3 = d[9];
    const float nrm = fmaxf(sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12f);   // F.normalize: x / max(|x|, eps)
    a.rot[4 * p] = q0 / nrm; a.rot[4 * p + 1] = q1 / nrm; a.rot[4 * p + 2] = q2 / nrm; a.rot[4 * p + 3] = q3 / nrm;
    // xyz = anchor + offsets * scaling[:3] (:170-171)
#pragma unroll
    for (int k = 0; k < 3; ++k) a.xyz[3 * p + k] = a.anchor[3 * i + k] + a.offsets[gs * 3 + k] * sc[k];
}


// ---- the same function on the matrix pipe (round 5) ------------------------------------------------------------------
// k_anchor_mlps spends 13.6 k scalar-operand fmas per anchor at one lane each (1.78 ms per million anchors, 15 TFLOP/s) and
// hands the K x 10 head outputs of EVERY candidate Gaussian to the assembly through HBM (400 MB written, 400 MB read) although
// about half of them are dropped.  Here a wave owns 16 anchors: [feat | view | dist] staged in its LDS slice, every layer a
// chain of v_mfma_f32_16x16x4_f32 with the bias as the initial accumulator (lane (g, e) supplies row e / output e at
// k = 4 kk + g and receives rows 4 g .. 4 g + 3 of output e), all weights of the launch in LDS at bank-conflict-free
// pitches.  Two launches around the scan of the keep flags:
//   k_ng_opacity   x -> opacity MLP -> tanh * mask -> nopa, keep                 (the flags the scan needs; 69 MFMAs per tile)
//   k_ng_emit      x again -> colour and covariance MLPs -> the tile's 16 x 10 K outputs in LDS -> the surviving Gaussians
//                  written straight to their final rows (position from the scan): no (n K, 10) intermediate, no assembly pass.
// x is rebuilt rather than kept: 200 MB of feature reads against 430 MB of x written and read back.  n_offsets <= 16 (the
// reference's configurations use 10: HAC/arguments/__init__.py:55); wider models stay on k_anchor_mlps.
typedef float f32x4n __attribute__((ext_vector_type(4)));
constexpr int NG_AUX = 9;     // anchor (3) + scaling (6) per row of a tile, k_ng_emit's LDS copy
#define NG_MF(c, a, b) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

template <int F> struct NGM {
    static constexpr int DINP = (F + 4 + 3) / 4 * 4;   // [feat | view | dist] padded to whole k-steps: 56 / 36
    static constexpr int DHP = (F + 3) / 4 * 4;        // hidden width padded: 52 / 32
    static constexpr int NT1 = (F + 15) / 16;          // hidden output tiles: 4 / 2
    static constexpr int P1 = DINP + 2, P2 = DHP + 2, PB = 6;   // LDS pitches of W1 / W2 / the bank's W1 (4 inputs)
};

struct MlpLds { const float *w1, *b1, *w2, *b2; };

// floats of one MLP's weights in LDS (first-layer pitch p1, nt2 output tiles)
template <int F> __host__ __device__ constexpr int ng_mlp_floats(int p1, int nt2) { return NGM<F>::NT1 * 16 * p1 + nt2 * 16 * NGM<F>::P2 + NGM<F>::NT1 * 16 + nt2 * 16; }

template <int F>
__device__ __forceinline__ MlpLds ng_stage(float *&sm, const Mlp &m, int din, int dinp, int p1, int dout, int nt2, int tid, int nthreads)
{
    using M = NGM<F>;
    float *W1s = sm, *W2s = W1s + M::NT1 * 16 * p1, *B1s = W2s + nt2 * 16 * M::P2, *B2s = B1s + M::NT1 * 16;
    sm = B2s + nt2 * 16;
    // (four loads in flight per trip: written as a plain loop, hipcc 7.2 waits for every element's load before it issues the next -- one HBM / L2 round trip
    //  per element, ~15 us at the head of every workgroup)
    for (int i0 = tid; i0 < M::NT1 * 16 * dinp; i0 += 4 * nthreads) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / dinp, k = i - c * dinp; v[u] = (i < M::NT1 * 16 * dinp && c < F && k < din) ? m.w1[c * din + k] : 0.0f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / dinp, k = i - c * dinp; if (i < M::NT1 * 16 * dinp) W1s[c * p1 + k] = v[u]; }
    }
    for (int i0 = tid; i0 < nt2 * 16 * M::DHP; i0 += 4 * nthreads) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / M::DHP, k = i - c * M::DHP; v[u] = (i < nt2 * 16 * M::DHP && c < dout && k < F) ? m.w2[c * F + k] : 0.0f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / M::DHP, k = i - c * M::DHP; if (i < nt2 * 16 * M::DHP) W2s[c * M::P2 + k] = v[u]; }
    }
    for (int i = tid; i < M::NT1 * 16; i += nthreads) B1s[i] = i < F ? m.b1[i] : 0.0f;
    for (int i = tid; i < nt2 * 16; i += nthreads) B2s[i] = i < dout ? m.b2[i] : 0.0f;
    return MlpLds{W1s, B1s, W2s, B2s};
}

__device__ __forceinline__ void ng_wave_sync()
{   // LDS operations of a wave execute in program order; this only keeps the compiler from moving them across a phase boundary
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The weight operands of output tile t + 1 are read from LDS while the MFMAs of tile t run -- two register sets and the scheduler held to that order
// (__builtin_amdgcn_sched_barrier): left to itself the compiler re-read BOTH operands from LDS directly in front of every pair of MFMAs, one LDS round
// trip per 64 cycles of matrix work (the same finding as in mlp2.hip: k_mlp2_mfma).
template <int NK>
__device__ __forceinline__ void ng_load_w(float (&w)[NK], const float *wr)
{
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) w[kk] = wr[4 * kk];
}
template <int NK>
__device__ __forceinline__ f32x4n ng_chain(const float (&a)[NK], const float (&w)[NK], float bias)
{
    f32x4n acc = {bias, bias, bias, bias};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) NG_MF(acc, a[kk], w[kk]);
    __builtin_amdgcn_sched_barrier(0);
    return acc;
}

// relu(x W1^T + b1) of the tile: A operands in registers, result into hs[16][P2] (columns F .. DHP - 1 come out as zeros)
template <int F, int NK>
__device__ __forceinline__ void ng_hidden(const float (&a)[NK], const float *W1s, int p1, const float *B1s, float *hs, int e, int g)
{
    using M = NGM<F>;
    f32x4n acc[M::NT1];
    float wb[2][NK];
    ng_load_w<NK>(wb[0], W1s + e * p1 + g);
#pragma unroll
    for (int t = 0; t < M::NT1; ++t) {
        if (t + 1 < M::NT1) ng_load_w<NK>(wb[(t + 1) & 1], W1s + (16 * (t + 1) + e) * p1 + g);
        acc[t] = ng_chain<NK>(a, wb[t & 1], B1s[16 * t + e]);
    }
#pragma unroll
    for (int t = 0; t < M::NT1; ++t)
        if (16 * t + e < M::DHP) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hs[(4 * g + i) * M::P2 + 16 * t + e] = acc[t][i] > 0.0f ? acc[t][i] : 0.0f;
        }
}

template <int F>
__device__ __forceinline__ f32x4n ng_out_tile(const float (&a)[NGM<F>::DHP / 4], const MlpLds &m, int t, int e, int g)
{
    using M = NGM<F>;
    float w[M::DHP / 4];
    ng_load_w<M::DHP / 4>(w, m.w2 + (16 * t + e) * M::P2 + g);
    return ng_chain<M::DHP / 4>(a, w, m.b2[16 * t + e]);
}

// the output tiles 0 .. nt - 1 of a second layer, two per trip so that the register set of a tile is a compile-time choice: fn(t, acc)
template <int F, typename FN>
__device__ __forceinline__ void ng_layer2(const float (&a)[NGM<F>::DHP / 4], const MlpLds &m, int nt, int e, int g, FN fn)
{
    using M = NGM<F>;
    constexpr int NK = M::DHP / 4;
    float w0[NK], w1[NK];
    ng_load_w<NK>(w0, m.w2 + e * M::P2 + g);
    for (int t = 0; t < nt; t += 2) {
        if (t + 1 < nt) ng_load_w<NK>(w1, m.w2 + (16 * (t + 1) + e) * M::P2 + g);
        fn(t, ng_chain<NK>(a, w0, m.b2[16 * t + e]));
        if (t + 1 < nt) {
            if (t + 2 < nt) ng_load_w<NK>(w0, m.w2 + (16 * (t + 2) + e) * M::P2 + g);
            fn(t + 1, ng_chain<NK>(a, w1, m.b2[16 * (t + 1) + e]));
        }
    }
}

// [feat | view | dist | 0] of anchors row0 .. row0 + 15 into xs[16][px] (rows past n: the last anchor again), the feature bank applied
// ROWS (a.rows != nullptr) is a template parameter, not a run-time test: hipcc 7.2 materialised the uniform `a.rows != nullptr` as a lane mask under the
// partial EXEC of the feature-load loop and branched on it again inside the divergent emission loop -- lanes that were inactive at the first place read
// rows[] through the null pointer (found by tests/test_gpu_hac_plus_codec.py on an un-decoded model: a memory fault that depended on which Gaussians survive)
template <int F, bool ROWS>
__device__ __forceinline__ void ng_build_x(const NGArgs &a, const float (&cam)[3], int64_t row0, float *xs, int px, float *hs, bool bank, const MlpLds &bk, int lane, float *aux = nullptr)
{
    using M = NGM<F>;
    const int e = lane & 15, g = lane >> 4;
    // every load of the tile is requested before the first one is used: as a run-time loop (`for (i = lane; i < 16 * F / 2; i += 64)`) the compiler
    // waited for each float2 before asking for the next -- seven dependent round trips per tile, 5 of the 7.8 us a wave spent on a tile of k_ng_opacity
    constexpr int NLD = (16 * (F / 2) + 63) / 64;
    float2 fv[NLD];
    float ax = 0.0f, ay = 0.0f, az = 0.0f, sv[6] = {};
    {
        int64_t rws[NLD];
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            const int i = lane + 64 * it, r = i / (F / 2);
            rws[it] = row0 + r < a.n ? row0 + r : a.n - 1;
            if (ROWS) rws[it] = i < 16 * (F / 2) ? (int64_t)a.rows[rws[it]] : 0;
        }
        int64_t arow = row0 + lane < a.n ? row0 + lane : a.n - 1;
        if (ROWS) arow = lane < 16 ? (int64_t)a.rows[arow] : 0;
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            const int i = lane + 64 * it, r = i / (F / 2), c2 = i - r * (F / 2);
            fv[it] = i < 16 * (F / 2) ? *reinterpret_cast<const float2 *>(a.feat + rws[it] * F + 2 * c2) : make_float2(0.0f, 0.0f);
        }
        if (lane < 16) { ax = a.anchor[3 * arow]; ay = a.anchor[3 * arow + 1]; az = a.anchor[3 * arow + 2]; }
        if (aux && lane < 16) {   // k_ng_emit: the tile's anchors and scalings, kept in LDS for the emission (aux[16][NG_AUX])
#pragma unroll
            for (int k = 0; k < 6; ++k) sv[k] = a.scaling[arow * 6 + k];
        }
    }
    if (aux && lane < 16) {
        float *q = aux + lane * NG_AUX;
        q[0] = ax; q[1] = ay; q[2] = az;
#pragma unroll
        for (int k = 0; k < 6; ++k) q[3 + k] = sv[k];
    }
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
        const int i = lane + 64 * it, r = i / (F / 2), c2 = i - r * (F / 2);
        if (i < 16 * (F / 2)) *reinterpret_cast<float2 *>(xs + r * px + 2 * c2) = fv[it];
    }
    if (lane < 16) {   // ob_view / ob_dist (:116-118)
        const float vx = ax - cam[0], vy = ay - cam[1], vz = az - cam[2];
        const float dist = sqrtf(vx * vx + vy * vy + vz * vz);
        float *x = xs + lane * px + F;
        x[0] = vx / dist; x[1] = vy / dist; x[2] = vz / dist; x[3] = dist;
        for (int k = F + 4; k < M::DINP; ++k) xs[lane * px + k] = 0.0f;
    }
    ng_wave_sync();
    if (!bank) return;
    // view-adaptive feature (:121-132): softmax(bank MLP(view, dist)) mixes the feature at strides 4 / 2 / 1
    {
        const float av[1] = {xs[e * px + F + g]};
        ng_hidden<F, 1>(av, bk.w1, M::PB, bk.b1, hs, e, g);
    }
    ng_wave_sync();
    float a2[M::DHP / 4];
#pragma unroll
    for (int kk = 0; kk < M::DHP / 4; ++kk) a2[kk] = hs[e * M::P2 + 4 * kk + g];
    const f32x4n z = ng_out_tile<F>(a2, bk, 0, e, g);
    ng_wave_sync();
    if (e < 3) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hs[(4 * g + i) * M::P2 + e] = z[i];
    }
    ng_wave_sync();
    if (lane < 16) {
        float z0 = hs[lane * M::P2], z1 = hs[lane * M::P2 + 1], z2 = hs[lane * M::P2 + 2];
        const float zm = fmaxf(z0, fmaxf(z1, z2));
        z0 = expf(z0 - zm); z1 = expf(z1 - zm); z2 = expf(z2 - zm);
        const float zs = z0 + z1 + z2;
        hs[lane * M::P2] = z0 / zs; hs[lane * M::P2 + 1] = z1 / zs; hs[lane * M::P2 + 2] = z2 / zs;
    }
    ng_wave_sync();
    constexpr int NIT = (16 * F + 63) / 64;
    float y[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = lane + 64 * it;
        if (idx < 16 * F) {
            const int r = idx / F, k = idx - r * F;
            const float *x = xs + r * px, *w = hs + r * M::P2;
            y[it] = x[(k % (F / 4)) * 4] * w[0] + x[(k % (F / 2)) * 2] * w[1] + x[k] * w[2];
        }
    }
    ng_wave_sync();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = lane + 64 * it;
        if (idx < 16 * F) { const int r = idx / F, k = idx - r * F; xs[r * px + k] = y[it]; }
    }
    ng_wave_sync();
}

template <int F, bool ROWS, bool TR = false>
__global__ __launch_bounds__(512) void k_ng_opacity(NGArgs a)
{
    using M = NGM<F>;
    extern __shared__ __attribute__((aligned(16))) float ngsm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6, e = lane & 15, g = lane >> 4;
    float *sm = ngsm;
    const bool bank = a.bank.w1 != nullptr;
    MlpLds bk = {};
    if (bank) bk = ng_stage<F>(sm, a.bank, 4, 4, M::PB, 3, 1, tid, blockDim.x);
    const MlpLds op = ng_stage<F>(sm, a.opacity, F + 4, M::DINP, M::P1, a.K, 1, tid, blockDim.x);
    __syncthreads();
    constexpr int PX = M::P1;
    float *xs = sm + wave * 16 * (PX + M::P2), *hs = xs + 16 * PX;
    const int64_t ntiles = (a.n + 15) / 16;
    const float cam[3] = {a.cam[0], a.cam[1], a.cam[2]};     // read once: inside the tile loop it was a round trip of its own per tile
    for (int64_t tile = (int64_t)blockIdx.x * waves + wave; tile < ntiles; tile += (int64_t)gridDim.x * waves) {
        const int64_t row0 = tile * 16;
        // the grid masks of this lane's four outputs: requested now, used after the MLP (their round trip is off the tile's chain)
        float mk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = row0 + 4 * g + i;
            mk[i] = 0.0f;
            if (e < a.K && row < a.n) mk[i] = a.mask[(ROWS ? (int64_t)a.rows[row] : row) * a.K + e];
        }
        ng_build_x<F, ROWS>(a, cam, row0, xs, PX, hs, bank, bk, lane);
        float a1[M::DINP / 4];
#pragma unroll
        for (int kk = 0; kk < M::DINP / 4; ++kk) a1[kk] = xs[e * PX + 4 * kk + g];
        ng_hidden<F, M::DINP / 4>(a1, op.w1, M::P1, op.b1, hs, e, g);
        ng_wave_sync();
        float a2[M::DHP / 4];
#pragma unroll
        for (int kk = 0; kk < M::DHP / 4; ++kk) a2[kk] = hs[e * M::P2 + 4 * kk + g];
        const f32x4n v = ng_out_tile<F>(a2, op, 0, e, g);
        // opacity: tanh head, times the binary grid mask; a Gaussian survives when the product is positive (:136-141)
        if (e < a.K) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t row = row0 + 4 * g + i;
                if (row < a.n) {
                    const float o = TR && a.mafter ? tanhf(v[i]) : tanhf(v[i]) * mk[i];
                    a.nopa[row * a.K + e] = o;
                    a.keep[row * a.K + e] = o > 0.0f ? 1u : 0u;
                    if (TR) a.keep8[row * a.K + e] = o > 0.0f ? 1 : 0;
                }
            }
        }
        ng_wave_sync();
    }
}

struct EmitArgs {
    const float *offsets, *scaling;
    const uint32_t *pos;
    int px;                            // pitch of the wave's tile buffer: even, >= DINP + 2 and >= 10 K
    float *xyz, *color, *opacity, *scale, *rot;
};

// NIT = candidates per lane in the emission = ceil(16 K / 64): a template parameter so that their attributes stay in registers
#ifndef NG_EMIT_LOADS_AT
#define NG_EMIT_LOADS_AT 1
#endif
template <int F, bool ROWS, int NIT, bool TR = false>
__global__ __launch_bounds__(512) void k_ng_emit(NGArgs a, EmitArgs o)
{
    using M = NGM<F>;
    extern __shared__ __attribute__((aligned(16))) float ngsm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6, e = lane & 15, g = lane >> 4;
    const int K = a.K, ntc = (3 * K + 15) / 16, ntv = (7 * K + 15) / 16, PX = o.px;
    float *sm = ngsm;
    const bool bank = a.bank.w1 != nullptr;
    MlpLds bk = {};
    if (bank) bk = ng_stage<F>(sm, a.bank, 4, 4, M::PB, 3, 1, tid, blockDim.x);
    const MlpLds col = ng_stage<F>(sm, a.color, F + 4, M::DINP, M::P1, 3 * K, ntc, tid, blockDim.x);
    const MlpLds cov = ng_stage<F>(sm, a.cov, F + 4, M::DINP, M::P1, 7 * K, ntv, tid, blockDim.x);
    __syncthreads();
    float *xs = sm + wave * 16 * (PX + M::P2 + NG_AUX), *hs = xs + 16 * PX, *aux = hs + 16 * M::P2;
    const int64_t ntiles = (a.n + 15) / 16;
    const float cam[3] = {a.cam[0], a.cam[1], a.cam[2]};     // read once: inside the tile loop it was a round trip of its own per tile
    for (int64_t tile = (int64_t)blockIdx.x * waves + wave; tile < ntiles; tile += (int64_t)gridDim.x * waves) {
        const int64_t row0 = tile * 16;
        ng_build_x<F, ROWS>(a, cam, row0, xs, PX, hs, bank, bk, lane, aux);
        // the emission's inputs (flag, position, attributes of the lane's NIT candidates): requested at NG_EMIT_LOADS_AT -- 0: where they are used, behind the
        // covariance MLP; 1: in front of it; 2: in front of both MLPs -- so that their round trip runs beside the matrix work
        const uint32_t *__restrict__ keepp = a.keep, *__restrict__ posp = o.pos;
        const float *__restrict__ nopap = a.nopa, *__restrict__ offp = o.offsets;
        bool kp[NIT];
        int64_t gis[NIT], srcs[NIT];
        int rr[NIT], jj[NIT];
        uint32_t kf[NIT], pp[NIT];
        float no[NIT], mm[NIT];
        float of[NIT][3];
        auto emission_loads = [&]() {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = lane + 64 * it;
                rr[it] = idx / K; jj[it] = idx - rr[it] * K;
                gis[it] = (row0 + rr[it]) * K + jj[it];
                kp[it] = idx < 16 * K && row0 + rr[it] < a.n;
            }
            // ONE batch: flag, position and offset of every candidate are requested together, the dropped candidates' too (anchor and scaling of the tile's
            // rows sit in LDS since ng_build_x) -- the flag -> position -> attributes chain was three dependent round trips per tile
#pragma unroll
            for (int it = 0; it < NIT; ++it) srcs[it] = ROWS ? (kp[it] ? (int64_t)a.rows[row0 + rr[it]] : 0) : (kp[it] ? row0 + rr[it] : 0);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int64_t gi = kp[it] ? gis[it] : 0;
                kf[it] = keepp[gi]; pp[it] = posp[gi]; no[it] = nopap[gi];
                mm[it] = TR && a.mafter ? a.mask[srcs[it] * K + (kp[it] ? jj[it] : 0)] : 1.0f;
#pragma unroll
                for (int k = 0; k < 3; ++k) of[it][k] = offp[(srcs[it] * K + (kp[it] ? jj[it] : 0)) * 3 + k];
            }
        };
        if (NG_EMIT_LOADS_AT == 2) emission_loads();
        float a1[M::DINP / 4];
#pragma unroll
        for (int kk = 0; kk < M::DINP / 4; ++kk) a1[kk] = xs[e * PX + 4 * kk + g];
        float a2[M::DHP / 4];
        // colour: sigmoid head (:147-148) -> columns 0 .. 3 K - 1 of the tile buffer (x is in registers now)
        ng_hidden<F, M::DINP / 4>(a1, col.w1, M::P1, col.b1, hs, e, g);
        ng_wave_sync();
#pragma unroll
        for (int kk = 0; kk < M::DHP / 4; ++kk) a2[kk] = hs[e * M::P2 + 4 * kk + g];
        ng_layer2<F>(a2, col, ntc, e, g, [&](int t, const f32x4n &v) {
            const int c = 16 * t + e;
            if (c < 3 * K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xs[(4 * g + i) * PX + c] = 1.0f / (1.0f + expf(-v[i]));
            }
        });
        ng_wave_sync();
        if (NG_EMIT_LOADS_AT == 1) emission_loads();
        // covariance: linear head, 7 per Gaussian (:151-152) -> columns 3 K .. 10 K - 1
        ng_hidden<F, M::DINP / 4>(a1, cov.w1, M::P1, cov.b1, hs, e, g);
        ng_wave_sync();
#pragma unroll
        for (int kk = 0; kk < M::DHP / 4; ++kk) a2[kk] = hs[e * M::P2 + 4 * kk + g];
        ng_layer2<F>(a2, cov, ntv, e, g, [&](int t, const f32x4n &v) {
            const int c = 16 * t + e;
            if (c < 7 * K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xs[(4 * g + i) * PX + 3 * K + c] = v[i];
            }
        });
        ng_wave_sync();
        // the surviving Gaussians of the tile, each to its final row (:160-171); the emission is bound by its loads' round trips, not by its stores
        // (HISTORY.md section 4)
        {
            float *__restrict__ oop = o.opacity, *__restrict__ ocol = o.color, *__restrict__ osc = o.scale, *__restrict__ orot = o.rot, *__restrict__ oxyz = o.xyz;
            if (NG_EMIT_LOADS_AT == 0) emission_loads();
#pragma unroll
            for (int it = 0; it < NIT; ++it) kp[it] = kp[it] && kf[it] != 0u;
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                if (kp[it]) {
                    const uint32_t p = pp[it];
                    const float *c3 = xs + rr[it] * PX + 3 * jj[it], *d = xs + rr[it] * PX + 3 * K + 7 * jj[it], *ar = aux + rr[it] * NG_AUX;
                    oop[p] = TR ? no[it] * mm[it] : no[it];
                    ocol[3 * p] = c3[0]; ocol[3 * p + 1] = c3[1]; ocol[3 * p + 2] = c3[2];
#pragma unroll
                    for (int k = 0; k < 3; ++k) osc[3 * p + k] = TR ? ar[6 + k] * (1.0f / (1.0f + expf(-d[k]))) * mm[it] : ar[6 + k] * (1.0f / (1.0f + expf(-d[k])));
                    const float q0 = d[3], q1 = d[4], q2 = d[5], q3 = d[6];
                    const float nrm = fmaxf(sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12f);
                    orot[4 * p] = q0 / nrm; orot[4 * p + 1] = q1 / nrm; orot[4 * p + 2] = q2 / nrm; orot[4 * p + 3] = q3 / nrm;
#pragma unroll
                    for (int k = 0; k < 3; ++k) oxyz[3 * p + k] = ar[k] + of[it][k] * ar[3 + k];
                }
        }
        ng_wave_sync();
    }
}

constexpr size_t NG_LDS_MAX = 160 * 1024;

template <int F> static size_t ng_lds_opacity(bool bank, int waves)
{
    using M = NGM<F>;
    return 4 * ((size_t)(bank ? ng_mlp_floats<F>(M::PB, 1) : 0) + ng_mlp_floats<F>(M::P1, 1) + (size_t)waves * 16 * (M::P1 + M::P2));
}
template <int F> static int ng_emit_pitch(int K) { const int px = std::max(NGM<F>::P1, 10 * K); return px + (px & 1); }
template <int F> static size_t ng_lds_emit(bool bank, int K, int waves)
{
    using M = NGM<F>;
    return 4 * ((size_t)(bank ? ng_mlp_floats<F>(M::PB, 1) : 0) + ng_mlp_floats<F>(M::P1, (3 * K + 15) / 16) + ng_mlp_floats<F>(M::P1, (7 * K + 15) / 16) +
                (size_t)waves * 16 * (ng_emit_pitch<F>(K) + M::P2 + NG_AUX));
}

// number of waves per workgroup for the two launches, 0 when the model does not fit the matrix-pipe path
template <int F> static int ng_mfma_waves(bool bank, int K)
{
    if (K > 16) return 0;
    for (int waves = 8; waves >= 4; waves -= 4)
        if (ng_lds_emit<F>(bank, K, waves) <= NG_LDS_MAX && ng_lds_opacity<F>(bank, waves) <= NG_LDS_MAX) return waves;
    return 0;
}

template <int F, bool ROWS, bool TR = false>
static int ng_mfma_opacity(gpcc_ctx *ctx, const NGArgs &a, int waves, hipStream_t st)
{
    const size_t lds = ng_lds_opacity<F>(a.bank.w1 != nullptr, waves);
    static PerDeviceOnce attr;
    GP_TRY(attr.run(ctx->device, [&]() -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ng_opacity<F, ROWS, TR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NG_LDS_MAX));
        return GPCC_OK;
    }));
    const unsigned grid = (unsigned)std::min<int64_t>(256, cdiv(cdiv(a.n, 16), waves));
    k_ng_opacity<F, ROWS, TR><<<grid, 64 * waves, lds, st>>>(a);
    LAUNCH_CHECK();
    return GPCC_OK;
}

template <int F, bool ROWS, int NIT, bool TR = false>
static int ng_mfma_emit_n(gpcc_ctx *ctx, const NGArgs &a, EmitArgs o, int waves, hipStream_t st)
{
    const size_t lds = ng_lds_emit<F>(a.bank.w1 != nullptr, a.K, waves);
    o.px = ng_emit_pitch<F>(a.K);
    static PerDeviceOnce attr;
    GP_TRY(attr.run(ctx->device, [&]() -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ng_emit<F, ROWS, NIT, TR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NG_LDS_MAX));
        return GPCC_OK;
    }));
    const unsigned grid = (unsigned)std::min<int64_t>(256, cdiv(cdiv(a.n, 16), waves));
    k_ng_emit<F, ROWS, NIT, TR><<<grid, 64 * waves, lds, st>>>(a, o);
    LAUNCH_CHECK();
    return GPCC_OK;
}

template <int F, bool ROWS, bool TR = false>
static int ng_mfma_emit(gpcc_ctx *ctx, const NGArgs &a, const EmitArgs &o, int waves, hipStream_t st)
{
    switch ((16 * a.K + 63) / 64) {
    case 1: return ng_mfma_emit_n<F, ROWS, 1, TR>(ctx, a, o, waves, st);
    case 2: return ng_mfma_emit_n<F, ROWS, 2, TR>(ctx, a, o, waves, st);
    case 3: return ng_mfma_emit_n<F, ROWS, 3, TR>(ctx, a, o, waves, st);
    default: return ng_mfma_emit_n<F, ROWS, 4, TR>(ctx, a, o, waves, st);
    }
}

// mlp / d_mlp order: bank, opacity, cov, colour; {w1, b1, w2, b2} each
void ng_mlps(const float *const *m, Mlp *bank, Mlp *opacity, Mlp *cov, Mlp *color)
{
    *bank = Mlp{m[0], m[1], m[2], m[3]}; *opacity = Mlp{m[4], m[5], m[6], m[7]}; *cov = Mlp{m[8], m[9], m[10], m[11]}; *color = Mlp{m[12], m[13], m[14], m[15]};
}

// the checks of the model's shape that every entry point makes; `who` names the Python function in the messages
int ng_check(const char *who, int64_t n, int feat_dim, int n_offsets, const float *const *mlp)
{
    if (feat_dim != 32 && feat_dim != 50) return fail(GPCC_ERR_ARG, "%s: feat_dim must be 32 or 50 (got %d)", who, feat_dim);
    if (n_offsets < 1 || n_offsets > 64) return fail(GPCC_ERR_ARG, "%s: bad n_offsets %d", who, n_offsets);
    if (n < 0 || n * n_offsets >= ((int64_t)1 << 31)) return fail(GPCC_ERR_ARG, "%s: too many Gaussians", who);
    for (int q = 4; q < 16; ++q)
        if (!mlp[q]) return fail(GPCC_ERR_ARG, "null MLP tensor %d", q);
    if (mlp[0] && feat_dim % 4) return fail(GPCC_ERR_ARG, "the feature bank needs feat_dim divisible by 4");
    return GPCC_OK;
}

// The launches that come per <F, ROWS, TR>, and the one place that maps the run-time triple (feat_dim, rows given, training) to the
// instantiations that exist: <32|50, true|false, false> and <32|50, false, true> -- the training path has no rows.  The three lines of ng_launch
// stand in the order rows, plain, training on purpose: it is the order of instantiation, and the compiler's inlining of the helpers the k_ng_opacity
// variants share follows it (with the training line first, four of them come out with other instruction streams).
enum NGStage { NG_OPACITY, NG_EMIT, NG_LANES };

template <int F, bool ROWS, bool TR>
int ng_launch_as(NGStage stage, gpcc_ctx *ctx, const NGArgs &a, const EmitArgs &o, int waves, hipStream_t st)
{
    if (stage == NG_OPACITY) return ng_mfma_opacity<F, ROWS, TR>(ctx, a, waves, st);
    if (stage == NG_EMIT) return ng_mfma_emit<F, ROWS, TR>(ctx, a, o, waves, st);
    k_anchor_mlps<F, TR><<<(unsigned)cdiv(a.n, TB), TB, 0, st>>>(a);
    LAUNCH_CHECK();
    return GPCC_OK;
}
int ng_launch(NGStage stage, int feat_dim, bool tr, gpcc_ctx *ctx, const NGArgs &a, const EmitArgs &o, int waves, hipStream_t st)
{
    if (a.rows) return feat_dim == 32 ? ng_launch_as<32, true, false>(stage, ctx, a, o, waves, st) : ng_launch_as<50, true, false>(stage, ctx, a, o, waves, st);
    if (!tr) return feat_dim == 32 ? ng_launch_as<32, false, false>(stage, ctx, a, o, waves, st) : ng_launch_as<50, false, false>(stage, ctx, a, o, waves, st);
    return feat_dim == 32 ? ng_launch_as<32, false, true>(stage, ctx, a, o, waves, st) : ng_launch_as<50, false, true>(stage, ctx, a, o, waves, st);
}

struct NGMode {            // what differs between gsnn_generate and gsnn_forward_train (the training path at the end of the file)
    bool tr;               // the TR kernels: bool keep flags, HAC++'s order on request
    const int32_t *rows;   // inference: NGArgs::rows
    uint32_t *pos;         // (n K + 1) the scan of the keep flags: memory of the caller (the backward's state), or null: arena
    float *nopa;           // (n K) an output of the training call, or null: arena
    int mafter; uint8_t *keep8;   // NGArgs::mafter, NGArgs::keep8
};

// The forward for n > 0 anchors: flags -> scan -> the surviving rows, and their count.
int ng_forward(gpcc_ctx *ctx, const NGMode &m, int64_t n, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
               const float *scaling, const float *mask, const float *cam_center, const float *const *mlp, float *xyz_out, float *color_out, float *opacity_out,
               float *scale_out, float *rot_out, int64_t *count_out, hipStream_t st)
{
    const int64_t nk = n * n_offsets;
    static const bool use_mfma = dev_env_int("GAUSPCC_NG_MFMA", 1) != 0;
    const int waves = !use_mfma ? 0 : feat_dim == 32 ? ng_mfma_waves<32>(mlp[0] != nullptr, n_offsets) : ng_mfma_waves<50>(mlp[0] != nullptr, n_offsets);
    GP_TRY(ctx->arena.reserve((size_t)nk * (4 + (waves ? 0 : 40) + 4 + 4) + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(keep, uint32_t, nk);
    float *nopa = m.nopa ? m.nopa : ctx->arena.take<float>(nk);
    uint32_t *pos = m.pos ? m.pos : ctx->arena.take<uint32_t>(nk + 1);
    if (!nopa || !pos) return fail(GPCC_ERR_NOMEM, "neural Gaussians workspace");
    NGArgs a = {};
    a.anchor = anchor; a.feat = feat; a.offsets = offsets; a.scaling = scaling; a.mask = mask; a.rows = m.rows; a.n = n; a.K = n_offsets; a.cam = cam_center;
    ng_mlps(mlp, &a.bank, &a.opacity, &a.cov, &a.color);
    a.nopa = nopa; a.keep = keep; a.mafter = m.mafter; a.keep8 = m.keep8;
    // the survivor count lands in pinned memory: a copy into the stack variable is staged by the runtime and holds the host until it is done -- the emission
    // was enqueued ~18 us after the scan ended
    GP_TRY(ctx->hstage.reserve(64));
    volatile uint32_t *htotal = reinterpret_cast<volatile uint32_t *>(ctx->hstage.p);
    *htotal = 0;
    const EmitArgs o = {offsets, scaling, pos, 0, xyz_out, color_out, opacity_out, scale_out, rot_out};
    if (!waves) {   // lane kernels: the head outputs go through `dense`
        TAKE(dense, float, nk * 10);
        a.dense = dense;
    }
    GP_TRY(ng_launch(waves ? NG_OPACITY : NG_LANES, feat_dim, m.tr, ctx, a, o, waves, st));
    GP_TRY(exclusive_scan_u32(ctx, st, keep, pos, nk, pos + nk));
    HIP_TRY(hipMemcpyAsync(const_cast<uint32_t *>(htotal), pos + nk, 4, hipMemcpyDeviceToHost, st));
    if (waves) {    // matrix pipe: colour / covariance and the surviving rows in one launch
        GP_TRY(ng_launch(NG_EMIT, feat_dim, m.tr, ctx, a, o, waves, st));
    } else {
        const AsmArgs b = {anchor, offsets, scaling, nopa, a.dense, m.rows, keep, pos, nk, n_offsets, xyz_out, color_out, opacity_out, scale_out, rot_out,
                           m.mafter ? mask : nullptr};
        if (m.tr) k_assemble<true><<<(unsigned)cdiv(nk, TB), TB, 0, st>>>(b);
        else k_assemble<false><<<(unsigned)cdiv(nk, TB), TB, 0, st>>>(b);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipStreamSynchronize(st));
    GP_TRY(device_error_check(ctx));
    *count_out = (int64_t)*htotal;
    return GPCC_OK;
}

}  // namespace

extern "C" int gsnn_generate(gpcc_ctx *ctx, int64_t n, const int32_t *rows, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
                             const float *scaling, const float *mask, const float *cam_center, const float *const *mlp /* 16 pointers */,
                             float *xyz_out, float *color_out, float *opacity_out, float *scale_out, float *rot_out, int64_t *count_out, void *stream)
{
    if (!ctx || !anchor || !feat || !offsets || !scaling || !mask || !cam_center || !mlp || !xyz_out || !color_out || !opacity_out || !scale_out || !rot_out || !count_out)
        return fail(GPCC_ERR_ARG, "null argument");
    *count_out = 0;
    if (n <= 0) return GPCC_OK;
    GP_TRY(ng_check("generate_neural_gaussians", n, feat_dim, n_offsets, mlp));
    HIP_TRY(hipSetDevice(ctx->device));
    return ng_forward(ctx, NGMode{false, rows, nullptr, nullptr, 0, nullptr}, n, feat_dim, n_offsets, anchor, feat, offsets, scaling, mask, cam_center, mlp, xyz_out,
                      color_out, opacity_out, scale_out, rot_out, count_out, (hipStream_t)stream);
}


// ==== training path: gsnn_forward_train / gsnn_backward ================================================================================
// The forward is the inference launches above with TR set (the HAC++ order, the bool keep flags); the scan's positions land in memory of the
// caller (the state the backward needs: keep of candidate g is pos[g + 1] != pos[g], its output row pos[g]).  Nothing of the MLPs is kept.
//
// The backward, three launches:
//   k_ngb_anchor   one lane per anchor: x, the hidden layers and the head outputs recomputed (the inference lane kernel's loops), the kept
//                  candidates' output gradients gathered through pos, dZ per head, dH = (dZ W2) * [h > 0], dX = sum dH W1, the bank and the
//                  view / dist chain back to feat and anchor; the per-anchor input gradients written with plain stores.  Per anchor it also
//                  writes the GEMM operands of the weight gradients, feature-major (column c of anchor i at c * np + i, np = n rounded up to
//                  16, rows n .. np - 1 zero): x | 1, h | 1 and dZ, dH of every MLP.
//   k_ngb_wgrad    dW = dA^T B over the anchors on the matrix pipe (v_mfma_f32_16x16x4_f32, exact fp32 products), the anchors the reduction
//                  dimension: workgroup (r, s) owns the fixed contiguous anchor range r (its size depends on n only) and the 64-row output
//                  strip s of one weight matrix, and writes one 64 x 64 partial.  The ones column of B gives the bias.
//   k_ngb_wsum     the partials of a strip added in range order.
// No float atomics: every sum has one order, so the gradients are bitwise reproducible across runs and streams.
namespace {

struct NGBArgs {
    const float *anchor, *feat, *offsets, *scaling, *mask, *cam;   // (n,3) (n,F) (n,K,3) (n,6) (n,K) (3)
    const uint32_t *pos;                                             // (n K + 1) from gsnn_forward_train
    int64_t n, np;
    int K, mafter;
    Mlp bank, opacity, cov, color;
    const float *g_xyz, *g_color, *g_opacity, *g_scale, *g_rot, *g_nopa;   // (m,3) (m,3) (m) (m,3) (m,4) (n K)
    float *d_anchor, *d_feat, *d_offsets, *d_scaling, *d_mask;              // (n,3) (n,F) (n,K,3) (n,6) (n,K)
    // GEMM operands, feature-major with pitch np
    float *X, *Hop, *Hcol, *Hcov, *dHop, *dHcol, *dHcov, *dZop, *dZcol, *dZcov;   // X: F + 5 columns, H*: F + 1, dH*: F, dZ: K / 3K / 7K
    float *Xb, *Hb, *dHb, *dZb;                                                     // bank: 5, F + 1, F, 3
};

template <int F>
__device__ __forceinline__ void ngb_store_h(const NGBArgs &a, int64_t i, const float (&h)[F], const float (&dh)[F], float *H, float *dH)
{
#pragma unroll
    for (int c = 0; c < F; ++c) { H[c * a.np + i] = h[c]; dH[c * a.np + i] = dh[c]; }
    H[F * a.np + i] = 1.0f;
}

// dh = (dz W2) * [h > 0] has been accumulated; dx += dh W1
template <int F, int DIN>
__device__ __forceinline__ void ngb_dx(const Mlp &m, float (&dh)[F], const float (&h)[F], float (&dx)[DIN])
{
#pragma unroll
    for (int c = 0; c < F; ++c) dh[c] = h[c] > 0.0f ? dh[c] : 0.0f;
#pragma unroll 2
    for (int c = 0; c < F; ++c) {
        const float *w = m.w1 + c * DIN;
#pragma unroll
        for (int k = 0; k < DIN; ++k) dx[k] = __builtin_fmaf(dh[c], w[k], dx[k]);
    }
}

template <int F>
__device__ __forceinline__ void ngb_acc_dh(const Mlp &m, int j, float dz, float (&dh)[F])
{
    const float *w = m.w2 + j * F;
#pragma unroll
    for (int c = 0; c < F; ++c) dh[c] = __builtin_fmaf(dz, w[c], dh[c]);
}

template <int F>
__global__ __launch_bounds__(TB) void k_ngb_anchor(NGBArgs a)
{
    constexpr int DIN = F + 4;
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= a.np) return;
    const bool bank = a.bank.w1 != nullptr;
    const int K = a.K;
    if (i >= a.n) {   // padding rows of the GEMM operands: zero
        for (int c = 0; c < DIN + 1; ++c) a.X[c * a.np + i] = 0.0f;
        for (int c = 0; c < F + 1; ++c) { a.Hop[c * a.np + i] = 0.0f; a.Hcol[c * a.np + i] = 0.0f; a.Hcov[c * a.np + i] = 0.0f; }
        for (int c = 0; c < F; ++c) { a.dHop[c * a.np + i] = 0.0f; a.dHcol[c * a.np + i] = 0.0f; a.dHcov[c * a.np + i] = 0.0f; }
        for (int c = 0; c < K; ++c) a.dZop[c * a.np + i] = 0.0f;
        for (int c = 0; c < 3 * K; ++c) a.dZcol[c * a.np + i] = 0.0f;
        for (int c = 0; c < 7 * K; ++c) a.dZcov[c * a.np + i] = 0.0f;
        if (bank) {
            for (int c = 0; c < 5; ++c) a.Xb[c * a.np + i] = 0.0f;
            for (int c = 0; c < F + 1; ++c) a.Hb[c * a.np + i] = 0.0f;
            for (int c = 0; c < F; ++c) a.dHb[c * a.np + i] = 0.0f;
            for (int c = 0; c < 3; ++c) a.dZb[c * a.np + i] = 0.0f;
        }
        return;
    }
    float x[DIN];
    const float vx = a.anchor[3 * i] - a.cam[0], vy = a.anchor[3 * i + 1] - a.cam[1], vz = a.anchor[3 * i + 2] - a.cam[2];
    const float dist = sqrtf(vx * vx + vy * vy + vz * vz);
    x[F] = vx / dist; x[F + 1] = vy / dist; x[F + 2] = vz / dist; x[F + 3] = dist;
#pragma unroll
    for (int k = 0; k < F; ++k) x[k] = a.feat[i * F + k];
    float bw[3] = {0.0f, 0.0f, 1.0f};
    if (bank) {   // the forward's feature bank (k_anchor_mlps), its softmax weights kept
        float hb[F];
        const float cv[4] = {x[F], x[F + 1], x[F + 2], x[F + 3]};
        hidden_layer<F, 4>(cv, a.bank, hb);
        float z0 = out_unit<F>(hb, a.bank, 0), z1 = out_unit<F>(hb, a.bank, 1), z2 = out_unit<F>(hb, a.bank, 2);
        const float zm = fmaxf(z0, fmaxf(z1, z2));
        z0 = expf(z0 - zm); z1 = expf(z1 - zm); z2 = expf(z2 - zm);
        const float zs = z0 + z1 + z2;
        bw[0] = z0 / zs; bw[1] = z1 / zs; bw[2] = z2 / zs;
        float y[F];
#pragma unroll
        for (int k = 0; k < F; ++k) y[k] = x[(k % (F / 4)) * 4] * bw[0] + x[(k % (F / 2)) * 2] * bw[1] + x[k] * bw[2];
#pragma unroll
        for (int k = 0; k < F; ++k) x[k] = y[k];
    }
#pragma unroll
    for (int k = 0; k < DIN; ++k) a.X[k * a.np + i] = x[k];
    a.X[DIN * a.np + i] = 1.0f;
    float sc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) sc[k] = a.scaling[6 * i + k];
    float da[3] = {0.0f, 0.0f, 0.0f}, dsc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // xyz = anchor + offsets * scaling[:3]
    for (int j = 0; j < K; ++j) {
        const int64_t g = i * K + j;
        const uint32_t p = a.pos[g];
        const bool kp = a.pos[g + 1] != p;
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        if (kp) {
            const float gx = a.g_xyz[3 * p], gy = a.g_xyz[3 * p + 1], gz = a.g_xyz[3 * p + 2];
            const float *of = a.offsets + 3 * g;
            d0 = gx * sc[0]; d1 = gy * sc[1]; d2 = gz * sc[2];
            dsc[0] = __builtin_fmaf(gx, of[0], dsc[0]); dsc[1] = __builtin_fmaf(gy, of[1], dsc[1]); dsc[2] = __builtin_fmaf(gz, of[2], dsc[2]);
            da[0] += gx; da[1] += gy; da[2] += gz;
        }
        a.d_offsets[3 * g] = d0; a.d_offsets[3 * g + 1] = d1; a.d_offsets[3 * g + 2] = d2;
    }
    float dx[DIN];
#pragma unroll
    for (int k = 0; k < DIN; ++k) dx[k] = 0.0f;
    float h[F], dh[F];
    // opacity head: HAC  neural_opacity = tanh(z) * mask, opacity = the kept neural_opacity
    //               HAC++ neural_opacity = tanh(z),    opacity = the kept tanh(z) * mask
    hidden_layer<F, DIN>(x, a.opacity, h);
#pragma unroll
    for (int c = 0; c < F; ++c) dh[c] = 0.0f;
    for (int j = 0; j < K; ++j) {
        const int64_t g = i * K + j;
        const uint32_t p = a.pos[g];
        const bool kp = a.pos[g + 1] != p;
        const float t = tanhf(out_unit<F>(h, a.opacity, j)), m = a.mask[g];
        const float gop = kp ? a.g_opacity[p] : 0.0f, gno = a.g_nopa[g];
        float dz, dm;
        if (a.mafter) { dz = (gno + gop * m) * (1.0f - t * t); dm = gop * t; }
        else { const float dn = gno + gop; dz = dn * m * (1.0f - t * t); dm = dn * t; }
        a.d_mask[g] = dm;
        a.dZop[j * a.np + i] = dz;
        ngb_acc_dh<F>(a.opacity, j, dz, dh);
    }
    ngb_dx<F, DIN>(a.opacity, dh, h, dx);
    ngb_store_h<F>(a, i, h, dh, a.Hop, a.dHop);
    // colour head: sigmoid
    hidden_layer<F, DIN>(x, a.color, h);
#pragma unroll
    for (int c = 0; c < F; ++c) dh[c] = 0.0f;
    for (int j = 0; j < 3 * K; ++j) {
        const int64_t g = i * K + j / 3;
        const uint32_t p = a.pos[g];
        float dz = 0.0f;
        if (a.pos[g + 1] != p) {
            const float s = 1.0f / (1.0f + expf(-out_unit<F>(h, a.color, j)));
            dz = a.g_color[3 * p + j % 3] * s * (1.0f - s);
        }
        a.dZcol[j * a.np + i] = dz;
        ngb_acc_dh<F>(a.color, j, dz, dh);
    }
    ngb_dx<F, DIN>(a.color, dh, h, dx);
    ngb_store_h<F>(a, i, h, dh, a.Hcol, a.dHcol);
    // covariance head: scaling = scaling[3:] * sigmoid(z[:3]) (* mask, HAC++), rot = z[3:7] / max(|z[3:7]|, 1e-12)
    hidden_layer<F, DIN>(x, a.cov, h);
#pragma unroll
    for (int c = 0; c < F; ++c) dh[c] = 0.0f;
    for (int j = 0; j < K; ++j) {
        const int64_t g = i * K + j;
        const uint32_t p = a.pos[g];
        float dz[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (a.pos[g + 1] != p) {
            float z[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) z[q] = out_unit<F>(h, a.cov, 7 * j + q);
            const float mk = a.mafter ? a.mask[g] : 1.0f;
            float dmk = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float s = 1.0f / (1.0f + expf(-z[k])), gs = a.g_scale[3 * p + k];
                dz[k] = gs * sc[3 + k] * mk * s * (1.0f - s);
                dsc[3 + k] = __builtin_fmaf(gs * s, mk, dsc[3 + k]);
                dmk = __builtin_fmaf(gs * sc[3 + k], s, dmk);
            }
            if (a.mafter) a.d_mask[g] += dmk;
            const float q0 = z[3], q1 = z[4], q2 = z[5], q3 = z[6];
            const float nrm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
            const float r0 = a.g_rot[4 * p], r1 = a.g_rot[4 * p + 1], r2 = a.g_rot[4 * p + 2], r3 = a.g_rot[4 * p + 3];
            if (nrm >= 1e-12f) {   // d(q / |q|) = (g - r (r . g)) / |q|
                const float u0 = q0 / nrm, u1 = q1 / nrm, u2 = q2 / nrm, u3 = q3 / nrm;
                const float rg = u0 * r0 + u1 * r1 + u2 * r2 + u3 * r3;
                dz[3] = (r0 - u0 * rg) / nrm; dz[4] = (r1 - u1 * rg) / nrm; dz[5] = (r2 - u2 * rg) / nrm; dz[6] = (r3 - u3 * rg) / nrm;
            } else {               // the denominator is the clamp's eps: a constant
                dz[3] = r0 / 1e-12f; dz[4] = r1 / 1e-12f; dz[5] = r2 / 1e-12f; dz[6] = r3 / 1e-12f;
            }
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            a.dZcov[(7 * j + q) * a.np + i] = dz[q];
            ngb_acc_dh<F>(a.cov, 7 * j + q, dz[q], dh);
        }
    }
    ngb_dx<F, DIN>(a.cov, dh, h, dx);
    ngb_store_h<F>(a, i, h, dh, a.Hcov, a.dHcov);
    // dx -> feat (through the bank) and view / dist
    float dview[4] = {dx[F], dx[F + 1], dx[F + 2], dx[F + 3]};
    if (bank) {
        float fr[F], df[F];
#pragma unroll
        for (int k = 0; k < F; ++k) { fr[k] = a.feat[i * F + k]; df[k] = 0.0f; }
        float dw0 = 0.0f, dw1 = 0.0f, dw2 = 0.0f;
#pragma unroll
        for (int k = 0; k < F; ++k) {
            const int k0 = (k % (F / 4)) * 4, k1 = (k % (F / 2)) * 2;
            dw0 = __builtin_fmaf(dx[k], fr[k0], dw0); dw1 = __builtin_fmaf(dx[k], fr[k1], dw1); dw2 = __builtin_fmaf(dx[k], fr[k], dw2);
            df[k0] = __builtin_fmaf(dx[k], bw[0], df[k0]); df[k1] = __builtin_fmaf(dx[k], bw[1], df[k1]); df[k] = __builtin_fmaf(dx[k], bw[2], df[k]);
        }
#pragma unroll
        for (int k = 0; k < F; ++k) a.d_feat[i * F + k] = df[k];
        // softmax: dz_s = w_s (dw_s - sum_t w_t dw_t)
        const float sdw = bw[0] * dw0 + bw[1] * dw1 + bw[2] * dw2;
        const float dzb[3] = {bw[0] * (dw0 - sdw), bw[1] * (dw1 - sdw), bw[2] * (dw2 - sdw)};
        const float cv[4] = {x[F], x[F + 1], x[F + 2], x[F + 3]};
        hidden_layer<F, 4>(cv, a.bank, h);
#pragma unroll
        for (int c = 0; c < F; ++c) dh[c] = 0.0f;
#pragma unroll
        for (int s = 0; s < 3; ++s) { a.dZb[s * a.np + i] = dzb[s]; ngb_acc_dh<F>(a.bank, s, dzb[s], dh); }
        ngb_dx<F, 4>(a.bank, dh, h, dview);
        ngb_store_h<F>(a, i, h, dh, a.Hb, a.dHb);
#pragma unroll
        for (int k = 0; k < 4; ++k) a.Xb[k * a.np + i] = cv[k];
        a.Xb[4 * a.np + i] = 1.0f;
    } else {
#pragma unroll
        for (int k = 0; k < F; ++k) a.d_feat[i * F + k] = dx[k];
    }
    // view = v / |v|, dist = |v|, v = anchor - cam:  dv = (dview - view (view . dview)) / dist + ddist view
    const float ux = x[F], uy = x[F + 1], uz = x[F + 2];
    const float ud = ux * dview[0] + uy * dview[1] + uz * dview[2];
    da[0] += (dview[0] - ux * ud) / dist + dview[3] * ux;
    da[1] += (dview[1] - uy * ud) / dist + dview[3] * uy;
    da[2] += (dview[2] - uz * ud) / dist + dview[3] * uz;
    a.d_anchor[3 * i] = da[0]; a.d_anchor[3 * i + 1] = da[1]; a.d_anchor[3 * i + 2] = da[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) a.d_scaling[6 * i + k] = dsc[k];
}

// one 64-row output strip of a weight gradient: dW[m][c] = sum_r A[m][r] B[c][r] for m0 <= m < min(m0 + 64, M), c < N (the last column of B
// is ones: c == N - 1 is the bias); dW[m][c] goes to w[m * (N - 1) + c], the bias to b[m]
struct NGStrip { const float *A, *B; float *w, *b; int M, N, m0; };
constexpr int NG_MAX_STRIPS = 16;
struct NGWArgs { NGStrip s[NG_MAX_STRIPS]; int64_t np, chunk; int ranges; float *partial; };

__global__ __launch_bounds__(64) void k_ngb_wgrad(NGWArgs a)
{
    const NGStrip s = a.s[blockIdx.y];
    const int lane = threadIdx.x, e = lane & 15, g = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk, r1 = min(a.np, r0 + a.chunk);
    const int nmt = min(4, (s.M - s.m0 + 15) / 16), nnt = (s.N + 15) / 16;
    f32x4n acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4n{0.0f, 0.0f, 0.0f, 0.0f};
    // lane (g, e) supplies anchors r + 4 g .. r + 4 g + 3 (one float4 per operand tile) at the four k-steps: A row m0 + 16 mt + e, B column 16 nt + e
    for (int64_t r = r0; r < r1; r += 16) {
        f32x4n av[4], bv[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = s.m0 + 16 * mt + e;
            av[mt] = mt < nmt && m < s.M ? *reinterpret_cast<const f32x4n *>(s.A + m * a.np + r + 4 * g) : f32x4n{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int c = 16 * nt + e;
            bv[nt] = nt < nnt && c < s.N ? *reinterpret_cast<const f32x4n *>(s.B + c * a.np + r + 4 * g) : f32x4n{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                if (mt < nmt) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        if (nt < nnt) NG_MF(acc[mt][nt], av[mt][kk], bv[nt][kk]);
                }
    }
    float *out = a.partial + ((int64_t)blockIdx.y * a.ranges + blockIdx.x) * 4096;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[(16 * mt + 4 * g + i) * 64 + 16 * nt + e] = acc[mt][nt][i];
}

__global__ __launch_bounds__(256) void k_ngb_wsum(NGWArgs a)
{
    const NGStrip s = a.s[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x, m = s.m0 + idx / 64, c = idx % 64;
    if (m >= s.M || m >= s.m0 + 64 || c >= s.N) return;
    const float *p = a.partial + (int64_t)blockIdx.y * a.ranges * 4096 + idx;
    double sum = 0.0;
    for (int r = 0; r < a.ranges; ++r) sum += (double)p[(int64_t)r * 4096];
    const float v = (float)sum;
    if (c < s.N - 1) s.w[(int64_t)m * (s.N - 1) + c] = v;
    else s.b[m] = v;
}

__global__ void k_ngb_zero(float *p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}

}  // namespace

extern "C" int gsnn_forward_train(gpcc_ctx *ctx, int64_t n, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
                                  const float *scaling, const float *mask, const float *cam_center, const float *const *mlp, int mask_after_opacity,
                                  float *xyz_out, float *color_out, float *opacity_out, float *scale_out, float *rot_out, float *nopa_out, uint8_t *keep_out,
                                  gsr_alloc_fn alloc, void *alloc_user, uint32_t **pos_out, int64_t *count_out, void *stream)
{
    if (!ctx || !mlp || !alloc || !pos_out || !count_out) return fail(GPCC_ERR_ARG, "null argument");
    *count_out = 0;
    *pos_out = nullptr;
    GP_TRY(ng_check("neural_gaussians_train", n, feat_dim, n_offsets, mlp));
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t *pos;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)(n * n_offsets + 1) * 4, &pos, "gsnn_forward_train"));
    *pos_out = pos;
    if (n == 0) { HIP_TRY(hipMemsetAsync(pos, 0, 4, st)); return GPCC_OK; }
    if (!anchor || !feat || !offsets || !scaling || !mask || !cam_center || !xyz_out || !color_out || !opacity_out || !scale_out || !rot_out || !nopa_out ||
        !keep_out)
        return fail(GPCC_ERR_ARG, "null argument");
    return ng_forward(ctx, NGMode{true, nullptr, pos, nopa_out, mask_after_opacity != 0, keep_out}, n, feat_dim, n_offsets, anchor, feat, offsets, scaling, mask,
                      cam_center, mlp, xyz_out, color_out, opacity_out, scale_out, rot_out, count_out, st);
}

extern "C" int gsnn_backward(gpcc_ctx *ctx, int64_t n, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
                             const float *scaling, const float *mask, const float *cam_center, const float *const *mlp, int mask_after_opacity,
                             const uint32_t *pos, const float *g_xyz, const float *g_color, const float *g_opacity, const float *g_scale, const float *g_rot,
                             const float *g_nopa, float *d_anchor, float *d_feat, float *d_offsets, float *d_scaling, float *d_mask, float *const *d_mlp,
                             gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx || !mlp || !d_mlp || !alloc) return fail(GPCC_ERR_ARG, "null argument");
    GP_TRY(ng_check("neural_gaussians_train", n, feat_dim, n_offsets, mlp));
    const bool bank = mlp[0] != nullptr;
    for (int q = bank ? 0 : 4; q < 16; ++q)
        if (!d_mlp[q]) return fail(GPCC_ERR_ARG, "null MLP gradient %d", q);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int F = feat_dim, K = n_offsets;
    if (n == 0) {   // no anchors: zero weight gradients
        const int64_t sz[16] = {(int64_t)F * 4, F, 3 * (int64_t)F, 3, (int64_t)F * (F + 4), F, (int64_t)K * F, K, (int64_t)F * (F + 4), F, 7 * (int64_t)K * F, 7 * K,
                                (int64_t)F * (F + 4), F, 3 * (int64_t)K * F, 3 * K};
        for (int q = bank ? 0 : 4; q < 16; ++q) {
            k_ngb_zero<<<(unsigned)cdiv(sz[q], 256), 256, 0, st>>>(d_mlp[q], sz[q]);
            LAUNCH_CHECK();
        }
        return GPCC_OK;
    }
    if (!anchor || !feat || !offsets || !scaling || !mask || !cam_center || !pos || !g_nopa || !d_anchor || !d_feat || !d_offsets || !d_scaling || !d_mask)
        return fail(GPCC_ERR_ARG, "null argument");
    const int64_t np = (n + 15) / 16 * 16;
    const int ncol = (F + 5) + 3 * (F + 1) + 3 * F + 11 * K + (bank ? 5 + (F + 1) + F + 3 : 0);
    // anchor ranges of the weight-gradient pass: a function of n only.  A range's float32 accumulator runs over few anchors (64 up to 16384
    // anchors, n / 256 beyond: the partials are 64 KB per range and strip) and k_ngb_wsum adds the partials in double: with 2048 anchors per
    // range a bias gradient over 2400 anchors was 5 float32 ulp off, where torch's tree sum stays within 1.
    const int ranges = (int)std::min<int64_t>(256, cdiv(np, 64));
    const int64_t chunk = cdiv(cdiv(np, ranges), 16) * 16;
    NGWArgs w = {};
    w.np = np; w.chunk = chunk; w.ranges = ranges;
    float *ws;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)ncol * np * 4 + (size_t)NG_MAX_STRIPS * ranges * 4096 * 4, &ws, "gsnn_backward"));
    NGBArgs b = {};
    b.anchor = anchor; b.feat = feat; b.offsets = offsets; b.scaling = scaling; b.mask = mask; b.cam = cam_center; b.pos = pos;
    b.n = n; b.np = np; b.K = K; b.mafter = mask_after_opacity != 0;
    ng_mlps(mlp, &b.bank, &b.opacity, &b.cov, &b.color);
    b.g_xyz = g_xyz; b.g_color = g_color; b.g_opacity = g_opacity; b.g_scale = g_scale; b.g_rot = g_rot; b.g_nopa = g_nopa;
    b.d_anchor = d_anchor; b.d_feat = d_feat; b.d_offsets = d_offsets; b.d_scaling = d_scaling; b.d_mask = d_mask;
    float *q = ws;
    auto take = [&](int cols) { float *p = q; q += (int64_t)cols * np; return p; };
    b.X = take(F + 5);
    b.Hop = take(F + 1); b.Hcol = take(F + 1); b.Hcov = take(F + 1);
    b.dHop = take(F); b.dHcol = take(F); b.dHcov = take(F);
    b.dZop = take(K); b.dZcol = take(3 * K); b.dZcov = take(7 * K);
    if (bank) { b.Xb = take(5); b.Hb = take(F + 1); b.dHb = take(F); b.dZb = take(3); }
    w.partial = q;
    if (F == 32) k_ngb_anchor<32><<<(unsigned)cdiv(np, TB), TB, 0, st>>>(b);
    else k_ngb_anchor<50><<<(unsigned)cdiv(np, TB), TB, 0, st>>>(b);
    LAUNCH_CHECK();
    // the strips: {A, B, w, b, M, N}; every M here is <= 448, N <= 55
    int ns = 0;
    auto strips = [&](const float *A, const float *B, float *wt, float *bs, int M, int N) {
        for (int m0 = 0; m0 < M; m0 += 64) w.s[ns++] = NGStrip{A, B, wt, bs, M, N, m0};
    };
    // mlp / d_mlp order: bank, opacity, cov, colour; {w1, b1, w2, b2} each
    strips(b.dHop, b.X, d_mlp[4], d_mlp[5], F, F + 5);
    strips(b.dZop, b.Hop, d_mlp[6], d_mlp[7], K, F + 1);
    strips(b.dHcov, b.X, d_mlp[8], d_mlp[9], F, F + 5);
    strips(b.dZcov, b.Hcov, d_mlp[10], d_mlp[11], 7 * K, F + 1);
    strips(b.dHcol, b.X, d_mlp[12], d_mlp[13], F, F + 5);
    strips(b.dZcol, b.Hcol, d_mlp[14], d_mlp[15], 3 * K, F + 1);
    if (bank) {
        strips(b.dHb, b.Xb, d_mlp[0], d_mlp[1], F, 5);
        strips(b.dZb, b.Hb, d_mlp[2], d_mlp[3], 3, F + 1);
    }
    k_ngb_wgrad<<<dim3((unsigned)ranges, (unsigned)ns), 64, 0, st>>>(w);
    LAUNCH_CHECK();
    k_ngb_wsum<<<dim3(16, (unsigned)ns), 256, 0, st>>>(w);
    LAUNCH_CHECK();
    return GPCC_OK;
}
