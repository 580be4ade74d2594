// mlp2_train.hip -- backward of the two-layer context MLPs (mlp2.hip): gshac_mlp2_backward.
// The training forward is gshac_mlp2_act itself, so nothing is saved: the backward recomputes the hidden pre-activation
// h = b1 + x W1^T with the forward's chain (bias, then fmaf over k ascending; the same class, hence the same padding steps), and the
// activation mask is the forward's bit for bit.  Then
//   g = (dy W2) o act'(h)    dx = g W1    dW2 = dy^T act(h)    db2 = sum dy    dW1 = g^T x    db1 = sum g
// Weight and bias gradients in a fixed order: the rows are cut into slabs whose size depends on n and the kernel class alone
// (gshac_mlp2_slab_rows), one workgroup walks its slab 16 rows at a time and writes ONE partial of every parameter gradient, and
// k_mlp2_bwd_reduce adds the partials in slab order.  No atomics: the result has the same bits run to run, on any stream, on any device.
// k_mlp2_bwd_plain states the arithmetic one element per thread; k_mlp2_bwd_mfma runs the three classes of the forward on the matrix pipe.
#include "common.hpp"

using namespace gpcc;

namespace {
constexpr int TB = 256, WAVES = TB / 64, ROWS = 16;
constexpr int TB_PLAIN = 1024;                        // k_mlp2_bwd_plain: a full workgroup, its loops have no other way to hide their loads
constexpr size_t LDS_MAX = 160 * 1024;
constexpr int SLABS_MFMA = 512, SLABS_PLAIN = 256;   // slabs a large n is cut into (two rounds of workgroups over 256 CUs / one)
constexpr int SLAB_TILES_MIN = 8;                    // a workgroup's set-up (both weight matrices into LDS) is shared by at least 128 rows

__device__ __forceinline__ float act_value(float h, float slope) { return h > 0.0f ? h : (slope != 0.0f ? h * slope : 0.0f); }
// torch's threshold_backward / leaky_relu_backward: the upstream value where h > 0, else 0 (ReLU) or slope times it
__device__ __forceinline__ float act_grad(float h, float d, float slope) { return h > 0.0f ? d : (slope != 0.0f ? d * slope : 0.0f); }

// The bias gradients are plain column sums over all rows, where a float32 running sum loses more than the products' chains do: they are
// compensated sums (Kahan: `comp` carries what the last addition rounded away), still one fixed order.  -ffp-contract=off, no fast-math.
__device__ __forceinline__ void add_compensated(float &sum, float &comp, float v)
{
    const float y = v - comp, t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

// Layout of one slab's partial (and of nothing else): dW1 (dh, din), db1 (dh), dW2 (dout, dh), db2 (dout): `params` words that k_mlp2_bwd_reduce adds;
// behind them the compensation terms of db1 and db2, which k_mlp2_bwd_plain carries from tile to tile there (k_mlp2_bwd_mfma has them in registers)
struct Part {
    int64_t w1, b1, w2, b2, params, c1, c2, total;
    __host__ __device__ Part(int din, int dh, int dout)
        : w1(0), b1((int64_t)dh * din), w2(b1 + dh), b2(w2 + (int64_t)dout * dh), params(b2 + dout), c1(params), c2(c1 + dh), total(c2 + dout) {}
};

// ------------------------------------------------------------------ the readable statement: any size the forward takes
// LDS: the tile's rows, their hidden pre-activations (later the activations) and g.  The slab's partial lives in the workspace and is
// updated tile by tile by the thread that owns the element (16-term fmaf chain over the tile's rows, rows ascending).
__global__ __launch_bounds__(TB_PLAIN) void k_mlp2_bwd_plain(const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1,
                                                       const float *__restrict__ w2, int64_t n, int din, int dh, int dout, float slope,
                                                       const float *__restrict__ dy, float *__restrict__ dx, int64_t slab_rows, float *__restrict__ parts)
{
    extern __shared__ float sm[];
    float *xs = sm, *hs = xs + ROWS * din, *gs = hs + ROWS * dh;
    const Part P(din, dh, dout);
    float *part = parts + (int64_t)blockIdx.x * P.total;
    const int64_t begin = (int64_t)blockIdx.x * slab_rows, end = min(n, begin + slab_rows);
    for (int64_t row0 = begin; row0 < end; row0 += ROWS) {
        const int rows = (int)min((int64_t)ROWS, end - row0);
        const bool first = row0 == begin;
        const float *dyt = dy + row0 * dout;
        for (int i = threadIdx.x; i < rows * din; i += TB_PLAIN) xs[i] = x[row0 * din + i];
        __syncthreads();
        for (int i = threadIdx.x; i < rows * dh; i += TB_PLAIN) {          // h, the forward's chain
            const int r = i / dh, c = i - r * dh;
            const float *w = w1 + (size_t)c * din, *xr = xs + r * din;
            float acc = b1[c];
            for (int k = 0; k < din; ++k) acc = __builtin_fmaf(xr[k], w[k], acc);
            hs[i] = acc;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < rows * dh; i += TB_PLAIN) {          // g = (dy W2) o act'(h); hs becomes act(h)
            const int r = i / dh, c = i - r * dh;
            float d = 0.0f;
            for (int o = 0; o < dout; ++o) d = __builtin_fmaf(dyt[r * dout + o], w2[(size_t)o * dh + c], d);
            const float h = hs[i];
            gs[i] = act_grad(h, d, slope);
            hs[i] = act_value(h, slope);
        }
        __syncthreads();
        if (dx)
            for (int i = threadIdx.x; i < rows * din; i += TB_PLAIN) {
                const int r = i / din, k = i - r * din;
                float acc = 0.0f;
                for (int c = 0; c < dh; ++c) acc = __builtin_fmaf(gs[r * dh + c], w1[(size_t)c * din + k], acc);
                dx[row0 * din + i] = acc;
            }
        for (int i = threadIdx.x; i < dh * din; i += TB_PLAIN) {           // dW1 += g^T x
            const int c = i / din, k = i - c * din;
            float acc = first ? 0.0f : part[P.w1 + i];
            for (int r = 0; r < rows; ++r) acc = __builtin_fmaf(gs[r * dh + c], xs[r * din + k], acc);
            part[P.w1 + i] = acc;
        }
        for (int c = threadIdx.x; c < dh; c += TB_PLAIN) {                 // db1 += sum g
            float acc = first ? 0.0f : part[P.b1 + c], comp = first ? 0.0f : part[P.c1 + c];
            for (int r = 0; r < rows; ++r) add_compensated(acc, comp, gs[r * dh + c]);
            part[P.b1 + c] = acc;
            part[P.c1 + c] = comp;
        }
        for (int i = threadIdx.x; i < dout * dh; i += TB_PLAIN) {          // dW2 += dy^T act(h)
            const int o = i / dh, c = i - o * dh;
            float acc = first ? 0.0f : part[P.w2 + i];
            for (int r = 0; r < rows; ++r) acc = __builtin_fmaf(dyt[r * dout + o], hs[r * dh + c], acc);
            part[P.w2 + i] = acc;
        }
        for (int o = threadIdx.x; o < dout; o += TB_PLAIN) {               // db2 += sum dy
            float acc = first ? 0.0f : part[P.b2 + o], comp = first ? 0.0f : part[P.c2 + o];
            for (int r = 0; r < rows; ++r) add_compensated(acc, comp, dyt[r * dout + o]);
            part[P.b2 + o] = acc;
            part[P.c2 + o] = comp;
        }
        __syncthreads();
    }
}

// The partials of all slabs, added in slab order (a compensated sum): one thread per parameter.
__global__ __launch_bounds__(TB) void k_mlp2_bwd_reduce(const float *__restrict__ parts, int64_t nslabs, int din, int dh, int dout,
                                                        float *__restrict__ dw1, float *__restrict__ db1, float *__restrict__ dw2, float *__restrict__ db2)
{
    const Part P(din, dh, dout);
    const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= P.params) return;
    float acc = parts[p], comp = 0.0f;
    for (int64_t s = 1; s < nslabs; ++s) add_compensated(acc, comp, parts[s * P.total + p]);
    if (p < P.b1) dw1[p] = acc;
    else if (p < P.w2) db1[p - P.b1] = acc;
    else if (p < P.b2) dw2[p - P.w2] = acc;
    else db2[p - P.b2] = acc;
}

// ------------------------------------------------------------------ the matrix pipe: the three classes of k_mlp2_mfma
// v_mfma_f32_16x16x4_f32: lane (g = lane / 16, e = lane % 16) supplies A[row e][k g] and B[k g][column e] and holds D[rows 4 g .. 4 g + 3][column e];
// every element of D is its own k-ascending fmaf chain on the accumulator (tools/ubench/mfma_order.hip).
// One workgroup of four waves per slab: both weight matrices and b1 in LDS (zero-padded to the class), then per 16-row tile
//   phase 1  wave w takes the hidden-unit tiles t = w, w + 4, ..: h (x W1^T on the bias), dy W2, and from both act(h) and g, into LDS
//   phase 2  dx tiles t = w, w + 4, ..; dW2 output-row tiles w, w + 4, .. and dW1 input-column tiles 3 - w, 7 - w, .. (the two lists
//            run against each other so that no wave gets the long end of both), accumulated in registers across the slab's tiles
//            (a tile is four more k-steps of every chain: rows ascending); threads 0 .. sum the tile's columns of g and dy for db1 / db2
// The tile after this one is loaded into registers while the phases run.
// LDS pitches: tiles read as [row 4 kk + g][column 16 t + e] (most reads) have a pitch of 8 mod 32 words: the four row groups of a wave
// land on different banks; W1, read both ways, has DIN + 4.
typedef float f32x4m __attribute__((ext_vector_type(4)));
constexpr int pitch8(int w) { return (w + 23) / 32 * 32 + 8; }

template <int DIN, int DH, int DOUT> struct Cls {
    static_assert(DIN % 16 == 0 && DH % 4 == 0, "whole dx tiles and MFMA k-steps");
    static constexpr int NT1 = (DH + 15) / 16, NT2 = (DOUT + 15) / 16, NTK = DIN / 16, DOUT4 = (DOUT + 3) / 4 * 4;
    static constexpr int P1 = DIN + 4, P2 = pitch8(DH), PX = pitch8(DIN), PD = pitch8(16 * NT2), PA = pitch8(16 * NT1);
    // W1 has whole tiles of rows (zeros); the B operands of W2's padding columns (hidden units >= DH of the last tile) run into the next row and,
    // from the last row, into b1: initialised words, and they only reach accumulator columns that are replaced by zeros
    static constexpr int W1_WORDS = 16 * NT1 * P1, W2_WORDS = DOUT4 * P2, B1_WORDS = 16 * NT1;
    static constexpr int LDS_WORDS = W1_WORDS + W2_WORDS + B1_WORDS + ROWS * (PX + PD + 2 * PA);
    static_assert(16 * NT1 - DH <= B1_WORDS, "W2's padding columns stay inside b1");
    static_assert(16 * NT2 <= TB && 16 * NT1 <= TB, "one thread per bias gradient");
    static_assert((size_t)LDS_WORDS * 4 <= LDS_MAX, "at most 160 KB of LDS");
    static constexpr int M2 = (NT2 + WAVES - 1) / WAVES, M1 = (NTK + WAVES - 1) / WAVES;   // dW2 row tiles / dW1 column tiles per wave
    static constexpr int NX = ROWS * DIN / TB, ND = ROWS * 16 * NT2 / TB;                   // words of a tile per thread
};

template <int DIN, int DH, int DOUT>
__global__ __launch_bounds__(TB) void k_mlp2_bwd_mfma(const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1,
                                                      const float *__restrict__ w2, int64_t n, int din, int dh, int dout, float slope,
                                                      const float *__restrict__ dy, float *__restrict__ dx, int64_t slab_rows, float *__restrict__ parts)
{
    using C = Cls<DIN, DH, DOUT>;
    constexpr int NT1 = C::NT1, NT2 = C::NT2, NTK = C::NTK, DOUT4 = C::DOUT4, P1 = C::P1, P2 = C::P2, PX = C::PX, PD = C::PD, PA = C::PA;
    constexpr int DOUTP = 16 * NT2;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *W1s = sm, *W2s = W1s + C::W1_WORDS, *B1s = W2s + C::W2_WORDS, *xs = B1s + C::B1_WORDS, *dys = xs + ROWS * PX, *as = dys + ROWS * PD, *gs = as + ROWS * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), e = lane & 15, g = lane >> 4;   // wave: scalar, so its branches are
    const int64_t begin = (int64_t)blockIdx.x * slab_rows, end = min(n, begin + slab_rows);

    float nx[C::NX], nd[C::ND];            // the next tile: rows past the end and columns past din / dout are zeros
    auto fetch = [&](int64_t row0) {
#pragma unroll
        for (int u = 0; u < C::NX; ++u) { const int i = tid + u * TB, r = i / DIN, c = i - r * DIN; nx[u] = (row0 + r < end && c < din) ? x[(row0 + r) * din + c] : 0.0f; }
#pragma unroll
        for (int u = 0; u < C::ND; ++u) { const int i = tid + u * TB, r = i / DOUTP, c = i - r * DOUTP; nd[u] = (row0 + r < end && c < dout) ? dy[(row0 + r) * dout + c] : 0.0f; }
    };
    fetch(begin);
    for (int i = tid; i < C::W1_WORDS; i += TB) { const int c = i / P1, k = i - c * P1; W1s[i] = (c < dh && k < din) ? w1[(size_t)c * din + k] : 0.0f; }
    for (int i = tid; i < C::W2_WORDS; i += TB) { const int o = i / P2, c = i - o * P2; W2s[i] = (o < dout && c < dh) ? w2[(size_t)o * dh + c] : 0.0f; }
    for (int i = tid; i < C::B1_WORDS; i += TB) B1s[i] = i < dh ? b1[i] : 0.0f;

    f32x4m acc2[C::M2][NT1], acc1[C::M1][NT1];   // dW2 tiles (rows 16 (wave + 4 m), hidden tile tc), dW1 tiles (hidden tile tc, columns 16 (3 - wave + 4 m))
#pragma unroll
    for (int m = 0; m < C::M2; ++m)
#pragma unroll
        for (int tc = 0; tc < NT1; ++tc) acc2[m][tc] = f32x4m{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int m = 0; m < C::M1; ++m)
#pragma unroll
        for (int tc = 0; tc < NT1; ++tc) acc1[m][tc] = f32x4m{0.0f, 0.0f, 0.0f, 0.0f};
    float sum_b1 = 0.0f, sum_b2 = 0.0f, comp_b1 = 0.0f, comp_b2 = 0.0f;

    for (int64_t row0 = begin; row0 < end; row0 += ROWS) {
#pragma unroll
        for (int u = 0; u < C::NX; ++u) { const int i = tid + u * TB, r = i / DIN, c = i - r * DIN; xs[r * PX + c] = nx[u]; }
#pragma unroll
        for (int u = 0; u < C::ND; ++u) { const int i = tid + u * TB, r = i / DOUTP, c = i - r * DOUTP; dys[r * PD + c] = nd[u]; }
        __syncthreads();
        if (row0 + ROWS < end) fetch(row0 + ROWS);

        // ---- phase 1: act(h) and g of the wave's hidden-unit tiles
        if (wave < NT1) {
            float ax[DIN / 4], ad[DOUT4 / 4];
#pragma unroll
            for (int kk = 0; kk < DIN / 4; ++kk) ax[kk] = xs[e * PX + 4 * kk + g];
#pragma unroll
            for (int kk = 0; kk < DOUT4 / 4; ++kk) ad[kk] = dys[e * PD + 4 * kk + g];
#pragma unroll
            for (int m = 0; m < (NT1 + WAVES - 1) / WAVES; ++m) {
                const int t = wave + WAVES * m;
                if (t < NT1) {
                    __builtin_amdgcn_sched_barrier(0);
                    const int c = 16 * t + e;
                    const float bias = B1s[c];
                    f32x4m h = {bias, bias, bias, bias}, d = {0.0f, 0.0f, 0.0f, 0.0f};
                    {
                        float wb[DIN / 4];
                        const float *wr = W1s + c * P1 + g;
#pragma unroll
                        for (int kk = 0; kk < DIN / 4; ++kk) wb[kk] = wr[4 * kk];
#pragma unroll
                        for (int kk = 0; kk < DIN / 4; ++kk) h = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[kk], wb[kk], h, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    {
                        float wb[DOUT4 / 4];
                        const float *wr = W2s + g * P2 + c;
#pragma unroll
                        for (int kk = 0; kk < DOUT4 / 4; ++kk) wb[kk] = wr[4 * kk * P2];
#pragma unroll
                        for (int kk = 0; kk < DOUT4 / 4; ++kk) d = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[kk], wb[kk], d, 0, 0, 0);
                    }
                    const bool real = c < dh;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        as[(4 * g + i) * PA + c] = real ? act_value(h[i], slope) : 0.0f;
                        gs[(4 * g + i) * PA + c] = real ? act_grad(h[i], d[i], slope) : 0.0f;
                    }
                }
            }
        }
        __syncthreads();

        // ---- phase 2
        if (tid < 16 * NT1) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) add_compensated(sum_b1, comp_b1, gs[r * PA + tid]);
        }
        if (tid < 16 * NT2) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) add_compensated(sum_b2, comp_b2, dys[r * PD + tid]);
        }
        if (dx && wave < NTK) {                                  // dx = g W1
            float ag[DH / 4];
#pragma unroll
            for (int kk = 0; kk < DH / 4; ++kk) ag[kk] = gs[e * PA + 4 * kk + g];
#pragma unroll
            for (int m = 0; m < C::M1; ++m) {
                const int t = wave + WAVES * m;
                if (t < NTK) {
                    float wb[DH / 4];
                    const float *wr = W1s + g * P1 + 16 * t + e;
#pragma unroll
                    for (int kk = 0; kk < DH / 4; ++kk) wb[kk] = wr[4 * kk * P1];
                    f32x4m acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int kk = 0; kk < DH / 4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[kk], wb[kk], acc, 0, 0, 0);
                    const int k = 16 * t + e;
                    if (k < din) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (row0 + 4 * g + i < end) dx[(row0 + 4 * g + i) * din + k] = acc[i];
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            // operands over the tile's rows (k = row 4 kk + g): act(h) as B of dW2, g as A of dW1, for every hidden tile
            float ba[NT1][4], ag[NT1][4];
#pragma unroll
            for (int tc = 0; tc < NT1; ++tc)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    ba[tc][kk] = as[(4 * kk + g) * PA + 16 * tc + e];
                    ag[tc][kk] = gs[(4 * kk + g) * PA + 16 * tc + e];
                }
#pragma unroll
            for (int m = 0; m < C::M2; ++m) {                    // dW2[o][c] += sum_r dy[r][o] act(h)[r][c]
                const int to = wave + WAVES * m;
                if (to < NT2) {
                    float a[4];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) a[kk] = dys[(4 * kk + g) * PD + 16 * to + e];
#pragma unroll
                    for (int tc = 0; tc < NT1; ++tc)
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) acc2[m][tc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], ba[tc][kk], acc2[m][tc], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < C::M1; ++m) {                    // dW1[c][k] += sum_r g[r][c] x[r][k]
                const int tk = WAVES - 1 - wave + WAVES * m;
                if (tk < NTK) {
                    float b[4];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) b[kk] = xs[(4 * kk + g) * PX + 16 * tk + e];
#pragma unroll
                    for (int tc = 0; tc < NT1; ++tc)
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) acc1[m][tc] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[tc][kk], b[kk], acc1[m][tc], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- the slab's partial
    const Part P(din, dh, dout);
    float *part = parts + (int64_t)blockIdx.x * P.total;
#pragma unroll
    for (int m = 0; m < C::M2; ++m) {
        const int to = wave + WAVES * m;
        if (to < NT2) {
#pragma unroll
            for (int tc = 0; tc < NT1; ++tc) {
                const int c = 16 * tc + e;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int o = 16 * to + 4 * g + i;
                    if (o < dout && c < dh) part[P.w2 + (int64_t)o * dh + c] = acc2[m][tc][i];
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < C::M1; ++m) {
        const int tk = WAVES - 1 - wave + WAVES * m;
        if (tk < NTK) {
            const int k = 16 * tk + e;
#pragma unroll
            for (int tc = 0; tc < NT1; ++tc)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = 16 * tc + 4 * g + i;
                    if (c < dh && k < din) part[P.w1 + (int64_t)c * din + k] = acc1[m][tc][i];
                }
        }
    }
    if (tid < dh) part[P.b1 + tid] = sum_b1;
    if (tid < dout) part[P.b2 + tid] = sum_b2;
}

template <int DIN, int DH, int DOUT>
int mfma_launch(gpcc_ctx *ctx, const float *x, const float *w1, const float *b1, const float *w2, int64_t n, int din, int dh, int dout, float slope,
                const float *dy, float *dx, int64_t slab_rows, int64_t nslabs, float *parts, hipStream_t st)
{
    static PerDeviceOnce attr;
    GP_TRY(attr.run(ctx->device, [&]() -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp2_bwd_mfma<DIN, DH, DOUT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
        return GPCC_OK;
    }));
    k_mlp2_bwd_mfma<DIN, DH, DOUT><<<(unsigned)nslabs, TB, (size_t)Cls<DIN, DH, DOUT>::LDS_WORDS * 4, st>>>(x, w1, b1, w2, n, din, dh, dout, slope, dy, dx,
                                                                                                          slab_rows, parts);
    LAUNCH_CHECK();
    return GPCC_OK;
}

// the class gshac_mlp2_act runs the layer in (the same tests in the same order): 0 = the plain kernel
int mlp2_class(int din, int dh, int dout)
{
    static const bool use_mfma = dev_env_int("GAUSPCC_MLP2_MFMA", 1) != 0;
    if (!use_mfma) return 0;
    if (din == 96 && dh == 100 && dout == 175) return 1;
    if (din <= 192 && dh <= 40 && dout <= 32) return 2;
    if (din <= 48 && dh <= 100 && dout <= 240) return 3;
    return 0;
}

bool sizes_ok(int din, int dh, int dout) { return din > 0 && dh > 0 && dout > 0 && (size_t)ROWS * (size_t)(din + dh) * 4 <= 64 * 1024; }

int64_t slab_rows_of(int64_t n, int cls)
{
    const int64_t tiles = cdiv(n, ROWS);
    return ROWS * std::max<int64_t>(SLAB_TILES_MIN, cdiv(tiles, cls ? SLABS_MFMA : SLABS_PLAIN));
}
}  // namespace

extern "C" int64_t gshac_mlp2_slab_rows(int64_t n, int din, int dh, int dout)
{
    if (n < 0 || !sizes_ok(din, dh, dout)) return 0;
    return slab_rows_of(n, mlp2_class(din, dh, dout));
}

extern "C" int gshac_mlp2_backward(gpcc_ctx *ctx, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, int64_t n, int din,
                                   int dh, int dout, int act, float slope, const float *dy, float *dx, float *dw1, float *db1, float *dw2, float *db2,
                                   gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    (void)b2;   // y's bias does not enter any gradient; the argument keeps the forward's list
    if (!ctx || !w1 || !b1 || !w2 || !dw1 || !db1 || !dw2 || !db2) return fail(GPCC_ERR_ARG, "gshac_mlp2_backward: null argument");
    if (act != 0 && act != 1) return fail(GPCC_ERR_ARG, "gshac_mlp2_backward: activation must be 0 (ReLU) or 1 (LeakyReLU)");
    if (n < 0) return fail(GPCC_ERR_ARG, "gshac_mlp2_backward: n = %lld", (long long)n);
    if (!sizes_ok(din, dh, dout)) return fail(GPCC_ERR_ARG, "gshac_mlp2_backward: unsupported layer sizes %d - %d - %d", din, dh, dout);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const Part P(din, dh, dout);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(dw1, 0, sizeof(float) * (size_t)dh * din, st));
        HIP_TRY(hipMemsetAsync(db1, 0, sizeof(float) * (size_t)dh, st));
        HIP_TRY(hipMemsetAsync(dw2, 0, sizeof(float) * (size_t)dout * dh, st));
        HIP_TRY(hipMemsetAsync(db2, 0, sizeof(float) * (size_t)dout, st));
        return GPCC_OK;
    }
    if (!x || !dy || !alloc) return fail(GPCC_ERR_ARG, "gshac_mlp2_backward: null argument");
    if (n * (int64_t)std::max(din, dout) >= ((int64_t)1 << 40)) return fail(GPCC_ERR_ARG, "gshac_mlp2_backward: n = %lld rows", (long long)n);
    const float sl = act == 1 ? slope : 0.0f;
    const int cls = mlp2_class(din, dh, dout);
    const int64_t slab_rows = slab_rows_of(n, cls), nslabs = cdiv(n, slab_rows);
    float *parts;
    GP_TRY(caller_block(alloc, alloc_user, "gshac_mlp2_backward", [&](Carver &c) { parts = c.take<float>((size_t)(nslabs * P.total)); }));
    if (cls == 1) GP_TRY((mfma_launch<96, 100, 175>(ctx, x, w1, b1, w2, n, din, dh, dout, sl, dy, dx, slab_rows, nslabs, parts, st)));
    else if (cls == 2) GP_TRY((mfma_launch<192, 40, 32>(ctx, x, w1, b1, w2, n, din, dh, dout, sl, dy, dx, slab_rows, nslabs, parts, st)));
    else if (cls == 3) GP_TRY((mfma_launch<48, 100, 240>(ctx, x, w1, b1, w2, n, din, dh, dout, sl, dy, dx, slab_rows, nslabs, parts, st)));
    else {
        static PerDeviceOnce attr;
        GP_TRY(attr.run(ctx->device, [&]() -> int {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp2_bwd_plain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
            return GPCC_OK;
        }));
        // 16 (din + dh) words <= 64 KB (sizes_ok), so with g at most 128 KB
        k_mlp2_bwd_plain<<<(unsigned)nslabs, TB_PLAIN, sizeof(float) * ROWS * (size_t)(din + 2 * dh), st>>>(x, w1, b1, w2, n, din, dh, dout, sl, dy, dx, slab_rows, parts);
        LAUNCH_CHECK();
    }
    k_mlp2_bwd_reduce<<<(unsigned)cdiv(P.params, TB), TB, 0, st>>>(parts, nslabs, din, dh, dout, dw1, db1, dw2, db2);
    LAUNCH_CHECK();
    return GPCC_OK;
}
