// mlp2.hip -- the two-layer context MLPs of HAC / HAC++:
//   gshac_mlp2 / gshac_mlp2_act   mlp_grid and HAC++'s channel-context MLPs: Linear - ReLU / LeakyReLU - Linear
//                                 (HAC/scene/gaussian_model.py:258-262, HAC-plus/scene/gaussian_model.py:117-168, 370-374)
// k_mlp2 states the arithmetic one output per thread; k_mlp2_mfma runs the same fmaf chains on the matrix pipe.
#include "common.hpp"

using namespace gpcc;

namespace {
constexpr int TB = 256;
}  // namespace


// ------------------------------------------------------------------ mlp_grid (a16): Linear - ReLU - Linear
// HAC's context MLP (scene/gaussian_model.py:258-262: Linear(96, 100) - ReLU - Linear(100, 175)) on the hash-grid
// features of a slice of anchors.  Encoder and decoder must obtain bit-identical means / scales / step sizes from it,
// so the arithmetic is specified, as for the geometry heads: acc = bias; for k ascending: acc = fmaf(x[k], W[c][k], acc).
// 16 rows per 256-thread block: the rows and their hidden activations live in LDS, every thread walks the k chain of
// its outputs; the two weight matrices (38 KB + 70 KB) stay in L1/L2.
namespace {
constexpr int MLP_ROWS = 16;
__global__ __launch_bounds__(TB) void k_mlp2(const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1,
                                             const float *__restrict__ w2, const float *__restrict__ b2, int64_t n, int din, int dh, int dout,
                                             float slope, float *__restrict__ y)
{
    extern __shared__ float sm[];
    float *xs = sm, *hs = sm + MLP_ROWS * din;
    const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
    const int rows = (int)min((int64_t)MLP_ROWS, n - row0);
    for (int i = threadIdx.x; i < rows * din; i += TB) xs[i] = x[row0 * din + i];
    __syncthreads();
    for (int i = threadIdx.x; i < rows * dh; i += TB) {
        const int r = i / dh, c = i - r * dh;
        const float *w = w1 + (size_t)c * din, *xr = xs + r * din;
        float acc = b1[c];
        for (int k = 0; k < din; ++k) acc = __builtin_fmaf(xr[k], w[k], acc);
        hs[i] = acc > 0.0f ? acc : (slope != 0.0f ? acc * slope : 0.0f);   // ReLU (slope 0) or LeakyReLU(slope): x > 0 ? x : x * slope
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * dout; i += TB) {
        const int r = i / dout, c = i - r * dout;
        const float *w = w2 + (size_t)c * dh, *hr = hs + r * dh;
        float acc = b2[c];
        for (int k = 0; k < dh; ++k) acc = __builtin_fmaf(hr[k], w[k], acc);
        y[(row0 + r) * dout + c] = acc;
    }
}
}  // namespace

namespace {
// The same two layers on the matrix pipe (round 3; k_mlp2 above stays for layer sizes this kernel does not take and as the
// readable statement of the arithmetic).  v_mfma_f32_16x16x4_f32 with the bias as the initial accumulator is the specified
// chain -- acc = b; for k ascending: acc = fmaf(x[k], W[c][k], acc) -- exactly (the heads of the geometry network rely on the
// same fact): MFMA number kk covers k = 4 kk .. 4 kk + 3, lane group g supplying k = 4 kk + g.  16 rows x 16 outputs per
// accumulator tile: 16 anchors are 7 x 24 + 11 x 25 = 443 MFMAs for HAC's 96-100-175 mlp_grid instead of ~55 k scalar
// fmas per row at one lane each (9.5 ms per million anchors at 5.8 TFLOP/s; the matrix pipes need 0.4 ms).
// One persistent workgroup per CU: both weight matrices in LDS ([c][k] at a pitch of K + 2 floats: the 32 lanes of an LDS
// read group hit 32 different banks), every wave takes whole 16-row tiles: the rows staged in LDS, the hidden layer written
// back over them, no block barrier after the weights have landed.
typedef float f32x4m __attribute__((ext_vector_type(4)));
constexpr int MLPM_WAVES_MAX = 8;   // waves per workgroup: 8 (two per SIMD: one's row loads, stores and drains under the other's MFMA chains) when the class's LDS allows, else 4
// DIN / DH / DOUT are the CLASS of the kernel (register arrays and LDS pitches are compile-time); the layer's own sizes din <= DIN,
// dh <= DH, dout <= DOUT are run-time: weights, biases and input columns beyond them are zeros in LDS, so the chain of an output
// is its own k = 0 .. din - 1 steps followed by fmaf(0, 0, acc) steps, which leave acc unchanged.  HAC's 96-100-175 runs in its
// exact class (no padding); HAC++'s mlp_grid (48-100-195 / 225) and its five channel-context MLPs (150 + 10 c - 40 - 30,
// LeakyReLU) in classes <48, 100, 240> and <192, 40, 32> (HAC-plus/scene/gaussian_model.py:117-168, 370-374).
template <int DIN, int DH, int DOUT>
__global__ __launch_bounds__(64 * MLPM_WAVES_MAX) void k_mlp2_mfma(const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1,
                                                              const float *__restrict__ w2, const float *__restrict__ b2, int64_t n, int din, int dh, int dout,
                                                              float slope, float *__restrict__ y, int PX)
{
    static_assert(DIN % 4 == 0 && DH % 4 == 0, "whole MFMA k-steps");
    constexpr int NT1 = (DH + 15) / 16, NT2 = (DOUT + 15) / 16, P1 = DIN + 2, P2 = DH + 2;
    // W1 holds DH rows and W2 DOUT rows, not whole tiles of 16: the B operands of the last tile's padding outputs are read from whatever follows
    // (inside the allocation) -- they only reach accumulator columns that are never stored (hidden units >= DH, outputs >= dout)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *W1s = sm, *W2s = W1s + DH * P1, *B1s = W2s + DOUT * P2, *B2s = B1s + NT1 * 16, *XS = B2s + NT2 * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, MLPM_WAVES = nthreads >> 6;
    const int e = lane & 15, g = lane >> 4;
    for (int i0 = tid; i0 < DH * DIN; i0 += 4 * nthreads) {     // (four loads in flight per trip, see the tile loads below)
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / DIN, k = i - c * DIN; v[u] = (i < DH * DIN && c < dh && k < din) ? w1[(size_t)c * din + k] : 0.0f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / DIN, k = i - c * DIN; if (i < DH * DIN) W1s[c * P1 + k] = v[u]; }
    }
    for (int i0 = tid; i0 < DOUT * DH; i0 += 4 * nthreads) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / DH, k = i - c * DH; v[u] = (i < DOUT * DH && c < dout && k < dh) ? w2[(size_t)c * dh + k] : 0.0f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * nthreads, c = i / DH, k = i - c * DH; if (i < DOUT * DH) W2s[c * P2 + k] = v[u]; }
    }
    for (int i = tid; i < NT1 * 16; i += nthreads) B1s[i] = i < dh ? b1[i] : 0.0f;
    for (int i = tid; i < NT2 * 16; i += nthreads) B2s[i] = i < dout ? b2[i] : 0.0f;
    __syncthreads();
    float *xs = XS + wave * 16 * PX;
    const int64_t ntiles = (n + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * MLPM_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * MLPM_WAVES) {
        const int64_t row0 = tile * 16;
        // the tile's rows: coalesced float2 loads (rows past n: the last row again), the wave's own LDS slice
        // (loads in batches that are in flight together: as one run-time loop hipcc 7.2 waited for every element before it requested the next --
        //  12 dependent round trips per tile of the 96-column class)
        if (din == DIN) {
            static_assert((16 * DIN / 2) % 64 == 0, "whole trips");
            constexpr int NLD = 16 * DIN / 2 / 64, NB = NLD % 6 == 0 ? 6 : (NLD % 4 == 0 ? 4 : NLD);
            const float *xt = x + (size_t)row0 * DIN;                        // wave-uniform base, 32-bit offsets
            const int last = (int)min((int64_t)15, n - 1 - row0);
#pragma unroll
            for (int b0 = 0; b0 < NLD; b0 += NB) {
                float2 v[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int i = lane + 64 * (b0 + u), r = i / (DIN / 2), c2 = i - r * (DIN / 2);
                    v[u] = *reinterpret_cast<const float2 *>(xt + min(r, last) * DIN + 2 * c2);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int i = lane + 64 * (b0 + u), r = i / (DIN / 2), c2 = i - r * (DIN / 2);
                    *reinterpret_cast<float2 *>(xs + r * PX + 2 * c2) = v[u];
                }
            }
        } else {   // a narrower layer in this class: column by column, zeros beyond din
            const float *xn = x + (size_t)row0 * din;
            const int lastn = (int)min((int64_t)15, n - 1 - row0);
            static_assert((16 * DIN / 64) % 4 == 0, "whole batches");
            for (int i0 = lane; i0 < 16 * DIN; i0 += 4 * 64) {      // unconditional loads (column clamped), four in flight
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int i = i0 + 64 * u, r = i / DIN, c = i - r * DIN; v[u] = xn[min(r, lastn) * din + min(c, din - 1)]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int i = i0 + 64 * u, r = i / DIN, c = i - r * DIN; xs[r * PX + c] = c < din ? v[u] : 0.0f; }
            }
        }
        float a[DIN / 4 > DH / 4 ? DIN / 4 : DH / 4];
#pragma unroll
        for (int kk = 0; kk < DIN / 4; ++kk) a[kk] = xs[e * PX + 4 * kk + g];        // A operand: row e, k = 4 kk + g
        // The weight operands of output tile t + 1 are read from LDS while the MFMAs of tile t run (two register sets, the scheduler held to that order):
        // left to itself the compiler placed every ds_read directly in front of the two MFMAs that use it, with one register pair for all of them --
        // a full LDS round trip (~110 cycles) per 64 cycles of matrix work, which is what "32 % of the fp32 matrix peak" was (round 3's figure).
        f32x4m hid[NT1];
        float wb[2][DIN / 4 > DH / 4 ? DIN / 4 : DH / 4];
        {
            const float *wr = W1s + e * P1 + g;                                    // B operand: output 16 t + e, k = 4 kk + g
#pragma unroll
            for (int kk = 0; kk < DIN / 4; ++kk) wb[0][kk] = wr[4 * kk];
        }
#pragma unroll
        for (int t = 0; t < NT1; ++t) {
            const float bias = B1s[16 * t + e];
            f32x4m acc = {bias, bias, bias, bias};
            if (t + 1 < NT1) {
                const float *wr = W1s + (16 * (t + 1) + e) * P1 + g;
#pragma unroll
                for (int kk = 0; kk < DIN / 4; ++kk) wb[(t + 1) & 1][kk] = wr[4 * kk];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < DIN / 4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], wb[t & 1][kk], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            hid[t] = acc;
        }
        // hidden = relu(...) over the rows' slots: lane (g, e) holds rows 4 g .. 4 g + 3 of output 16 t + e (LDS operations of a
        // wave execute in program order: the A reads above are done)
#pragma unroll
        for (int t = 0; t < NT1; ++t)
            if (16 * t + e < DH) {                 // the padding outputs of the last tile have no slot (and no reader)
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float h = hid[t][i]; xs[(4 * g + i) * PX + 16 * t + e] = h > 0.0f ? h : (slope != 0.0f ? h * slope : 0.0f); }
            }
#pragma unroll
        for (int kk = 0; kk < DH / 4; ++kk) a[kk] = xs[e * PX + 4 * kk + g];
        {
            const float *wr = W2s + e * P2 + g;
#pragma unroll
            for (int kk = 0; kk < DH / 4; ++kk) wb[0][kk] = wr[4 * kk];
        }
#pragma unroll
        for (int t = 0; t < NT2; ++t) {
            const float bias = B2s[16 * t + e];
            f32x4m acc = {bias, bias, bias, bias};
            if (t + 1 < NT2) {
                const float *wr = W2s + (16 * (t + 1) + e) * P2 + g;
#pragma unroll
                for (int kk = 0; kk < DH / 4; ++kk) wb[(t + 1) & 1][kk] = wr[4 * kk];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < DH / 4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], wb[t & 1][kk], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            const int c = 16 * t + e;
            if (c < dout) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (row0 + 4 * g + i < n) y[(size_t)(row0 + 4 * g + i) * dout + c] = acc[i];
            }
        }
    }
}
template <int DIN, int DH, int DOUT>
static size_t mlpm_lds_bytes(int waves, int px)
{
    constexpr int NT1 = (DH + 15) / 16, NT2 = (DOUT + 15) / 16, P1 = DIN + 2, P2 = DH + 2;
    return sizeof(float) * ((size_t)DH * P1 + (size_t)DOUT * P2 + NT1 * 16 + NT2 * 16 + (size_t)waves * 16 * px);
}
}  // namespace

template <int DIN, int DH, int DOUT>
static int mlp2_mfma_launch(gpcc_ctx *ctx, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, int64_t n, int din, int dh, int dout,
                            float slope, float *y, hipStream_t st)
{
    static PerDeviceOnce attr;
    // eight waves when they fit (if need be with the rows' LDS pitch without its two padding words: two-way conflicts on the 49 A-operand reads of a
    // tile, nothing on the 443 B-operand reads), else four
    constexpr int PXW = (DIN > DH ? DIN : DH);
    constexpr size_t LDS_MAX = 160 * 1024;
    int waves = 8, px = PXW + 2;
    if (mlpm_lds_bytes<DIN, DH, DOUT>(8, px) > LDS_MAX) px = PXW;
    if (mlpm_lds_bytes<DIN, DH, DOUT>(8, px) > LDS_MAX) { waves = 4; px = PXW + 2; }
    const size_t lds = mlpm_lds_bytes<DIN, DH, DOUT>(waves, px);
    GP_TRY(attr.run(ctx->device, [&]() -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp2_mfma<DIN, DH, DOUT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
        return GPCC_OK;
    }));
    const unsigned grid = (unsigned)std::min<int64_t>(256, cdiv(cdiv(n, 16), waves));
    k_mlp2_mfma<DIN, DH, DOUT><<<grid, 64 * waves, lds, st>>>(x, w1, b1, w2, b2, n, din, dh, dout, slope, y, px);
    LAUNCH_CHECK();
    return GPCC_OK;
}

// ------------------------------------------------------------------ wide first layers: TC-GS's mlp_triplane, 603-100-175
// (TC-GS/scene/gaussian_model.py: Linear(K * 3 * tri_feat_dim + 3, 2 * feat_dim) - ReLU - Linear(2 * feat_dim, (50 + 6 + 30) * 2 + 3).)  W1 is 100 x 603 floats,
// 241 KB: it does not fit the CU's LDS, so the resident-weights layout above cannot be instantiated.  Here no weight is staged at all: both matrices stay in
// L2 (311 KB together) and a wave reads its B operands from there, one dword per lane and k-step -- W1[16 t + e][4 kk + g] is the 16-byte piece of 16
// consecutive rows -- while it carries FOUR 16-row tiles through the first layer at once (4 x 7 accumulator tiles, 112 registers), so a B operand fetched
// once feeds four MFMAs and W1 crosses the L2 once per 64 rows.  The chain of every output is the specified one: the bias as the initial accumulator, then
// MFMA kk covers k = 4 kk .. 4 kk + 3 in ascending order; k >= din, hidden units >= dh and rows >= n are supplied as zeros (fmaf(0, 0, acc) leaves acc
// unchanged).  Loop bounds follow the layer's own din / dh / dout, so a narrower layer of the class does a narrower layer's work.  The hidden layer of one
// row tile at a time goes through 6.5 KB of the wave's LDS to become the second layer's A operands.
// What this form is not: k-slabs of W1 and of the input rows staged in LDS (a 100 x 64 slab of W1 double-buffered behind a block barrier per slab, the rows'
// slabs beside it), which would turn the 16-byte pieces the x and W1 reads are now (16 rows 4 din bytes apart) into whole lines and let a second wave
// per SIMD cover the loads.  That kernel has not been built or measured.  This one was chosen because it needs no barrier and no LDS for weights and
// is the specified chain by construction; it leaves the pipe at 0.17 of its fp32 peak (27 TFLOP/s at 603-100-175: one wave per SIMD at 189 VGPRs +
// 112 AGPRs waits on every k-step's L2 loads) and is 2.6 x slower than torch's GEMM on the same layer, so slab staging is the known next step.
// Against the plain k_mlp2 it is faster on every shape measured (a million rows, profiles/r07_tcgs_codec.txt): 4.1 x at 603-100-175, 7.4 x at 300-100-175,
// 6.3 x at 128-100-175, 5.8 x at 256-64-32, 2.6 x at 100-64-20, 4.3 x at 64-64-64 -- layers the resident-weights classes miss ran on k_mlp2 before.
template <int DH, int DOUT>
__global__ __launch_bounds__(256) void k_mlp2_mfma_wide(const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1,
                                                        const float *__restrict__ w2, const float *__restrict__ b2, int64_t n, int din, int dh, int dout,
                                                        float slope, float *__restrict__ y)
{
    static_assert(DH % 4 == 0, "whole MFMA k-steps");
    constexpr int RT = 4, NT1 = (DH + 15) / 16, NT2 = (DOUT + 15) / 16, PH = DH + 2;
    __shared__ float hs_all[4][16 * PH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, e = lane & 15, g = lane >> 4;
    float *hs = hs_all[wave];
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
    if (row0 >= n) return;                                  // (no block barrier below: a wave that has no rows leaves)
    f32x4m acc[RT][NT1];
#pragma unroll
    for (int t = 0; t < NT1; ++t) {
        const float bias = 16 * t + e < dh ? b1[16 * t + e] : 0.0f;
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r][t] = f32x4m{bias, bias, bias, bias};
    }
    const float *xr[RT];
    bool rin[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int64_t row = row0 + 16 * r + e;
        rin[r] = row < n;
        xr[r] = x + (size_t)(rin[r] ? row : row0) * din;    // (a row past the end reads nothing: its operand is zero)
    }
    const int nkk = (din + 3) / 4;
    for (int kk = 0; kk < nkk; ++kk) {
        const int k = 4 * kk + g;
        const bool kin = k < din;
        float a[RT], bw[NT1];
#pragma unroll
        for (int r = 0; r < RT; ++r) a[r] = kin && rin[r] ? xr[r][k] : 0.0f;
#pragma unroll
        for (int t = 0; t < NT1; ++t) bw[t] = kin && 16 * t + e < dh ? w1[(size_t)(16 * t + e) * din + k] : 0.0f;
#pragma unroll
        for (int t = 0; t < NT1; ++t) {
            if (16 * t >= dh) break;                        // (wave-uniform)
#pragma unroll
            for (int r = 0; r < RT; ++r) acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], bw[t], acc[r][t], 0, 0, 0);
        }
    }
    const int nk2 = (dh + 3) / 4;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (row0 + 16 * r >= n) break;                      // (wave-uniform)
        // hidden = relu(...) of this row tile: lane (g, e) holds rows 4 g .. 4 g + 3 of unit 16 t + e; units >= dh are exact zeros
#pragma unroll
        for (int t = 0; t < NT1; ++t)
            if (16 * t + e < DH) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float h = acc[r][t][i]; hs[(4 * g + i) * PH + 16 * t + e] = h > 0.0f ? h : (slope != 0.0f ? h * slope : 0.0f); }
            }
        __builtin_amdgcn_wave_barrier();
        float a2[DH / 4];
#pragma unroll
        for (int kk = 0; kk < DH / 4; ++kk) a2[kk] = hs[e * PH + 4 * kk + g];
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int t = 0; t < NT2; ++t) {
            if (16 * t >= dout) break;                      // (wave-uniform)
            const int c = 16 * t + e;
            const bool cin = c < dout;
            const float bias = cin ? b2[c] : 0.0f;
            f32x4m o = {bias, bias, bias, bias};
            const float *wr = w2 + (size_t)(cin ? c : 0) * dh;
            float bw2[DH / 4];
#pragma unroll
            for (int kk = 0; kk < DH / 4; ++kk) bw2[kk] = cin && 4 * kk + g < dh ? wr[4 * kk + g] : 0.0f;
#pragma unroll
            for (int kk = 0; kk < DH / 4; ++kk)
                if (kk < nk2) o = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[kk], bw2[kk], o, 0, 0, 0);
            if (cin) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (row0 + 16 * r + 4 * g + i < n) y[(size_t)(row0 + 16 * r + 4 * g + i) * dout + c] = o[i];
            }
        }
    }
}

template <int DH, int DOUT>
static int mlp2_wide_launch(gpcc_ctx *, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, int64_t n, int din, int dh, int dout,
                            float slope, float *y, hipStream_t st)
{
    k_mlp2_mfma_wide<DH, DOUT><<<(unsigned)cdiv(cdiv(n, 64), 4), 256, 0, st>>>(x, w1, b1, w2, b2, n, din, dh, dout, slope, y);
    LAUNCH_CHECK();
    return GPCC_OK;
}

// act: 0 = ReLU, 1 = LeakyReLU(slope) between the two layers
extern "C" int gshac_mlp2_act(gpcc_ctx *ctx, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, int64_t n, int din, int dh,
                              int dout, int act, float slope, float *y, void *stream)
{
    if (!ctx || !x || !w1 || !b1 || !w2 || !b2 || !y) return fail(GPCC_ERR_ARG, "null argument");
    if (act != 0 && act != 1) return fail(GPCC_ERR_ARG, "mlp2: activation must be 0 (ReLU) or 1 (LeakyReLU)");
    if (n <= 0) return GPCC_OK;
    if (din <= 0 || dh <= 0 || dout <= 0 || (size_t)MLP_ROWS * (size_t)(din + dh) * 4 > 64 * 1024) return fail(GPCC_ERR_ARG, "mlp2: unsupported layer sizes");
    HIP_TRY(hipSetDevice(ctx->device));
    const float sl = act == 1 ? slope : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    static const bool use_mfma = dev_env_int("GAUSPCC_MLP2_MFMA", 1) != 0;
    if (use_mfma) {
        // the smallest class that holds the layer (HAC's mlp_grid in its exact class)
        if (din == 96 && dh == 100 && dout == 175) return mlp2_mfma_launch<96, 100, 175>(ctx, x, w1, b1, w2, b2, n, din, dh, dout, sl, y, st);
        if (din <= 192 && dh <= 40 && dout <= 32) return mlp2_mfma_launch<192, 40, 32>(ctx, x, w1, b1, w2, b2, n, din, dh, dout, sl, y, st);
        if (din <= 48 && dh <= 100 && dout <= 240) return mlp2_mfma_launch<48, 100, 240>(ctx, x, w1, b1, w2, b2, n, din, dh, dout, sl, y, st);
        // TC-GS's mlp_triplane (603-100-175) and what else has a first layer too wide for the resident-weights classes
        if (din <= 608 && dh <= 100 && dout <= 176) return mlp2_wide_launch<100, 176>(ctx, x, w1, b1, w2, b2, n, din, dh, dout, sl, y, st);
    }
    k_mlp2<<<(unsigned)cdiv(n, MLP_ROWS), TB, (size_t)MLP_ROWS * (size_t)(din + dh) * 4, st>>>(x, w1, b1, w2, b2, n, din, dh, dout, sl, y);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gshac_mlp2(gpcc_ctx *ctx, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, int64_t n, int din, int dh,
                          int dout, float *y, void *stream)
{
    return gshac_mlp2_act(ctx, x, w1, b1, w2, b2, n, din, dh, dout, 0, 0.0f, y, stream);
}
