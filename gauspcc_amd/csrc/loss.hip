// loss.hip -- the photometric loss of the 3DGS training step (HAC/utils/loss_utils.py: ssim, l1_loss; the same file in HAC++, TC-GS,
// CAT-3DGS):
//   gsr_ssim_forward   SSIM over a Gaussian window (sigma 1.5, zero padding window_size / 2) of every (batch, channel) plane, its mean
//                      (or per-item means), optionally the mean |x - y| and (1 - l) L1 + l (1 - SSIM); with a gradient pending, the
//                      partial-derivative maps the backward reads
//   gsr_ssim_backward  dL/dx and dL/dy from those maps
//
// One workgroup = one 32 x 32 output tile of one plane.  The tile plus a halo of R = window_size / 2 is staged in LDS (outside the image:
// 0, the reference's zero padding), a horizontal pass gives the row sums of the five products for the tile's columns over all staged rows,
// a vertical pass gives the five moments of each output.  The window is the outer product of the float32 1-D taps (symmetric), so the
// backward's transposed correlation is the same separable correlation, applied to the maps.
//
// Per pixel, in float32 with the reference's grouping (sigma^2 = E - mu^2):
//   A = 2 mu1 mu2 + C1, B = 2 (E[xy] - mu1 mu2) + C2, C = (mu1^2 + mu2^2) + C1, D = ((E[x^2] - mu1^2) + (E[y^2] - mu2^2)) + C2, S = AB / (CD)
// Maps (the closed forms of include/gauspcc.h, regrouped so that equal images give exactly 0):
//   m1 = dS/dmu1  = 2 (mu2 (B - A) + mu1 S (C - D)) / (CD)          m3 = dS/dE[xy] = 2 t,  t = A / (CD)
//   m2 = dS/dE[x^2] = dS/dE[y^2] = -t (B / D)                        m4 = dS/dmu2  = 2 (mu1 (B - A) + mu2 S (C - D)) / (CD)
// With x = y everywhere: A = C and B = D bit for bit, S = 1, m1 = m4 = 0 and m3 = -2 m2, so the gradient's two E terms cancel exactly.
//
// Sums: each workgroup writes (sum S, sum |x - y|) in double to its slot; k_ssim_reduce adds the slots in a fixed order.  No atomics:
// results are bitwise reproducible.
#include "common.hpp"

#include <math.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int TW = 32, TH = 32;          // output tile; a thread owns one column and 4 consecutive rows of it
constexpr int ROWS_PER_THREAD = TH / (TB / TW);
constexpr int MAX_R = 15;                // window_size <= 31
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct Taps {
    float w[2 * MAX_R + 1];
};

struct Plane {
    int H, W, C;                         // image size, channels (plane p belongs to batch item p / C)
    int tiles_x, tiles;                  // tiles per row, per plane
};

__device__ __forceinline__ void tile_of(const Plane &P, int &plane, int &y0, int &x0)
{
    plane = blockIdx.x / P.tiles;
    const int t = blockIdx.x - plane * P.tiles;
    y0 = (t / P.tiles_x) * TH;
    x0 = (t % P.tiles_x) * TW;
}

// fixed-order sum of two doubles per thread; thread 0 writes the totals
__device__ __forceinline__ void block_sum2(double a, double b, double2 *s, double2 *out)
{
    s[threadIdx.x] = make_double2(a, b);
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s[threadIdx.x].x += s[threadIdx.x + w].x;
            s[threadIdx.x].y += s[threadIdx.x + w].y;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// ------------------------------------------------------------------ forward: moments, S, maps, per-workgroup sums
template <int R>
__global__ __launch_bounds__(TB) void k_ssim_fwd(const float *__restrict__ x, const float *__restrict__ y, Plane P, Taps T,
                                                 float *__restrict__ maps, int nmaps, int64_t map_stride, double2 *__restrict__ part)
{
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    __shared__ float2 sxy[SH][SW];
    __shared__ float hm[5][SH][TW];
    __shared__ double2 red[TB];

    int plane, y0, x0;
    tile_of(P, plane, y0, x0);
    const int64_t base = (int64_t)plane * P.H * P.W;
    for (int i = threadIdx.x; i < SH * SW; i += TB) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 - R + r, gx = x0 - R + c;
        float2 v = make_float2(0.f, 0.f);
        if (gy >= 0 && gy < P.H && gx >= 0 && gx < P.W) {
            const int64_t o = base + (int64_t)gy * P.W + gx;
            v = make_float2(x[o], y[o]);
        }
        sxy[r][c] = v;
    }
    __syncthreads();

    const int c = threadIdx.x % TW;
    for (int r = threadIdx.x / TW; r < SH; r += TB / TW) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const float2 v = sxy[r][c + k];
            const float w = T.w[k];
            a0 = fmaf(w, v.x, a0);
            a1 = fmaf(w, v.y, a1);
            a2 = fmaf(w, v.x * v.x, a2);
            a3 = fmaf(w, v.y * v.y, a3);
            a4 = fmaf(w, v.x * v.y, a4);
        }
        hm[0][r][c] = a0; hm[1][r][c] = a1; hm[2][r][c] = a2; hm[3][r][c] = a3; hm[4][r][c] = a4;
    }
    __syncthreads();

    const int r0 = (threadIdx.x / TW) * ROWS_PER_THREAD;
    float m[ROWS_PER_THREAD][5];
#pragma unroll
    for (int o = 0; o < ROWS_PER_THREAD; ++o)
#pragma unroll
        for (int q = 0; q < 5; ++q) m[o][q] = 0.f;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD + 2 * R; ++j) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hm[q][r0 + j][c];
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; ++o) {
            const int k = j - o;
            if (k >= 0 && k <= 2 * R) {
#pragma unroll
                for (int q = 0; q < 5; ++q) m[o][q] = fmaf(T.w[k], v[q], m[o][q]);
            }
        }
    }

    float ssum = 0.f, lsum = 0.f;
    const int gx = x0 + c;
#pragma unroll
    for (int o = 0; o < ROWS_PER_THREAD; ++o) {
        const int gy = y0 + r0 + o;
        if (gy >= P.H || gx >= P.W) continue;
        const float mu1 = m[o][0], mu2 = m[o][1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = m[o][2] - mu1_sq, s2 = m[o][3] - mu2_sq, s12 = m[o][4] - mu12;
        const float A = 2.f * mu12 + C1, B = 2.f * s12 + C2;
        const float Cc = (mu1_sq + mu2_sq) + C1, D = (s1 + s2) + C2;
        const float cd = Cc * D;
        const float S = (A * B) / cd;
        const float2 v = sxy[R + r0 + o][R + c];
        ssum += S;
        lsum += fabsf(v.x - v.y);
        if (nmaps) {
            const int64_t p = base + (int64_t)gy * P.W + gx;
            const float t = A / cd, bma = B - A, cmd = Cc - D;
            maps[p] = 2.f * (mu2 * bma + (mu1 * S) * cmd) / cd;
            maps[map_stride + p] = -(t * (B / D));
            maps[2 * map_stride + p] = 2.f * t;
            if (nmaps == 4) maps[3 * map_stride + p] = 2.f * (mu1 * bma + (mu2 * S) * cmd) / cd;
        }
    }
    block_sum2((double)ssum, (double)lsum, red, &part[blockIdx.x]);
}

// ------------------------------------------------------------------ the means: one workgroup per output, slots in a fixed order
// out[b] = sum of S over the slots of item b / n; with l1 (one output only): l1 = sum |x - y| / n, loss = k1 l1 + lam (1 - out[0])
__global__ __launch_bounds__(TB) void k_ssim_reduce(const double2 *__restrict__ part, int64_t slots_per_out, double n, float *__restrict__ out,
                                                    float *__restrict__ l1, float *__restrict__ loss, float k1, float lam)
{
    __shared__ double2 red[TB];
    __shared__ double2 tot;
    const double2 *p = part + (int64_t)blockIdx.x * slots_per_out;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < slots_per_out; i += TB) {
        a += p[i].x;
        b += p[i].y;
    }
    block_sum2(a, b, red, &tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float s = (float)(tot.x / n);
        out[blockIdx.x] = s;
        if (l1) {
            const float v = (float)(tot.y / n);
            *l1 = v;
            if (loss) *loss = k1 * v + lam * (1.f - s);
        }
    }
}

// ------------------------------------------------------------------ backward: correlate the maps, combine with x, y
// dx(p) = gs [ (W*m1)(p) + 2 x(p) (W*m2)(p) + y(p) (W*m3)(p) ] + gl sign(x - y)
// dy(p) = gs [ (W*m4)(p) + 2 y(p) (W*m2)(p) + x(p) (W*m3)(p) ] - gl sign(x - y)
template <int R>
__global__ __launch_bounds__(TB) void k_ssim_bwd(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ maps,
                                                 int nmaps, int64_t map_stride, Plane P, Taps T, const float *__restrict__ gssim, int per_item,
                                                 float ssim_scale, float nssim, const float *__restrict__ gl1, float l1_scale, float nl1,
                                                 float *__restrict__ dx, float *__restrict__ dy)
{
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    __shared__ float4 sm[SH][SW];
    __shared__ float4 hm[SH][TW];

    int plane, y0, x0;
    tile_of(P, plane, y0, x0);
    const int64_t base = (int64_t)plane * P.H * P.W;
    for (int i = threadIdx.x; i < SH * SW; i += TB) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 - R + r, gx = x0 - R + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < P.H && gx >= 0 && gx < P.W) {
            const int64_t o = base + (int64_t)gy * P.W + gx;
            v.x = maps[o];
            v.y = maps[map_stride + o];
            v.z = maps[2 * map_stride + o];
            if (nmaps == 4) v.w = maps[3 * map_stride + o];
        }
        sm[r][c] = v;
    }
    __syncthreads();

    const int c = threadIdx.x % TW;
    for (int r = threadIdx.x / TW; r < SH; r += TB / TW) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const float4 v = sm[r][c + k];
            const float w = T.w[k];
            a.x = fmaf(w, v.x, a.x);
            a.y = fmaf(w, v.y, a.y);
            a.z = fmaf(w, v.z, a.z);
            a.w = fmaf(w, v.w, a.w);
        }
        hm[r][c] = a;
    }
    __syncthreads();

    const int r0 = (threadIdx.x / TW) * ROWS_PER_THREAD;
    float4 s[ROWS_PER_THREAD];
#pragma unroll
    for (int o = 0; o < ROWS_PER_THREAD; ++o) s[o] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD + 2 * R; ++j) {
        const float4 v = hm[r0 + j][c];
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; ++o) {
            const int k = j - o;
            if (k >= 0 && k <= 2 * R) {
                const float w = T.w[k];
                s[o].x = fmaf(w, v.x, s[o].x);
                s[o].y = fmaf(w, v.y, s[o].y);
                s[o].z = fmaf(w, v.z, s[o].z);
                s[o].w = fmaf(w, v.w, s[o].w);
            }
        }
    }

    const int item = plane / P.C;
    const float gs = ssim_scale * gssim[per_item ? item : 0] / nssim;
    const float gl = gl1 ? l1_scale * gl1[0] / nl1 : 0.f;
    const int gx = x0 + c;
#pragma unroll
    for (int o = 0; o < ROWS_PER_THREAD; ++o) {
        const int gy = y0 + r0 + o;
        if (gy >= P.H || gx >= P.W) continue;
        const int64_t p = base + (int64_t)gy * P.W + gx;
        const float xv = x[p], yv = y[p];
        const float d = xv - yv;
        const float sg = (float)(d > 0.f) - (float)(d < 0.f);
        // products rounded one by one (no fma): with equal images the two E terms are exact negatives
        if (dx) {
            float g = gs * ((s[o].x + (2.f * xv) * s[o].y) + yv * s[o].z);
            if (gl1) g += gl * sg;
            dx[p] = g;
        }
        if (dy) {
            float g = gs * ((s[o].w + (2.f * yv) * s[o].y) + xv * s[o].z);
            if (gl1) g -= gl * sg;
            dy[p] = g;
        }
    }
}

void load_taps(const float *taps, int ws, Taps &T)
{
    for (int i = 0; i <= 2 * MAX_R; ++i) T.w[i] = i < ws ? taps[i] : 0.f;
}

int check_shape(const char *who, int64_t b, int64_t c, int64_t h, int64_t w, int ws, Plane &P, int64_t &blocks)
{
    if (b < 1 || c < 1 || h < 1 || w < 1 || h > INT32_MAX || w > INT32_MAX || c > INT32_MAX)
        return fail(GPCC_ERR_ARG, "%s: shape (%lld, %lld, %lld, %lld)", who, (long long)b, (long long)c, (long long)h, (long long)w);
    if (ws < 1 || ws > 2 * MAX_R + 1 || ws % 2 == 0) return fail(GPCC_ERR_ARG, "%s: window_size %d is not odd in [1, %d]", who, ws, 2 * MAX_R + 1);
    const int64_t tiles = cdiv(w, TW) * cdiv(h, TH);
    if (tiles > ((int64_t)1 << 24) || b * c > ((int64_t)1 << 24) || tiles * b * c > ((int64_t)1 << 24))
        return fail(GPCC_ERR_ARG, "%s: (%lld, %lld, %lld, %lld) needs more than 2^24 tiles of %dx%d", who, (long long)b, (long long)c, (long long)h,
                    (long long)w, TW, TH);
    P.H = (int)h; P.W = (int)w; P.C = (int)c;
    P.tiles_x = (int)cdiv(w, TW);
    P.tiles = (int)tiles;
    blocks = tiles * b * c;
    return GPCC_OK;
}

}  // namespace

#define SSIM_RADII(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

extern "C" int gsr_ssim_forward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t batch, int64_t channels, int64_t height, int64_t width,
                                int window_size, const float *taps, int size_average, float *ssim_out, float *l1_out, float *loss_out, double lambda_dssim,
                                float *maps, int nmaps, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsr_ssim_forward: null context");
    Plane P;
    int64_t blocks;
    GP_TRY(check_shape("gsr_ssim_forward", batch, channels, height, width, window_size, P, blocks));
    if (!img1 || !img2 || !taps || !ssim_out || !alloc) return fail(GPCC_ERR_ARG, "gsr_ssim_forward: null argument");
    if (nmaps != 0 && nmaps != 3 && nmaps != 4) return fail(GPCC_ERR_ARG, "gsr_ssim_forward: nmaps = %d not in {0, 3, 4}", nmaps);
    if (nmaps && !maps) return fail(GPCC_ERR_ARG, "gsr_ssim_forward: null maps");
    if ((l1_out || loss_out) && !size_average) return fail(GPCC_ERR_ARG, "gsr_ssim_forward: l1 / loss need size_average");
    if (loss_out && !l1_out) return fail(GPCC_ERR_ARG, "gsr_ssim_forward: loss needs l1_out");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    double2 *part;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)blocks * sizeof(double2), &part, "gsr_ssim_forward"));

    Taps T;
    load_taps(taps, window_size, T);
    const int64_t n = batch * channels * height * width;
    switch (window_size / 2) {
#define SSIM_FWD(R) case R: k_ssim_fwd<R><<<(unsigned)blocks, TB, 0, st>>>(img1, img2, P, T, maps, nmaps, n, part); break;
        SSIM_RADII(SSIM_FWD)
#undef SSIM_FWD
    }
    LAUNCH_CHECK();
    const int nout = size_average ? 1 : (int)batch;
    const double per = size_average ? (double)n : (double)(channels * height * width);
    k_ssim_reduce<<<nout, TB, 0, st>>>(part, blocks / nout, per, ssim_out, l1_out, loss_out, (float)(1.0 - lambda_dssim), (float)lambda_dssim);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_ssim_backward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t batch, int64_t channels, int64_t height, int64_t width,
                                 int window_size, const float *taps, int size_average, const float *maps, int nmaps, const float *grad_ssim, float ssim_scale,
                                 const float *grad_l1, float l1_scale, float *grad_img1, float *grad_img2, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsr_ssim_backward: null context");
    Plane P;
    int64_t blocks;
    GP_TRY(check_shape("gsr_ssim_backward", batch, channels, height, width, window_size, P, blocks));
    if (!img1 || !img2 || !taps || !maps || !grad_ssim) return fail(GPCC_ERR_ARG, "gsr_ssim_backward: null argument");
    if (nmaps != 3 && nmaps != 4) return fail(GPCC_ERR_ARG, "gsr_ssim_backward: nmaps = %d not in {3, 4}", nmaps);
    if (grad_img2 && nmaps != 4) return fail(GPCC_ERR_ARG, "gsr_ssim_backward: grad_img2 needs the fourth map");
    if (grad_l1 && !size_average) return fail(GPCC_ERR_ARG, "gsr_ssim_backward: l1 needs size_average");
    if (!grad_img1 && !grad_img2) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;

    Taps T;
    load_taps(taps, window_size, T);
    const int64_t n = batch * channels * height * width;
    const float nssim = size_average ? (float)n : (float)(channels * height * width), nl1 = (float)n;
    switch (window_size / 2) {
#define SSIM_BWD(R)                                                                                                                  \
    case R:                                                                                                                          \
        k_ssim_bwd<R><<<(unsigned)blocks, TB, 0, st>>>(img1, img2, maps, nmaps, n, P, T, grad_ssim, !size_average, ssim_scale, nssim, \
                                                       grad_l1, l1_scale, nl1, grad_img1, grad_img2);                                \
        break;
        SSIM_RADII(SSIM_BWD)
#undef SSIM_BWD
    }
    LAUNCH_CHECK();
    return GPCC_OK;
}
