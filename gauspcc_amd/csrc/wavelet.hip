// wavelet.hip -- TC-GS's wavelet term of the training loss (TC-GS/utils/loss_utils.py:66-83: wavelet_loss) and the one-level Haar
// transform pair behind gauspcc_amd.wavelets (the DWTForward / DWTInverse the reference takes from pytorch_wavelets, wave 'haar',
// mode 'zero'):
//   gsr_wavelet_l1_forward    the weighted sum of the seven band L1 means of a two-level Haar DWT of two images, one pass
//   gsr_wavelet_l1_backward   its gradient for either image, one pass, nothing saved
//   gsr_haar_forward          one level: a plane to LL and the three detail bands
//   gsr_haar_inverse          one level back; also the adjoint of gsr_haar_forward (Haar is orthonormal)
//
// The transform (float32, products rounded one by one): s = (float)0.7071067811865476, a plane reads as zero outside.  On a quad a b / c d
// the row pass gives lo0 = a s + b s, hi0 = a s - b s, lo1 = c s + d s, hi1 = c s - d s, the column pass
//   LL = lo0 s + lo1 s,  band0 = lo0 s - lo1 s (high along height),  band1 = hi0 s + hi1 s (high along width),  band2 = hi0 s - hi1 s.
// The filters have two taps and stride two, so quads do not overlap: two levels of an image are one pass over its 4 x 4 pixel blocks,
// each giving 12 level-1 detail coefficients, 4 LL1 values, and from those 3 level-2 detail coefficients and 1 LL2.
//
// Loss kernels: one lane owns one 4 x 4 block of one plane, a wave's lanes are adjacent in x.  With W a multiple of 4 and 16-byte
// aligned images a block is four 16-byte row loads per image; otherwise guarded scalar loads.  Pixels outside the image read as zero,
// so coefficients outside a band are 0 in both images and add nothing to the sums or to the gradient.
// Sums: seven per lane, added over the wave and the workgroup in double, one record of seven doubles per workgroup; k_wavelet_finish
// adds the records in a fixed order.  No atomics: results are bitwise reproducible.
#include "common.hpp"

#include <math.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int WAVE = 64;
constexpr int NB = 7;                    // LL2, level-1 bands 0..2, level-2 bands 0..2
constexpr float S = 0.7071067811865476f;

struct Geom {
    int H, W;
    int nbx, nby;                        // 4 x 4 blocks per row, per column of a plane
    int64_t lanes;                       // planes * nby * nbx
    int vec;                             // rows are whole float4s at 16-byte aligned addresses
};

struct BandScale {
    double w[NB];                        // forward: the weight of band b
    double inv_count[NB];                // forward: 1 / (planes h_b w_b)
    float k[NB];                         // backward: w[b] / count_b
};

struct Coef {
    float ll2, d1[4][3], d2[3];          // d1[q]: quad q = 2 qy + qx of the block
};

__device__ __forceinline__ void haar_quad(float a, float b, float c, float d, float &ll, float &b0, float &b1, float &b2)
{
    const float lo0 = a * S + b * S, hi0 = a * S - b * S;
    const float lo1 = c * S + d * S, hi1 = c * S - d * S;
    ll = lo0 * S + lo1 * S;
    b0 = lo0 * S - lo1 * S;
    b1 = hi0 * S + hi1 * S;
    b2 = hi0 * S - hi1 * S;
}

__device__ __forceinline__ void block_coefs(const float p[4][4], Coef &c)
{
    float ll1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = 2 * (q >> 1), x = 2 * (q & 1);
        haar_quad(p[y][x], p[y][x + 1], p[y + 1][x], p[y + 1][x + 1], ll1[q], c.d1[q][0], c.d1[q][1], c.d1[q][2]);
    }
    haar_quad(ll1[0], ll1[1], ll1[2], ll1[3], c.ll2, c.d2[0], c.d2[1], c.d2[2]);
}

__device__ __forceinline__ bool block_of(const Geom &G, int &plane, int &y0, int &x0)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= G.lanes) return false;
    const int64_t t = i / G.nbx;
    x0 = (int)(i - t * G.nbx) * 4;
    plane = (int)(t / G.nby);
    y0 = (int)(t - (int64_t)plane * G.nby) * 4;
    return true;
}

__device__ __forceinline__ void load_block(const float *__restrict__ img, const Geom &G, int plane, int y0, int x0, float p[4][4])
{
    const float *base = img + ((int64_t)plane * G.H + y0) * G.W + x0;
    if (G.vec) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y0 + r < G.H) v = *reinterpret_cast<const float4 *>(base + (int64_t)r * G.W);
            p[r][0] = v.x; p[r][1] = v.y; p[r][2] = v.z; p[r][3] = v.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) p[r][c] = (y0 + r < G.H && x0 + c < G.W) ? base[(int64_t)r * G.W + c] : 0.f;
    }
}

// the coefficients of img1's block minus those of img2's
__device__ __forceinline__ void diff_coefs(const float *__restrict__ x, const float *__restrict__ y, const Geom &G, int plane, int y0, int x0, Coef &d)
{
    float p[4][4];
    Coef cx, cy;
    load_block(x, G, plane, y0, x0, p);
    block_coefs(p, cx);
    load_block(y, G, plane, y0, x0, p);
    block_coefs(p, cy);
    d.ll2 = cx.ll2 - cy.ll2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) d.d1[q][k] = cx.d1[q][k] - cy.d1[q][k];
        d.d2[k] = cx.d2[k] - cy.d2[k];
    }
}

// fixed-order sums of NB doubles per thread: afterwards tot[b], b < NB, is valid in every thread with threadIdx.x < NB
__device__ __forceinline__ double block_sum7(double s[NB], double (*red)[NB])
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) s[b] += __shfl_down(s[b], off, WAVE);
    if (threadIdx.x % WAVE == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) red[threadIdx.x / WAVE][b] = s[b];
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < NB) {
#pragma unroll
        for (int w = 0; w < TB / WAVE; ++w) t += red[w][threadIdx.x];
    }
    return t;
}

// ------------------------------------------------------------------ loss forward
__global__ __launch_bounds__(TB) void k_wavelet_fwd(const float *__restrict__ x, const float *__restrict__ y, Geom G, double *__restrict__ part)
{
    __shared__ double red[TB / WAVE][NB];
    double s[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) s[b] = 0.0;
    int plane, y0, x0;
    if (block_of(G, plane, y0, x0)) {
        Coef d;
        diff_coefs(x, y, G, plane, y0, x0, d);
        s[0] = (double)fabsf(d.ll2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[1 + k] = ((double)fabsf(d.d1[0][k]) + (double)fabsf(d.d1[1][k])) + ((double)fabsf(d.d1[2][k]) + (double)fabsf(d.d1[3][k]));
            s[4 + k] = (double)fabsf(d.d2[k]);
        }
    }
    const double t = block_sum7(s, red);
    if (threadIdx.x < NB) part[(int64_t)blockIdx.x * NB + threadIdx.x] = t;
}

// one workgroup: bands[b] = sum_b / count_b, loss = sum over the bands with a weight of w[b] bands[b]
__global__ __launch_bounds__(TB) void k_wavelet_finish(const double *__restrict__ part, int64_t nrec, BandScale B, float *__restrict__ loss,
                                                       float *__restrict__ bands)
{
    __shared__ double red[TB / WAVE][NB];
    __shared__ double mean[NB];
    double s[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) s[b] = 0.0;
    for (int64_t i = threadIdx.x; i < nrec; i += TB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) s[b] += part[i * NB + b];
    }
    const double t = block_sum7(s, red);
    if (threadIdx.x < NB) mean[threadIdx.x] = t * B.inv_count[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0;
        for (int b = 0; b < NB; ++b) {
            if (bands) bands[b] = (float)mean[b];
            if (B.w[b] != 0.0) l += B.w[b] * mean[b];
        }
        *loss = (float)l;
    }
}

// ------------------------------------------------------------------ loss backward
__device__ __forceinline__ float sgn(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }
// the sign of pixel (py, px) of a quad in band k: band0 is high along height, band1 high along width, band2 both
__device__ __forceinline__ float pat(int k, int py, int px) { return (k == 0 ? py : k == 1 ? px : (py ^ px)) ? -1.f : 1.f; }

__global__ __launch_bounds__(TB) void k_wavelet_bwd(const float *__restrict__ x, const float *__restrict__ y, Geom G, BandScale B,
                                                    const float *__restrict__ grad, float *__restrict__ dx, float *__restrict__ dy)
{
    int plane, y0, x0;
    if (!block_of(G, plane, y0, x0)) return;
    Coef d;
    diff_coefs(x, y, G, plane, y0, x0, d);
    const float g = grad[0];
    float c[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) c[b] = g * B.k[b];
    float e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e2[k] = sgn(d.d2[k]) * c[4 + k];
    const float e0 = sgn(d.ll2) * c[0];
    float out[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int qy = q >> 1, qx = q & 1;
        // d loss / d LL1[q]: LL2 and the level-2 bands hold LL1[q] with +-1/2, a pixel holds LL1[q] with 1/2
        const float t = 0.25f * (e0 + ((pat(0, qy, qx) * e2[0] + pat(1, qy, qx) * e2[1]) + pat(2, qy, qx) * e2[2]));
        float e1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) e1[k] = sgn(d.d1[q][k]) * c[1 + k];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px)
                out[2 * qy + py][2 * qx + px] = 0.5f * ((pat(0, py, px) * e1[0] + pat(1, py, px) * e1[1]) + pat(2, py, px) * e1[2]) + t;
    }
    const int64_t base = ((int64_t)plane * G.H + y0) * G.W + x0;
    if (G.vec) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (y0 + r >= G.H) continue;
            const int64_t o = base + (int64_t)r * G.W;
            if (dx) *reinterpret_cast<float4 *>(dx + o) = make_float4(out[r][0], out[r][1], out[r][2], out[r][3]);
            if (dy) *reinterpret_cast<float4 *>(dy + o) = make_float4(-out[r][0], -out[r][1], -out[r][2], -out[r][3]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                if (y0 + r >= G.H || x0 + cc >= G.W) continue;
                const int64_t o = base + (int64_t)r * G.W + cc;
                if (dx) dx[o] = out[r][cc];
                if (dy) dy[o] = -out[r][cc];
            }
    }
}

// ------------------------------------------------------------------ one level, forward and inverse
// one lane = one coefficient position (r, k) of one plane: the quad x[2r..2r+1][2k..2k+1]
__global__ __launch_bounds__(TB) void k_haar_fwd(const float *__restrict__ x, int H, int W, int h, int w, int64_t n, int vec,
                                                 float *__restrict__ ll, float *__restrict__ high)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int64_t t = i / w;
    const int k = (int)(i - t * w);
    const int64_t plane = t / h;
    const int r = (int)(t - plane * h);
    const float *base = x + (plane * H + 2 * r) * W + 2 * k;
    float a, b = 0.f, c = 0.f, d = 0.f;
    const bool row1 = 2 * r + 1 < H;
    if (vec) {
        const float2 u = *reinterpret_cast<const float2 *>(base);
        a = u.x; b = u.y;
        if (row1) {
            const float2 v = *reinterpret_cast<const float2 *>(base + W);
            c = v.x; d = v.y;
        }
    } else {
        const bool col1 = 2 * k + 1 < W;
        a = base[0];
        if (col1) b = base[1];
        if (row1) c = base[W];
        if (row1 && col1) d = base[W + 1];
    }
    float o0, o1, o2, o3;
    haar_quad(a, b, c, d, o0, o1, o2, o3);
    const int64_t hw = (int64_t)h * w, pos = (int64_t)r * w + k;
    ll[plane * hw + pos] = o0;
    float *hp = high + plane * 3 * hw + pos;
    hp[0] = o1;
    hp[hw] = o2;
    hp[2 * hw] = o3;
}

// the column pass back first (lo, hi of the two rows), then the row pass; outputs beyond (Ho, Wo) are the cropped padding
__global__ __launch_bounds__(TB) void k_haar_inv(const float *__restrict__ ll, const float *__restrict__ high, int h, int w, int64_t n, int Ho, int Wo,
                                                 int vec, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int64_t t = i / w;
    const int k = (int)(i - t * w);
    const int64_t plane = t / h;
    const int r = (int)(t - plane * h);
    const int64_t hw = (int64_t)h * w, pos = (int64_t)r * w + k;
    const float v0 = ll[plane * hw + pos];
    float v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (high) {
        const float *hp = high + plane * 3 * hw + pos;
        v1 = hp[0]; v2 = hp[hw]; v3 = hp[2 * hw];
    }
    const float lo0 = v0 * S + v1 * S, lo1 = v0 * S - v1 * S;
    const float hi0 = v2 * S + v3 * S, hi1 = v2 * S - v3 * S;
    const float a = lo0 * S + hi0 * S, b = lo0 * S - hi0 * S;
    const float c = lo1 * S + hi1 * S, d = lo1 * S - hi1 * S;
    float *base = out + (plane * Ho + 2 * r) * Wo + 2 * k;
    const bool row1 = 2 * r + 1 < Ho;
    if (vec) {
        *reinterpret_cast<float2 *>(base) = make_float2(a, b);
        if (row1) *reinterpret_cast<float2 *>(base + Wo) = make_float2(c, d);
    } else {
        const bool col1 = 2 * k + 1 < Wo;
        base[0] = a;
        if (col1) base[1] = b;
        if (row1) base[Wo] = c;
        if (row1 && col1) base[Wo + 1] = d;
    }
}

bool aligned(const void *p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

int loss_geometry(const char *who, int64_t planes, int64_t H, int64_t W, const double *weights, Geom &G, BandScale &B, int64_t &groups)
{
    if (planes < 1 || H < 1 || W < 1 || planes > INT32_MAX || H > INT32_MAX - 3 || W > INT32_MAX - 3)
        return fail(GPCC_ERR_ARG, "%s: shape (%lld, %lld, %lld)", who, (long long)planes, (long long)H, (long long)W);
    if (!weights) return fail(GPCC_ERR_ARG, "%s: null weights", who);
    const int64_t nbx = cdiv(W, 4), nby = cdiv(H, 4);
    groups = nbx * nby > ((int64_t)1 << 32) ? -1 : cdiv(planes * nbx * nby, TB);   // the product stays below 2^63
    if (groups < 0 || groups > ((int64_t)1 << 24))
        return fail(GPCC_ERR_ARG, "%s: (%lld, %lld, %lld) needs more than 2^24 workgroups of %d 4x4 blocks", who, (long long)planes, (long long)H,
                    (long long)W, TB);
    G.H = (int)H; G.W = (int)W; G.nbx = (int)nbx; G.nby = (int)nby;
    G.lanes = planes * nbx * nby;
    G.vec = W % 4 == 0;
    const int64_t h1 = cdiv(H, 2), w1 = cdiv(W, 2), h2 = cdiv(h1, 2), w2 = cdiv(w1, 2);
    for (int b = 0; b < NB; ++b) {
        const double count = (double)planes * (double)(b >= 1 && b <= 3 ? h1 * w1 : h2 * w2);
        B.w[b] = weights[b];
        B.inv_count[b] = 1.0 / count;
        B.k[b] = (float)(weights[b] / count);
    }
    return GPCC_OK;
}

int level_geometry(const char *who, int64_t planes, int64_t h, int64_t w, int64_t H, int64_t W, int64_t &n, int64_t &groups)
{
    if (planes < 1 || h < 1 || w < 1 || h > INT32_MAX / 2 || w > INT32_MAX / 2)
        return fail(GPCC_ERR_ARG, "%s: shape (%lld, %lld, %lld)", who, (long long)planes, (long long)h, (long long)w);
    if ((H != 2 * h && H != 2 * h - 1) || (W != 2 * w && W != 2 * w - 1))
        return fail(GPCC_ERR_ARG, "%s: a (%lld, %lld) plane does not belong to (%lld, %lld) bands", who, (long long)H, (long long)W, (long long)h, (long long)w);
    if (planes > ((int64_t)1 << 32) / cdiv(h * w, TB)) return fail(GPCC_ERR_ARG, "%s: (%lld, %lld, %lld) needs more than 2^32 lanes", who, (long long)planes, (long long)h, (long long)w);
    n = planes * h * w;
    groups = cdiv(n, TB);
    if (groups > ((int64_t)1 << 24)) return fail(GPCC_ERR_ARG, "%s: (%lld, %lld, %lld) needs more than 2^24 workgroups", who, (long long)planes, (long long)h, (long long)w);
    return GPCC_OK;
}

}  // namespace

extern "C" int gsr_wavelet_l1_forward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t planes, int64_t height, int64_t width,
                                      const double *weights, float *loss_out, float *bands_out, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsr_wavelet_l1_forward: null context");
    Geom G;
    BandScale B;
    int64_t groups;
    GP_TRY(loss_geometry("gsr_wavelet_l1_forward", planes, height, width, weights, G, B, groups));
    if (!img1 || !img2 || !loss_out || !alloc) return fail(GPCC_ERR_ARG, "gsr_wavelet_l1_forward: null argument");
    G.vec = G.vec && aligned(img1, 16) && aligned(img2, 16);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    double *part;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)groups * NB * sizeof(double), &part, "gsr_wavelet_l1_forward"));
    k_wavelet_fwd<<<(unsigned)groups, TB, 0, st>>>(img1, img2, G, part);
    LAUNCH_CHECK();
    k_wavelet_finish<<<1, TB, 0, st>>>(part, groups, B, loss_out, bands_out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_wavelet_l1_backward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t planes, int64_t height, int64_t width,
                                       const double *weights, const float *grad_loss, float *grad_img1, float *grad_img2, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsr_wavelet_l1_backward: null context");
    Geom G;
    BandScale B;
    int64_t groups;
    GP_TRY(loss_geometry("gsr_wavelet_l1_backward", planes, height, width, weights, G, B, groups));
    if (!img1 || !img2 || !grad_loss) return fail(GPCC_ERR_ARG, "gsr_wavelet_l1_backward: null argument");
    if (!grad_img1 && !grad_img2) return GPCC_OK;
    G.vec = G.vec && aligned(img1, 16) && aligned(img2, 16) && aligned(grad_img1, 16) && aligned(grad_img2, 16);
    HIP_TRY(hipSetDevice(ctx->device));
    k_wavelet_bwd<<<(unsigned)groups, TB, 0, (hipStream_t)stream>>>(img1, img2, G, B, grad_loss, grad_img1, grad_img2);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_haar_forward(gpcc_ctx *ctx, const float *x, int64_t planes, int64_t height, int64_t width, float *ll_out, float *high_out, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsr_haar_forward: null context");
    if (height < 1 || width < 1) return fail(GPCC_ERR_ARG, "gsr_haar_forward: shape (%lld, %lld, %lld)", (long long)planes, (long long)height, (long long)width);
    const int64_t h = cdiv(height, 2), w = cdiv(width, 2);
    int64_t n, groups;
    GP_TRY(level_geometry("gsr_haar_forward", planes, h, w, height, width, n, groups));
    if (!x || !ll_out || !high_out) return fail(GPCC_ERR_ARG, "gsr_haar_forward: null argument");
    const int vec = width % 2 == 0 && aligned(x, 8);
    HIP_TRY(hipSetDevice(ctx->device));
    k_haar_fwd<<<(unsigned)groups, TB, 0, (hipStream_t)stream>>>(x, (int)height, (int)width, (int)h, (int)w, n, vec, ll_out, high_out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_haar_inverse(gpcc_ctx *ctx, const float *ll, const float *high, int64_t planes, int64_t h, int64_t w, float *out, int64_t out_height,
                                int64_t out_width, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gsr_haar_inverse: null context");
    int64_t n, groups;
    GP_TRY(level_geometry("gsr_haar_inverse", planes, h, w, out_height, out_width, n, groups));
    if (!ll || !out) return fail(GPCC_ERR_ARG, "gsr_haar_inverse: null argument");
    const int vec = out_width % 2 == 0 && aligned(out, 8);
    HIP_TRY(hipSetDevice(ctx->device));
    k_haar_inv<<<(unsigned)groups, TB, 0, (hipStream_t)stream>>>(ll, high, (int)h, (int)w, n, (int)out_height, (int)out_width, vec, out);
    LAUNCH_CHECK();
    return GPCC_OK;
}
