// triplane.hip -- TC-GS's tri-plane context sampler (TC-GS/utils/triplane.py: sample_from_planes, Triplane.sample), forward and backward:
//   gsge_plane_forward   out (N, K 3 C): every sample (n, k) read bilinearly from the three (C, H, W) feature planes
//   gsge_plane_backward  the plane gradient (no float atomics) and, when wanted, the coordinate gradient
//   gsge_plane_rows_forward / _backward   the same with an output row of K 3 C + T floats whose last T columns are a copy of a row-aligned
//                        (N, T) tail (TC-GS: the anchor, T = 3: the (N, 603) input of mlp_triplane, without torch.cat); the backward reads the
//                        upstream gradient in place with that row stride.  The two entry points above forward here with T = 0: the same bits.
//
// Arithmetic per sample and plane p, float32 in the reference's expression order (include/gauspcc.h has the full contract):
//   mag_p = sqrt(min(min(|proj_p(max)|^2, |proj_p(min)|^2), radii^2)), proj_0 = (x, y), proj_1 = (x, z), proj_2 = (z, x)
//   u_0 = (c.y, c.z), u_1 = (c.x, c.z), u_2 = (c.x, c.y) of c = 2 coordinate;  x = 6 (u / mag_p * 2 - 1);  m = max(|x|^2, eps)
//   z = x (m <= 1) or ((2 sqrt(m) - 1) / m) x;  g = z / 2;  pixel = ((g + 1) size - 1) / 2, g[0] along W, g[1] along H
//   bilinear, corners outside the plane contribute 0.  A pixel coordinate that is not finite gives zeros and no gradient; no index is formed.
//
// The planes are first transposed to channel-last (3, H W, C) in the caller's workspace (3 C H W floats, read and written once: ~1 % of the
// output's traffic at 1 M anchors): a corner is then C contiguous floats instead of C cache lines.
// Forward: a workgroup owns whole output rows -- floor(PF_SAMPLES / K) of them, K 3 C + T floats each -- which is a contiguous piece of the
// row-major output because the tensor is exactly that wide.  One thread per (sample, plane) leaves four texel indices and weights in LDS;
// then the workgroup walks its output elements in order (element -> row and column by one magic division, feature column -> slot and channel
// by a second; tail columns are copied from the tail), so a wave's scalar stores (and its four corner reads) are contiguous: 256 bytes per
// store instruction wherever a row starts.  The repeat form (coordinates (N, 3), K copies) computes an anchor's three entries once and
// writes them to the K slots the walk reads.  With T = 0 and (N, K, 3) coordinates the output is (N K, 3 C) in all but name: rows of one
// sample, 64 per workgroup, for any K.
// Backward, planes: one (texel row, slot) entry per (sample, plane, corner), sentinel for padding corners; stable radix sort by texel row;
// sorted_sum.hpp's sum and combine with one wave per chunk of PB_CHUNK entries and one lane per channel, into a channel-last gradient that
// is transposed back to (3, C, H, W).  The repeat form first adds the K copies of the upstream gradient per (n, plane) in k order.
// Backward, coordinates: one thread per sample.  All three read the upstream gradient through GradRows: row n of it starts at n * stride.
#include "common.hpp"
#include "primitives.hpp"
#include "sorted_sum.hpp"

#include <float.h>
#include <math.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int PF_SAMPLES = 64;            // (n, k) samples per forward workgroup, at most
constexpr int PF_SLOTS = PF_SAMPLES * 3;  // their (sample, plane) entries
constexpr int MAX_C = 256, MAX_SIZE = 4096, MAX_TAIL = 16;
constexpr int PB_CHUNK = 256;             // sorted entries per wave of the sum pass
constexpr int PB_WALK = 8;

struct Geom {
    int C, H, W;
    int rep;           // output copies per coordinate row (1: coordinates are (N, K, 3))
    uint32_t magic;    // floor(2^32 / C) + 1: e / C = umulhi(e, magic) for e < 2^16 (C >= 2)
    float radii_sq;
    // the output rows: `per` coordinate rows and `slots` = (sample, plane) entries each, slots C + tail floats wide, `rows` of them per workgroup
    int per, slots, tail, rows;
    uint32_t width, magic_w;   // width = slots C + tail >= 3; floor(2^32 / width) + 1, for e < 2^16 as above
};

// The upstream gradient of (coordinate row, plane) entry u, C contiguous floats: entry u of a contiguous (U, C) matrix (per == 0), or entry
// u % per of row u / per of a matrix whose rows are `stride` floats apart (the (N, K 3 C + T) gradient read in place).
struct GradRows {
    const float *__restrict__ g;
    int64_t stride;
    uint32_t per;
    int C;
    __device__ __forceinline__ const float *at(uint32_t u) const
    {
        if (per == 0) return g + (int64_t)u * C;
        const uint32_t n = u / per;
        return g + (int64_t)n * stride + (int64_t)(u - n * per) * C;
    }
};

// sqrt(mag_sq[p]) from the bounds (device memory: no host copy, no synchronisation)
__device__ __forceinline__ float plane_mag(const float *__restrict__ mx, const float *__restrict__ mn, float radii_sq, int p)
{
    const int i = p == 2 ? 2 : 0, j = p == 0 ? 1 : (p == 1 ? 2 : 0);
    const float smax = mx[i] * mx[i] + mx[j] * mx[j], smin = mn[i] * mn[i] + mn[j] * mn[j];
    return sqrtf(fminf(fminf(smax, smin), radii_sq));
}

struct Pixel {
    float ix, iy;      // pixel coordinates along W and H
    float x0, x1, m;   // the contraction's input and its clamped squared norm
};

// c: the coordinate row (3 floats); the plane's two components are a (along W) and b (along H)
__device__ __forceinline__ Pixel plane_pixel(const float *__restrict__ c, int p, float mag, int H, int W)
{
    const float a = 2.0f * c[p == 0 ? 1 : 0], b = 2.0f * c[p == 2 ? 1 : 2];
    Pixel q;
    q.x0 = 6.0f * (a / mag * 2.0f - 1.0f);
    q.x1 = 6.0f * (b / mag * 2.0f - 1.0f);
    const float n2 = q.x0 * q.x0 + q.x1 * q.x1;
    q.m = n2 < FLT_EPSILON ? FLT_EPSILON : n2;     // NaN stays NaN, as torch.clamp keeps it
    float z0 = q.x0, z1 = q.x1;
    if (!(q.m <= 1.0f)) {
        const float s = (2.0f * sqrtf(q.m) - 1.0f) / q.m;
        z0 = s * q.x0;
        z1 = s * q.x1;
    }
    q.ix = ((0.5f * z0 + 1.0f) * (float)W - 1.0f) * 0.5f;
    q.iy = ((0.5f * z1 + 1.0f) * (float)H - 1.0f) * 0.5f;
    return q;
}

// The four corners in grid_sample's order nw, ne, sw, se: texel index within the three planes (p H W + y W + x), -1 for a corner outside
// the plane, and the weights as grid_sample forms them.  Bounds are tested on the floats; only an in-range value becomes an index.
__device__ __forceinline__ bool plane_corners(const Pixel &q, int p, int H, int W, int (&t)[4], float (&w)[4])
{
    if (!(isfinite(q.ix) && isfinite(q.iy))) {
        for (int c = 0; c < 4; ++c) { t[c] = -1; w[c] = 0.0f; }
        return false;
    }
    const float xw = floorf(q.ix), yn = floorf(q.iy), xe = xw + 1.0f, ys = yn + 1.0f;
    w[0] = (xe - q.ix) * (ys - q.iy);
    w[1] = (q.ix - xw) * (ys - q.iy);
    w[2] = (xe - q.ix) * (q.iy - yn);
    w[3] = (q.ix - xw) * (q.iy - yn);
    const bool inx0 = xw >= 0.0f && xw < (float)W, inx1 = xe >= 0.0f && xe < (float)W;
    const bool iny0 = yn >= 0.0f && yn < (float)H, iny1 = ys >= 0.0f && ys < (float)H;
    const int x0 = inx0 ? (int)xw : 0, x1 = inx1 ? (int)xe : 0, y0 = iny0 ? (int)yn : 0, y1 = iny1 ? (int)ys : 0;
    const int base = p * H * W;
    t[0] = inx0 && iny0 ? base + y0 * W + x0 : -1;
    t[1] = inx1 && iny0 ? base + y0 * W + x1 : -1;
    t[2] = inx0 && iny1 ? base + y1 * W + x0 : -1;
    t[3] = inx1 && iny1 ? base + y1 * W + x1 : -1;
    return true;
}

// ------------------------------------------------------------------ (B, R, S) -> (B, S, R), 32 x 32 tiles through LDS
__global__ __launch_bounds__(TB) void k_plane_transpose(const float *__restrict__ in, float *__restrict__ out, int R, int S, int tiles_s)
{
    __shared__ float tile[32][33];
    const int tr = blockIdx.x / tiles_s, ts = blockIdx.x - tr * tiles_s;
    const int64_t base = (int64_t)blockIdx.y * R * S;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int j = ly; j < 32; j += TB / 32) {
        const int r = tr * 32 + j, s = ts * 32 + lx;
        if (r < R && s < S) tile[j][lx] = in[base + (int64_t)r * S + s];
    }
    __syncthreads();
    for (int j = ly; j < 32; j += TB / 32) {
        const int s = ts * 32 + j, r = tr * 32 + lx;
        if (r < R && s < S) out[base + (int64_t)s * R + r] = tile[lx][j];
    }
}

void transpose_launch(hipStream_t st, const float *in, float *out, int batch, int64_t R, int64_t S)
{
    const int64_t tiles_s = cdiv(S, 32), tiles_r = cdiv(R, 32);
    k_plane_transpose<<<dim3((unsigned)(tiles_r * tiles_s), batch), TB, 0, st>>>(in, out, (int)R, (int)S, (int)tiles_s);
}

// ------------------------------------------------------------------ forward
// NR output rows; workgroup b owns rows [b G.rows, (b + 1) G.rows): their G.per coordinate rows each and their G.width output floats each.
// G.rows G.per G.rep <= PF_SAMPLES samples, so the slots fit the LDS tables and an element index stays below 2^16.
__global__ __launch_bounds__(TB) void k_plane_fwd(const float *__restrict__ planes_cl, const float *__restrict__ coords, const float *__restrict__ maxc,
                                                  const float *__restrict__ minc, const float *__restrict__ tail, Geom G, int64_t NR,
                                                  float *__restrict__ out)
{
    __shared__ int4 st[PF_SLOTS];
    __shared__ float4 sw[PF_SLOTS];
    const int64_t a0 = (int64_t)blockIdx.x * G.rows;
    const int na = (int)min((int64_t)G.rows, NR - a0);
    const int64_t r0 = a0 * G.per;
    const int nr = na * G.per;
    for (int u = threadIdx.x; u < nr * 3; u += TB) {
        const int r = u / 3, p = u - 3 * r;
        const Pixel q = plane_pixel(coords + (r0 + r) * 3, p, plane_mag(maxc, minc, G.radii_sq, p), G.H, G.W);
        int t[4];
        float w[4];
        plane_corners(q, p, G.H, G.W, t, w);
        for (int k = 0; k < G.rep; ++k) {
            const int slot = (r * G.rep + k) * 3 + p;
            st[slot] = make_int4(t[0], t[1], t[2], t[3]);
            sw[slot] = make_float4(w[0], w[1], w[2], w[3]);
        }
    }
    __syncthreads();
    const uint32_t C = (uint32_t)G.C, width = G.width, feat = width - (uint32_t)G.tail, ne = (uint32_t)na * width;
    float *o = out + a0 * (int64_t)width;
    const float *tl = tail ? tail + a0 * G.tail : nullptr;
    for (uint32_t e = threadIdx.x; e < ne; e += TB) {
        uint32_t a = 0, col = e;
        if (G.tail) {      // without a tail the rows are one run of slots: no row boundary to find
            a = __umulhi(e, G.magic_w);
            col = e - a * width;
            if (col >= feat) {
                o[e] = tl[a * (uint32_t)G.tail + (col - feat)];
                continue;
            }
        }
        const uint32_t sl = C == 1 ? col : __umulhi(col, G.magic), ch = col - sl * C;
        const uint32_t slot = a * (uint32_t)G.slots + sl;
        const int4 t = st[slot];
        const float4 w = sw[slot];
        float v = 0.0f;
        if (t.x >= 0) v = __builtin_fmaf(planes_cl[(int64_t)t.x * C + ch], w.x, v);
        if (t.y >= 0) v = __builtin_fmaf(planes_cl[(int64_t)t.y * C + ch], w.y, v);
        if (t.z >= 0) v = __builtin_fmaf(planes_cl[(int64_t)t.z * C + ch], w.z, v);
        if (t.w >= 0) v = __builtin_fmaf(planes_cl[(int64_t)t.w * C + ch], w.w, v);
        o[e] = v;
    }
}

// ------------------------------------------------------------------ backward
// repeat form: folded[(n 3 + p) C + ch] = sum over k, in k order, of grad[n stride + (k 3 + p) C + ch]
__global__ __launch_bounds__(TB) void k_plane_fold(const float *__restrict__ grad, int64_t stride, int64_t total, int row, int K, float *__restrict__ folded)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= total) return;
    const int64_t n = i / row;
    const float *g = grad + n * stride + (i - n * row);
    float s = g[0];
    for (int k = 1; k < K; ++k) s += g[(int64_t)k * row];
    folded[i] = s;
}

// one thread per (coordinate row, plane) u: slots 4 u .. 4 u + 3
__global__ __launch_bounds__(TB) void k_plane_keys(const float *__restrict__ coords, const float *__restrict__ maxc, const float *__restrict__ minc, Geom G,
                                                   int64_t U, uint32_t n_rows, uint64_t *__restrict__ keys, uint32_t *__restrict__ slots,
                                                   float *__restrict__ wts)
{
    const int64_t u = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (u >= U) return;
    const int64_t r = u / 3;
    const int p = (int)(u - 3 * r);
    const Pixel q = plane_pixel(coords + r * 3, p, plane_mag(maxc, minc, G.radii_sq, p), G.H, G.W);
    int t[4];
    float w[4];
    plane_corners(q, p, G.H, G.W, t, w);
    for (int c = 0; c < 4; ++c) {
        const int64_t s = u * 4 + c;
        keys[s] = t[c] >= 0 ? (uint32_t)t[c] : n_rows;
        slots[s] = (uint32_t)s;
        wts[s] = w[c];
    }
}

// one lane = one channel of the wave's chunk; g: upstream gradient per (coordinate row, plane), C contiguous floats each
struct PlaneRowSum {
    GradRows g;
    const uint32_t *__restrict__ slots;
    const float *__restrict__ wts;
    float *__restrict__ grad_cl, *__restrict__ head, *__restrict__ tail;
    int C, ch;
    float acc;
    __device__ __forceinline__ void zero() { acc = 0.0f; }
    __device__ __forceinline__ void add(int64_t i)
    {
        const uint32_t s = slots[i];
        acc = __builtin_fmaf(wts[s], g.at(s >> 2)[ch], acc);
    }
    __device__ __forceinline__ void to_head(int64_t t) { head[t * C + ch] = acc; }
    __device__ __forceinline__ void to_tail(int64_t t) { tail[t * C + ch] = acc; }
    __device__ __forceinline__ void to_row(uint32_t row) { grad_cl[(int64_t)row * C + ch] = acc; }
};

// grad_cl is zeroed before: a texel row is written once, by the sum or by the combine pass
__global__ __launch_bounds__(TB) void k_plane_bwd_sum(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slots, const float *__restrict__ wts,
                                                      GradRows g, int C, int64_t E, uint32_t n_rows, float *__restrict__ grad_cl,
                                                      float *__restrict__ head, float *__restrict__ tail, uint8_t *__restrict__ own)
{
    const int64_t t = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    const int ch = blockIdx.y * 64 + (threadIdx.x & 63);
    if (t * PB_CHUNK >= E || ch >= C) return;
    PlaneRowSum a{g, slots, wts, grad_cl, head, tail, C, ch, 0.0f};
    sorted_chunk_sum<PB_CHUNK>(keys, t, E, n_rows, a, own);   // every lane of the chunk writes the same own[t]
}

__global__ __launch_bounds__(TB) void k_plane_bwd_combine(const uint64_t *__restrict__ keys, int64_t E, int64_t nchunks, const float *__restrict__ head,
                                                          const float *__restrict__ tail, const uint8_t *__restrict__ own, int C,
                                                          float *__restrict__ grad_cl)
{
    const int64_t t = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    const int ch = blockIdx.y * 64 + (threadIdx.x & 63);
    if (ch >= C) return;
    sorted_combine<PB_CHUNK, 1, PB_WALK>(keys, E, nchunks, t, head + ch, tail + ch, C, own,
                                         [&](uint32_t row, const float (&s)[1]) { grad_cl[(int64_t)row * C + ch] = s[0]; });
}

// Coordinate gradient, one thread per coordinate row.  d out / d pixel as grid_sample's backward forms it, then through
// pixel = ((g + 1) size - 1) / 2, g = z / 2, z = contract(x) (both branches), x = 6 (2 c / mag * 2 - 1).
__global__ __launch_bounds__(TB) void k_plane_bwd_coords(const float *__restrict__ planes_cl, const float *__restrict__ coords, const float *__restrict__ maxc,
                                                         const float *__restrict__ minc, Geom G, int64_t M, GradRows g,
                                                         float *__restrict__ grad_coords)
{
    const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (r >= M) return;
    const int C = G.C;
    float gc[3] = {0.0f, 0.0f, 0.0f};
    for (int p = 0; p < 3; ++p) {
        const float mag = plane_mag(maxc, minc, G.radii_sq, p);
        const Pixel q = plane_pixel(coords + r * 3, p, mag, G.H, G.W);
        int t[4];
        float w[4];
        if (!plane_corners(q, p, G.H, G.W, t, w)) continue;
        const float xw = floorf(q.ix), yn = floorf(q.iy);
        const float dxe = (xw + 1.0f) - q.ix, dxw = q.ix - xw, dys = (yn + 1.0f) - q.iy, dyn = q.iy - yn;
        const float *go = g.at((uint32_t)(r * 3 + p));
        float gix = 0.0f, giy = 0.0f;
        for (int ch = 0; ch < C; ++ch) {
            const float gv = go[ch];
            const float nw = t[0] >= 0 ? planes_cl[(int64_t)t[0] * C + ch] : 0.0f, ne = t[1] >= 0 ? planes_cl[(int64_t)t[1] * C + ch] : 0.0f;
            const float sw = t[2] >= 0 ? planes_cl[(int64_t)t[2] * C + ch] : 0.0f, se = t[3] >= 0 ? planes_cl[(int64_t)t[3] * C + ch] : 0.0f;
            gix = __builtin_fmaf((ne - nw) * dys + (se - sw) * dyn, gv, gix);
            giy = __builtin_fmaf((sw - nw) * dxe + (se - ne) * dxw, gv, giy);
        }
        // d pixel / d z = size / 4
        const float gz0 = gix * (0.25f * (float)G.W), gz1 = giy * (0.25f * (float)G.H);
        float gx0 = gz0, gx1 = gz1;
        if (!(q.m <= 1.0f)) {
            // z = s(m) x, s = (2 sqrt(m) - 1) / m, ds/dm = (1 - sqrt(m)) / m^2, m = |x|^2
            const float rt = sqrtf(q.m), s = (2.0f * rt - 1.0f) / q.m, ds = (1.0f - rt) / (q.m * q.m);
            const float dot = 2.0f * ds * (gz0 * q.x0 + gz1 * q.x1);
            gx0 = __builtin_fmaf(dot, q.x0, s * gz0);
            gx1 = __builtin_fmaf(dot, q.x1, s * gz1);
        }
        // d x / d coordinate = 6 * 2 * 2 / mag
        const float k = 24.0f / mag;
        gc[p == 0 ? 1 : 0] += k * gx0;
        gc[p == 2 ? 1 : 2] += k * gx1;
    }
    for (int d = 0; d < 3; ++d) grad_coords[r * 3 + d] = gc[d];
}

uint32_t magic_of(int d) { return (uint32_t)((((uint64_t)1 << 32) / (uint64_t)d) + 1); }

// NR: the output rows the forward's workgroups are dealt (n, or n k one-sample rows when there is no tail and no repeat)
int check_args(const char *who, int64_t n, int k, int repeat, int C, int H, int W, int T, Geom &G, int64_t &M, int64_t &NR)
{
    if (n < 0 || k < 1) return fail(GPCC_ERR_ARG, "%s: n = %lld, k = %d", who, (long long)n, k);
    if (C < 1 || C > MAX_C) return fail(GPCC_ERR_ARG, "%s: %d channels outside [1, %d]", who, C, MAX_C);
    if (H < 2 || H > MAX_SIZE || W < 2 || W > MAX_SIZE) return fail(GPCC_ERR_ARG, "%s: planes of %d x %d outside [2, %d]", who, H, W, MAX_SIZE);
    if (T < 0 || T > MAX_TAIL) return fail(GPCC_ERR_ARG, "%s: a tail of %d columns outside [0, %d]", who, T, MAX_TAIL);
    if (repeat && k > PF_SAMPLES) return fail(GPCC_ERR_ARG, "%s: repeat = %d above %d", who, k, PF_SAMPLES);
    if (T && k > PF_SAMPLES) return fail(GPCC_ERR_ARG, "%s: k = %d above %d with a tail (a workgroup owns whole rows)", who, k, PF_SAMPLES);
    if (n * k * 12 >= ((int64_t)1 << 32)) return fail(GPCC_ERR_ARG, "%s: %lld x %d samples: more than 2^32 (sample, plane, corner) slots", who, (long long)n, k);
    G.C = C; G.H = H; G.W = W;
    G.rep = repeat ? k : 1;
    G.magic = magic_of(C);   // unused for C = 1
    M = repeat ? n : n * k;
    G.tail = T;
    if (T == 0 && !repeat) {     // (n k, 3 C): rows of one sample
        NR = n * k;
        G.per = 1; G.slots = 3; G.rows = PF_SAMPLES;
    } else {
        NR = n;
        G.per = repeat ? 1 : k; G.slots = 3 * k; G.rows = PF_SAMPLES / k;
    }
    G.width = (uint32_t)(G.slots * C + T);
    G.magic_w = magic_of((int)G.width);
    return GPCC_OK;
}

}  // namespace

extern "C" int gsge_plane_rows_forward(gpcc_ctx *ctx, const float *planes, const float *coordinates, const float *max_coords, const float *min_coords,
                                       double radii, int64_t n, int k, int repeat, int channels, int height, int width, const float *tail, int tail_width,
                                       float *out, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    const char *who = tail_width ? "gsge_plane_rows_forward" : "gsge_plane_forward";
    if (!ctx) return fail(GPCC_ERR_ARG, "%s: null context", who);
    Geom G;
    int64_t M, NR;
    GP_TRY(check_args(who, n, k, repeat, channels, height, width, tail_width, G, M, NR));
    if (n == 0) return GPCC_OK;
    if (!planes || !coordinates || !max_coords || !min_coords || !out || !alloc || (tail_width && !tail)) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    G.radii_sq = (float)(radii * radii);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)height * width;
    float *planes_cl;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)(3 * HW * channels) * sizeof(float), &planes_cl, who));
    transpose_launch(st, planes, planes_cl, 3, channels, HW);
    LAUNCH_CHECK();
    k_plane_fwd<<<(unsigned)cdiv(NR, G.rows), TB, 0, st>>>(planes_cl, coordinates, max_coords, min_coords, tail_width ? tail : nullptr, G, NR, out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsge_plane_forward(gpcc_ctx *ctx, const float *planes, const float *coordinates, const float *max_coords, const float *min_coords,
                                  double radii, int64_t n, int k, int repeat, int channels, int height, int width, float *out, gsr_alloc_fn alloc,
                                  void *alloc_user, void *stream)
{
    return gsge_plane_rows_forward(ctx, planes, coordinates, max_coords, min_coords, radii, n, k, repeat, channels, height, width, nullptr, 0, out, alloc,
                                   alloc_user, stream);
}

extern "C" int gsge_plane_rows_backward(gpcc_ctx *ctx, const float *grad_out, const float *planes, const float *coordinates, const float *max_coords,
                                        const float *min_coords, double radii, int64_t n, int k, int repeat, int channels, int height, int width,
                                        int tail_width, float *grad_planes, float *grad_coordinates, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    const char *who = tail_width ? "gsge_plane_rows_backward" : "gsge_plane_backward";
    if (!ctx) return fail(GPCC_ERR_ARG, "%s: null context", who);
    Geom G;
    int64_t M, NR;
    GP_TRY(check_args(who, n, k, repeat, channels, height, width, tail_width, G, M, NR));
    if (!grad_planes || !alloc) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int C = channels;
    const int64_t HW = (int64_t)height * width, plane_floats = 3 * HW * C;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(grad_planes, 0, (size_t)plane_floats * sizeof(float), st));
        return GPCC_OK;
    }
    if (!grad_out || !planes || !coordinates || !max_coords || !min_coords) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    G.radii_sq = (float)(radii * radii);
    const bool fold = repeat && k > 1;
    const int64_t U = M * 3, E = U * 4, nchunks = cdiv(E, PB_CHUNK);
    const int64_t stride = (int64_t)k * 3 * C + tail_width;      // floats between two rows of grad_out
    const uint32_t n_rows = (uint32_t)(3 * HW);
    uint64_t *ka, *kb;
    uint32_t *va, *vb, *hist;
    float *wts, *head, *tail, *grad_cl, *planes_cl = nullptr, *folded = nullptr;
    uint8_t *own;
    GP_TRY(caller_block(alloc, alloc_user, who, [&](Carver &c) {
        ka = c.take<uint64_t>(E); kb = c.take<uint64_t>(E); va = c.take<uint32_t>(E); vb = c.take<uint32_t>(E); wts = c.take<float>(E);
        hist = c.take<uint32_t>(radix_sort_hist_words(E)); head = c.take<float>(nchunks * C); tail = c.take<float>(nchunks * C);
        own = c.take<uint8_t>(nchunks); grad_cl = c.take<float>(plane_floats);
        if (grad_coordinates) planes_cl = c.take<float>(plane_floats);
        if (fold) folded = c.take<float>(U * C);
    }));
    // entry u = (coordinate row, plane): contiguous without a tail (and after the fold); else 3 k entries per row of grad_out (3 in the
    // repeat form with k = 1)
    GradRows g{grad_out, stride, tail_width ? (uint32_t)(3 * k) : 0u, C};
    if (fold) {
        k_plane_fold<<<(unsigned)cdiv(U * C, TB), TB, 0, st>>>(grad_out, stride, U * C, 3 * C, k, folded);
        LAUNCH_CHECK();
        g = GradRows{folded, 0, 0u, C};
    }
    k_plane_keys<<<(unsigned)cdiv(U, TB), TB, 0, st>>>(coordinates, max_coords, min_coords, G, U, n_rows, ka, va, wts);
    LAUNCH_CHECK();
    int bits = 1;
    while (((int64_t)1 << bits) <= (int64_t)n_rows) ++bits;    // the sentinel n_rows sorts last
    uint64_t *k0 = ka, *k1 = kb;
    uint32_t *v0 = va, *v1 = vb;
    GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, E, bits, hist));
    HIP_TRY(hipMemsetAsync(grad_cl, 0, (size_t)plane_floats * sizeof(float), st));
    const dim3 grid((unsigned)cdiv(nchunks, TB / 64), (unsigned)cdiv(C, 64));
    k_plane_bwd_sum<<<grid, TB, 0, st>>>(k0, v0, wts, g, C, E, n_rows, grad_cl, head, tail, own);
    LAUNCH_CHECK();
    k_plane_bwd_combine<<<grid, TB, 0, st>>>(k0, E, nchunks, head, tail, own, C, grad_cl);
    LAUNCH_CHECK();
    transpose_launch(st, grad_cl, grad_planes, 3, HW, C);
    LAUNCH_CHECK();
    if (grad_coordinates) {
        transpose_launch(st, planes, planes_cl, 3, C, HW);
        LAUNCH_CHECK();
        k_plane_bwd_coords<<<(unsigned)cdiv(M, TB), TB, 0, st>>>(planes_cl, coordinates, max_coords, min_coords, G, M, g, grad_coordinates);
        LAUNCH_CHECK();
    }
    return GPCC_OK;
}

extern "C" int gsge_plane_backward(gpcc_ctx *ctx, const float *grad_out, const float *planes, const float *coordinates, const float *max_coords,
                                   const float *min_coords, double radii, int64_t n, int k, int repeat, int channels, int height, int width,
                                   float *grad_planes, float *grad_coordinates, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    return gsge_plane_rows_backward(ctx, grad_out, planes, coordinates, max_coords, min_coords, radii, n, k, repeat, channels, height, width, 0, grad_planes,
                                    grad_coordinates, alloc, alloc_user, stream);
}
