// ms_triplane.hip -- CAT-3DGS's multi-scale tri-plane features (CAT-3DGS/scene/triplane.py: TriPlaneField.forward, get_density,
// interpolate_ms_features, grid_sample_wrapper), forward and backward:
//   gsge_msplane_forward   out (N, L 3 C): every point read bilinearly from the three (C, H, W) planes of each of L levels, the levels
//                          accumulated (F_l = T_l + F_{l-1} while level > l) and concatenated
//   gsge_msplane_backward  one gradient per plane (no float atomics) and, on the normalize_aabb path, the coordinate gradient
//
// Arithmetic per point, float32 in the reference's expression order (include/gauspcc.h has the full contract):
//   contract:  p = pts - pca_mean; q_j = sum_i p_i R[i][j]; q = q / variance; x = ((q + 1) / 2) * 2 - 1; mag = |x|_2
//              x = (2 - 1 / mag) (x / mag) m + x (1 - m), m = (mag > 1) as 0 / 1 (the reference's blend); x = x / 4 + 0.5
//              g = (x - con_aabb[0]) * ((aabb[1] - aabb[0]) / (con_aabb[1] - con_aabb[0])) + aabb[0]
//   otherwise: g = (pts - aabb[0]) * (2 / (aabb[1] - aabb[0])) - 1      (contract = 2: the last line of the transform alone; 3: g = pts)
//   plane p of every level reads components (0, 1), (0, 2), (1, 2) of g, the first along W: pixel = (g + 1) / 2 * (size - 1) clamped to
//   [0, size - 1] (align_corners, border padding); a corner at index `size` has weight 0 and is never read.
//   A point whose g is not finite gives a zero row and no gradient; no index is formed from it.
//
// All 3 L planes are first transposed to channel-last rows in the caller's workspace, one row space: plane i's texel (y, x) is row
// base_i + y W_i + x of C contiguous floats.  The quantiser rintf(16 v) / 16 is applied there, once per texel.
// Forward: a workgroup owns PTS = MF_SLOTS / (3 L) consecutive points = a contiguous piece of the output.  One thread per point leaves g
// in LDS, one thread per (point, level, plane) four rows and weights; then thread e = (point, plane, channel) walks the levels with the
// running sum in a register and stores L values: a wave's stores and corner reads are contiguous runs of 3 C floats (four channels per
// lane as one float4 when C is a multiple of 4).
// Backward, planes: one (row, slot) entry per (point, level, plane, corner), sentinel for corners that are not read and for levels
// that `level` leaves out; stable radix sort by row; sorted_sum.hpp's sum and combine with one wave per chunk and one lane per channel;
// the upstream gradient of level l is formed on the fly as the sum of the grad_out blocks l' >= l in ascending order.  The channel-last
// gradient is transposed back into the caller's per-plane tensors.
// Backward, coordinates: one wave per point, one lane per channel, the lanes added in a fixed butterfly.
#include "common.hpp"
#include "primitives.hpp"
#include "sorted_sum.hpp"

#include <float.h>
#include <math.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int MAX_LEVELS = 8, MAX_PLANES = 3 * MAX_LEVELS;
constexpr int MF_SLOTS = 192;             // (point, level, plane) entries per forward workgroup: MF_SLOTS * MAX_C < 2^16 (the magic division)
constexpr int MAX_C = 256, MAX_SIZE = 4096;
constexpr int MB_CHUNK = 256;             // sorted entries per wave of the sum pass
constexpr int MB_WALK = 8;

struct MsGeom {
    int C, L, level, contract;            // contract: 0 normalize_aabb, 1 the whole transform, 2 con_normalize_aabb alone, 3 none
    int vec;                              // channels per lane of the forward walk: 4 when C is a multiple of 4 and out is 16-byte aligned, else 1
    uint32_t magic;                       // floor(2^32 / CV) + 1, CV = C / vec: e / CV = umulhi(e, magic) for e < 2^16 (CV >= 2)
    int H[MAX_PLANES], W[MAX_PLANES];
    uint32_t base[MAX_PLANES + 1];        // first row of plane i; base[3 L] = all rows
};

struct MsPlanes {
    float *p[MAX_PLANES];
};

struct MsXform {
    const float *pca_mean, *rotation, *variance, *aabb, *con_aabb;
};

// level l takes part in the output (and has a gradient)
__device__ __forceinline__ bool level_used(const MsGeom &G, int l) { return l == 0 || G.level > l; }

// g (3) of one point; false when a component is not finite
__device__ __forceinline__ bool ms_grid_coord(const float *__restrict__ pt, const MsGeom &G, const MsXform &X, float (&g)[3])
{
    const float *a0 = X.aabb, *a1 = X.aabb + 3;
    if (G.contract == 1) {
        float p[3], x[3];
        for (int i = 0; i < 3; ++i) p[i] = pt[i] - X.pca_mean[i];
        for (int j = 0; j < 3; ++j) {
            const float q = (p[0] * X.rotation[j] + p[1] * X.rotation[3 + j] + p[2] * X.rotation[6 + j]) / X.variance[j];
            x[j] = ((q + 1.0f) / 2.0f) * 2.0f - 1.0f;
        }
        const float mag = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        const float m = mag > 1.0f ? 1.0f : 0.0f;
        for (int j = 0; j < 3; ++j) {
            const float xc = (2.0f - 1.0f / mag) * (x[j] / mag);
            const float y = (xc * m + x[j] * (1.0f - m)) / 4.0f + 0.5f;
            const float *c0 = X.con_aabb, *c1 = X.con_aabb + 3;
            g[j] = (y - c0[j]) * ((a1[j] - a0[j]) / (c1[j] - c0[j])) + a0[j];
        }
    } else if (G.contract == 2) {
        const float *c0 = X.con_aabb, *c1 = X.con_aabb + 3;
        for (int j = 0; j < 3; ++j) g[j] = (pt[j] - c0[j]) * ((a1[j] - a0[j]) / (c1[j] - c0[j])) + a0[j];
    } else if (G.contract == 3) {
        for (int j = 0; j < 3; ++j) g[j] = pt[j];
    } else {
        for (int j = 0; j < 3; ++j) g[j] = (pt[j] - a0[j]) * (2.0f / (a1[j] - a0[j])) - 1.0f;
    }
    return isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]);
}

struct MsPixel {
    float ix, iy;        // clamped pixel coordinates along W and H
    bool inx, iny;       // strictly inside (0, size - 1): the coordinate gradient passes
};

// plane p reads components (0, 1), (0, 2), (1, 2); g is finite
__device__ __forceinline__ MsPixel ms_pixel(const float (&g)[3], int p, int H, int W)
{
    const float a = g[p == 2 ? 1 : 0], b = g[p == 0 ? 1 : 2];
    const float ux = (a + 1.0f) / 2.0f * (float)(W - 1), uy = (b + 1.0f) / 2.0f * (float)(H - 1);
    MsPixel q;
    q.ix = fminf((float)(W - 1), fmaxf(ux, 0.0f));
    q.iy = fminf((float)(H - 1), fmaxf(uy, 0.0f));
    q.inx = ux > 0.0f && ux < (float)(W - 1);
    q.iny = uy > 0.0f && uy < (float)(H - 1);
    return q;
}

// The four corners in grid_sample's order nw, ne, sw, se: row within the row space, -1 for the corner at index `size` (its weight is 0),
// and the weights as grid_sample forms them.  q lies in [0, size - 1], so the north-west corner always exists.
__device__ __forceinline__ void ms_corners(const MsPixel &q, uint32_t base, int H, int W, int (&t)[4], float (&w)[4])
{
    const float xw = floorf(q.ix), yn = floorf(q.iy), xe = xw + 1.0f, ys = yn + 1.0f;
    w[0] = (xe - q.ix) * (ys - q.iy);
    w[1] = (q.ix - xw) * (ys - q.iy);
    w[2] = (xe - q.ix) * (q.iy - yn);
    w[3] = (q.ix - xw) * (q.iy - yn);
    const int x0 = (int)xw, y0 = (int)yn;
    const bool e = x0 + 1 < W, s = y0 + 1 < H;
    const int r = (int)base + y0 * W + x0;
    t[0] = r;
    t[1] = e ? r + 1 : -1;
    t[2] = s ? r + W : -1;
    t[3] = e && s ? r + W + 1 : -1;
}

// ------------------------------------------------------------------ (C, H W) <-> (H W, C) of every plane, 32 x 32 tiles through LDS
// to_cl: planes[i] (C, HW) -> cl rows base[i].., quantised when asked; otherwise cl rows -> planes[i] (C, HW)
__global__ __launch_bounds__(TB) void k_msplane_transpose(MsPlanes P, MsGeom G, float *__restrict__ cl, int to_cl, int quantise)
{
    __shared__ float tile[32][33];
    const int i = blockIdx.y, C = G.C, HW = G.H[i] * G.W[i];
    const int tiles_c = (C + 31) >> 5, tiles_s = (HW + 31) >> 5;
    if ((int)blockIdx.x >= tiles_c * tiles_s) return;
    const int tc = blockIdx.x / tiles_s, ts = blockIdx.x - tc * tiles_s;
    float *plane = P.p[i];
    float *rows = cl + (int64_t)G.base[i] * C;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    if (to_cl) {
        for (int j = ly; j < 32; j += TB / 32) {
            const int c = tc * 32 + j, s = ts * 32 + lx;
            if (c < C && s < HW) {
                const float v = plane[(int64_t)c * HW + s];
                tile[j][lx] = quantise ? rintf(16.0f * v) / 16.0f : v;
            }
        }
        __syncthreads();
        for (int j = ly; j < 32; j += TB / 32) {
            const int s = ts * 32 + j, c = tc * 32 + lx;
            if (c < C && s < HW) rows[(int64_t)s * C + c] = tile[lx][j];
        }
    } else {
        for (int j = ly; j < 32; j += TB / 32) {
            const int s = ts * 32 + j, c = tc * 32 + lx;
            if (c < C && s < HW) tile[j][lx] = rows[(int64_t)s * C + c];
        }
        __syncthreads();
        for (int j = ly; j < 32; j += TB / 32) {
            const int c = tc * 32 + j, s = ts * 32 + lx;
            if (c < C && s < HW) plane[(int64_t)c * HW + s] = tile[lx][j];
        }
    }
}

void transpose_launch(hipStream_t st, const MsPlanes &P, const MsGeom &G, float *cl, int to_cl, int quantise)
{
    int64_t tiles = 0;
    for (int i = 0; i < 3 * G.L; ++i) tiles = std::max(tiles, cdiv(G.C, 32) * cdiv((int64_t)G.H[i] * G.W[i], 32));
    k_msplane_transpose<<<dim3((unsigned)tiles, 3 * G.L), TB, 0, st>>>(P, G, cl, to_cl, quantise);
}

// ------------------------------------------------------------------ forward
__device__ __forceinline__ void fma_to(float &v, float a, float w) { v = __builtin_fmaf(a, w, v); }
__device__ __forceinline__ void fma_to(float4 &v, const float4 &a, float w)
{
    v.x = __builtin_fmaf(a.x, w, v.x); v.y = __builtin_fmaf(a.y, w, v.y); v.z = __builtin_fmaf(a.z, w, v.z); v.w = __builtin_fmaf(a.w, w, v.w);
}
__device__ __forceinline__ float add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 add(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// The workgroup's output elements in order, T = float or float4 (C a multiple of 4: rows and output are 16-byte aligned): thread e is
// (point r, plane p, channel unit) and walks the levels with the running sum in registers.
template <class T>
__device__ __forceinline__ void ms_walk(const float *__restrict__ cl, const int4 *st, const float4 *sw, const MsGeom &G, int nr, float *__restrict__ o)
{
    constexpr int V = sizeof(T) / sizeof(float);
    const int L = G.L;
    const uint32_t CV = (uint32_t)G.C / V, C3 = 3 * CV, ne = (uint32_t)(nr * 3) * CV;    // in units of T
    const T *rows = reinterpret_cast<const T *>(cl);
    T *ov = reinterpret_cast<T *>(o);
    for (uint32_t e = threadIdx.x; e < ne; e += TB) {
        const uint32_t rp = CV == 1 ? e : __umulhi(e, G.magic), ch = e - rp * CV, r = rp / 3;
        T *oe = ov + (int64_t)r * (L - 1) * C3 + e;          // (r L + l) 3 C + p C + ch = r (L - 1) 3 C + e + l 3 C
        T f = {};
        for (int l = 0; l < L; ++l) {
            const int4 t = st[rp * L + l];
            const float4 w = sw[rp * L + l];
            T v = {};
            if (t.x >= 0) fma_to(v, rows[(int64_t)t.x * CV + ch], w.x);
            if (t.y >= 0) fma_to(v, rows[(int64_t)t.y * CV + ch], w.y);
            if (t.z >= 0) fma_to(v, rows[(int64_t)t.z * CV + ch], w.z);
            if (t.w >= 0) fma_to(v, rows[(int64_t)t.w * CV + ch], w.w);
            f = l == 0 ? v : add(v, f);                           // a level that is left out has no corners: v = 0 repeats F_{l-1}
            oe[(int64_t)l * C3] = f;
        }
    }
}

// workgroup b owns points [b PTS, (b + 1) PTS), PTS = MF_SLOTS / (3 L), and the L 3 C output elements of each
__global__ __launch_bounds__(TB) void k_msplane_fwd(const float *__restrict__ cl, const float *__restrict__ pts, MsXform X, MsGeom G, int64_t N,
                                                    float *__restrict__ out)
{
    __shared__ int4 st[MF_SLOTS];
    __shared__ float4 sw[MF_SLOTS];
    __shared__ float sg[MF_SLOTS / 3][4];
    const int L = G.L, PTS = MF_SLOTS / (3 * L);
    const int64_t r0 = (int64_t)blockIdx.x * PTS;
    const int nr = (int)min((int64_t)PTS, N - r0);
    for (int r = threadIdx.x; r < nr; r += TB) {
        float g[3];
        const bool ok = ms_grid_coord(pts + (r0 + r) * 3, G, X, g);
        sg[r][0] = g[0]; sg[r][1] = g[1]; sg[r][2] = g[2];
        sg[r][3] = ok ? 1.0f : 0.0f;
    }
    __syncthreads();
    // slot (r, p, l): the walk below reads a thread's L slots one after the other
    for (int u = threadIdx.x; u < nr * 3 * L; u += TB) {
        const int rp = u / L, l = u - rp * L, r = rp / 3, p = rp - 3 * r;
        int t[4] = {-1, -1, -1, -1};
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (sg[r][3] != 0.0f && level_used(G, l)) {
            const float g[3] = {sg[r][0], sg[r][1], sg[r][2]};
            const int i = l * 3 + p;
            ms_corners(ms_pixel(g, p, G.H[i], G.W[i]), G.base[i], G.H[i], G.W[i], t, w);
        }
        st[u] = make_int4(t[0], t[1], t[2], t[3]);
        sw[u] = make_float4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    float *o = out + r0 * L * (int64_t)(3 * G.C);
    if (G.vec == 4) ms_walk<float4>(cl, st, sw, G, nr, o);
    else ms_walk<float>(cl, st, sw, G, nr, o);
}

// ------------------------------------------------------------------ backward
// one thread per (point, level, plane) u = (n L + l) 3 + p: slots 4 u .. 4 u + 3
__global__ __launch_bounds__(TB) void k_msplane_keys(const float *__restrict__ pts, MsXform X, MsGeom G, int64_t U, uint32_t n_rows,
                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ slots, float *__restrict__ wts)
{
    const int64_t u = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (u >= U) return;
    const int64_t nl = u / 3, n = nl / G.L;
    const int p = (int)(u - 3 * nl), l = (int)(nl - n * G.L);
    int t[4] = {-1, -1, -1, -1};
    float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float g[3];
    if (level_used(G, l) && ms_grid_coord(pts + n * 3, G, X, g)) {
        const int i = l * 3 + p;
        ms_corners(ms_pixel(g, p, G.H[i], G.W[i]), G.base[i], G.H[i], G.W[i], t, w);
    }
    for (int c = 0; c < 4; ++c) {
        const int64_t s = u * 4 + c;
        keys[s] = t[c] >= 0 ? (uint32_t)t[c] : n_rows;
        slots[s] = (uint32_t)s;
        wts[s] = w[c];
    }
}

// the gradient reaching T_l[n, p, ch]: the grad_out blocks l' >= l of the point, added in ascending order; go -> block l of (n, p)
__device__ __forceinline__ float level_grad(const float *__restrict__ go, int l, int L, int64_t C3)
{
    float s = go[0];
    for (int k = l + 1; k < L; ++k) s += go[(int64_t)(k - l) * C3];
    return s;
}

// one lane = one channel of the wave's chunk
struct MsRowSum {
    const float *__restrict__ g;          // grad_out (N, L 3 C)
    const uint32_t *__restrict__ slots;
    const float *__restrict__ wts;
    float *__restrict__ grad_cl, *__restrict__ head, *__restrict__ tail;
    int C, L, ch;
    float acc;
    __device__ __forceinline__ void zero() { acc = 0.0f; }
    __device__ __forceinline__ void add(int64_t i)
    {
        const uint32_t s = slots[i], u = s >> 2, nl = u / 3, l = nl % (uint32_t)L;      // u = (n L + l) 3 + p: block l of (n, p) starts at u C
        acc = __builtin_fmaf(wts[s], level_grad(g + (int64_t)u * C + ch, (int)l, L, 3 * (int64_t)C), acc);
    }
    __device__ __forceinline__ void to_head(int64_t t) { head[t * C + ch] = acc; }
    __device__ __forceinline__ void to_tail(int64_t t) { tail[t * C + ch] = acc; }
    __device__ __forceinline__ void to_row(uint32_t row) { grad_cl[(int64_t)row * C + ch] = acc; }
};

// grad_cl is zeroed before: a row is written once, by the sum or by the combine pass
__global__ __launch_bounds__(TB) void k_msplane_bwd_sum(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slots, const float *__restrict__ wts,
                                                        const float *__restrict__ g, int C, int L, int64_t E, uint32_t n_rows,
                                                        float *__restrict__ grad_cl, float *__restrict__ head, float *__restrict__ tail,
                                                        uint8_t *__restrict__ own)
{
    const int64_t t = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    const int ch = blockIdx.y * 64 + (threadIdx.x & 63);
    if (t * MB_CHUNK >= E || ch >= C) return;
    MsRowSum a{g, slots, wts, grad_cl, head, tail, C, L, ch, 0.0f};
    sorted_chunk_sum<MB_CHUNK>(keys, t, E, n_rows, a, own);   // every lane of the chunk writes the same own[t]
}

__global__ __launch_bounds__(TB) void k_msplane_bwd_combine(const uint64_t *__restrict__ keys, int64_t E, int64_t nchunks, const float *__restrict__ head,
                                                            const float *__restrict__ tail, const uint8_t *__restrict__ own, int C,
                                                            float *__restrict__ grad_cl)
{
    const int64_t t = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    const int ch = blockIdx.y * 64 + (threadIdx.x & 63);
    if (ch >= C) return;
    sorted_combine<MB_CHUNK, 1, MB_WALK>(keys, E, nchunks, t, head + ch, tail + ch, C, own,
                                         [&](uint32_t row, const float (&s)[1]) { grad_cl[(int64_t)row * C + ch] = s[0]; });
}

// Coordinate gradient on the normalize_aabb path, one wave per point and one lane per channel (a wave's reads of the upstream gradient
// and of the corner rows are contiguous): d out / d pixel as grid_sample's backward forms it, zero along an axis whose pixel coordinate
// was clamped, through pixel = (g + 1) / 2 (size - 1) per lane, the lanes added in a fixed butterfly, then through
// g = (pts - aabb[0]) (2 / (aabb[1] - aabb[0])) - 1.  A point whose g is not finite gets 0, whatever the aabb.
__global__ __launch_bounds__(TB) void k_msplane_bwd_pts(const float *__restrict__ cl, const float *__restrict__ pts, MsXform X, MsGeom G, int64_t N,
                                                        const float *__restrict__ go, float *__restrict__ grad_pts)
{
    const int64_t n = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (n >= N) return;                                       // the whole wave
    const int lane = threadIdx.x & 63, C = G.C, L = G.L;
    const int64_t C3 = 3 * (int64_t)C;
    float gg[3] = {0.0f, 0.0f, 0.0f}, g[3];
    const bool ok = ms_grid_coord(pts + n * 3, G, X, g);      // the same in every lane
    if (ok) {
        for (int l = 0; l < L; ++l) {
            if (!level_used(G, l)) continue;
            for (int p = 0; p < 3; ++p) {
                const int i = l * 3 + p, H = G.H[i], W = G.W[i];
                const MsPixel q = ms_pixel(g, p, H, W);
                int t[4];
                float w[4];
                ms_corners(q, G.base[i], H, W, t, w);
                const float xw = floorf(q.ix), yn = floorf(q.iy);
                const float dxe = (xw + 1.0f) - q.ix, dxw = q.ix - xw, dys = (yn + 1.0f) - q.iy, dyn = q.iy - yn;
                const float *gb = go + (n * L + l) * C3 + (int64_t)p * C;
                float gix = 0.0f, giy = 0.0f;
                for (int ch = lane; ch < C; ch += 64) {
                    const float gv = level_grad(gb + ch, l, L, C3);
                    const float nw = cl[(int64_t)t[0] * C + ch], ne = t[1] >= 0 ? cl[(int64_t)t[1] * C + ch] : 0.0f;
                    const float sw = t[2] >= 0 ? cl[(int64_t)t[2] * C + ch] : 0.0f, se = t[3] >= 0 ? cl[(int64_t)t[3] * C + ch] : 0.0f;
                    gix = __builtin_fmaf((ne - nw) * dys + (se - sw) * dyn, gv, gix);
                    giy = __builtin_fmaf((sw - nw) * dxe + (se - ne) * dxw, gv, giy);
                }
                if (q.inx) gg[p == 2 ? 1 : 0] += gix * ((float)(W - 1) / 2.0f);
                if (q.iny) gg[p == 0 ? 1 : 2] += giy * ((float)(H - 1) / 2.0f);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; ++d) gg[d] += __shfl_xor(gg[d], off, 64);
    if (lane < 3) {
        const float v = lane == 0 ? gg[0] : (lane == 1 ? gg[1] : gg[2]);
        grad_pts[n * 3 + lane] = !ok ? 0.0f : (G.contract == 3 ? v : v * (2.0f / (X.aabb[3 + lane] - X.aabb[lane])));
    }
}

int check_args(const char *who, int64_t n, int n_levels, int C, const int *heights, const int *widths, int level, MsGeom &G)
{
    if (n < 0) return fail(GPCC_ERR_ARG, "%s: n = %lld", who, (long long)n);
    if (n_levels < 1 || n_levels > MAX_LEVELS) return fail(GPCC_ERR_ARG, "%s: %d levels outside [1, %d]", who, n_levels, MAX_LEVELS);
    if (C < 1 || C > MAX_C) return fail(GPCC_ERR_ARG, "%s: %d channels outside [1, %d]", who, C, MAX_C);
    if (!heights || !widths) return fail(GPCC_ERR_ARG, "%s: null plane sizes", who);
    if (n * 3 * n_levels * 4 >= ((int64_t)1 << 32))
        return fail(GPCC_ERR_ARG, "%s: %lld points x %d levels: more than 2^32 (point, level, plane, corner) slots", who, (long long)n, n_levels);
    G.C = C; G.L = n_levels; G.level = level;
    G.vec = 1;
    G.magic = (uint32_t)((((uint64_t)1 << 32) / (uint64_t)C) + 1);   // unused for C = 1
    uint32_t rows = 0;
    for (int i = 0; i < 3 * n_levels; ++i) {
        const int H = heights[i], W = widths[i];
        if (H < 2 || H > MAX_SIZE || W < 2 || W > MAX_SIZE) return fail(GPCC_ERR_ARG, "%s: plane %d of %d x %d outside [2, %d]", who, i, H, W, MAX_SIZE);
        G.H[i] = H; G.W[i] = W; G.base[i] = rows;
        rows += (uint32_t)(H * W);                                    // at most 24 x 2^24 rows
    }
    for (int i = 3 * n_levels; i < MAX_PLANES; ++i) { G.H[i] = G.W[i] = 0; G.base[i] = rows; }
    G.base[MAX_PLANES] = rows;
    return GPCC_OK;
}

// contract: 0 normalize_aabb, 1 the whole transform, 2 con_normalize_aabb alone, 3 none
bool bad_xform(int contract, const float *pca_mean, const float *rotation, const float *variance, const float *aabb, const float *con_aabb)
{
    if (contract < 0 || contract > 3) return true;
    if (contract != 3 && !aabb) return true;
    if ((contract == 1 || contract == 2) && !con_aabb) return true;
    return contract == 1 && (!pca_mean || !rotation || !variance);
}

}  // namespace

extern "C" int gsge_msplane_forward(gpcc_ctx *ctx, const float *pts, int64_t n, int n_levels, const float *const *planes, int channels,
                                    const int *heights, const int *widths, int level, int quantise, int contract, const float *pca_mean,
                                    const float *rotation, const float *variance, const float *aabb, const float *con_aabb, float *out,
                                    gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    const char *who = "gsge_msplane_forward";
    if (!ctx) return fail(GPCC_ERR_ARG, "%s: null context", who);
    MsGeom G;
    GP_TRY(check_args(who, n, n_levels, channels, heights, widths, level, G));
    G.contract = contract;
    if (n == 0) return GPCC_OK;
    if (!pts || !planes || !out || !alloc || bad_xform(contract, pca_mean, rotation, variance, aabb, con_aabb))
        return fail(GPCC_ERR_ARG, "%s: null argument or contract = %d", who, contract);
    MsPlanes P = {};
    for (int i = 0; i < 3 * n_levels; ++i) {
        if (!planes[i]) return fail(GPCC_ERR_ARG, "%s: plane %d is null", who, i);
        P.p[i] = const_cast<float *>(planes[i]);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const MsXform X{pca_mean, rotation, variance, aabb, con_aabb};
    float *cl;
    GP_TRY(caller_alloc(alloc, alloc_user, (size_t)G.base[MAX_PLANES] * channels * sizeof(float), &cl, who));
    if (channels % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(cl) & 15) == 0) {
        G.vec = 4;
        G.magic = (uint32_t)((((uint64_t)1 << 32) / (uint64_t)(channels / 4)) + 1);
    }
    transpose_launch(st, P, G, cl, 1, quantise != 0);
    LAUNCH_CHECK();
    k_msplane_fwd<<<(unsigned)cdiv(n, MF_SLOTS / (3 * n_levels)), TB, 0, st>>>(cl, pts, X, G, n, out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsge_msplane_backward(gpcc_ctx *ctx, const float *grad_out, const float *pts, int64_t n, int n_levels, const float *const *planes,
                                     int channels, const int *heights, const int *widths, int level, int quantise, int contract,
                                     const float *pca_mean, const float *rotation, const float *variance, const float *aabb, const float *con_aabb,
                                     float *const *grad_planes, float *grad_pts, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    const char *who = "gsge_msplane_backward";
    if (!ctx) return fail(GPCC_ERR_ARG, "%s: null context", who);
    MsGeom G;
    GP_TRY(check_args(who, n, n_levels, channels, heights, widths, level, G));
    G.contract = contract;
    if (grad_pts && (contract == 1 || contract == 2)) return fail(GPCC_ERR_ARG, "%s: no coordinate gradient with contract (the reference detaches the points)", who);
    if (!grad_planes || !alloc) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    MsPlanes GP = {}, P = {};
    for (int i = 0; i < 3 * n_levels; ++i) {
        if (!grad_planes[i]) return fail(GPCC_ERR_ARG, "%s: gradient of plane %d is null", who, i);
        GP.p[i] = grad_planes[i];
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int C = channels;
    if (n == 0) {
        for (int i = 0; i < 3 * n_levels; ++i) HIP_TRY(hipMemsetAsync(GP.p[i], 0, (size_t)G.H[i] * G.W[i] * C * sizeof(float), st));
        return GPCC_OK;
    }
    if (!grad_out || !pts || bad_xform(contract, pca_mean, rotation, variance, aabb, con_aabb)) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    if (grad_pts) {
        if (!planes) return fail(GPCC_ERR_ARG, "%s: null argument", who);
        for (int i = 0; i < 3 * n_levels; ++i) {
            if (!planes[i]) return fail(GPCC_ERR_ARG, "%s: plane %d is null", who, i);
            P.p[i] = const_cast<float *>(planes[i]);
        }
    }
    const MsXform X{pca_mean, rotation, variance, aabb, con_aabb};
    const uint32_t n_rows = G.base[MAX_PLANES];
    const int64_t U = n * n_levels * 3, E = U * 4, nchunks = cdiv(E, MB_CHUNK), cl_floats = (int64_t)n_rows * C;
    uint64_t *ka, *kb;
    uint32_t *va, *vb, *hist;
    float *wts, *head, *tail, *grad_cl, *cl = nullptr;
    uint8_t *own;
    GP_TRY(caller_block(alloc, alloc_user, who, [&](Carver &c) {
        ka = c.take<uint64_t>(E); kb = c.take<uint64_t>(E); va = c.take<uint32_t>(E); vb = c.take<uint32_t>(E); wts = c.take<float>(E);
        hist = c.take<uint32_t>(radix_sort_hist_words(E)); head = c.take<float>(nchunks * C); tail = c.take<float>(nchunks * C);
        own = c.take<uint8_t>(nchunks); grad_cl = c.take<float>(cl_floats);
        if (grad_pts) cl = c.take<float>(cl_floats);
    }));
    k_msplane_keys<<<(unsigned)cdiv(U, TB), TB, 0, st>>>(pts, X, G, U, n_rows, ka, va, wts);
    LAUNCH_CHECK();
    int bits = 1;
    while (((int64_t)1 << bits) <= (int64_t)n_rows) ++bits;    // the sentinel n_rows sorts last
    uint64_t *k0 = ka, *k1 = kb;
    uint32_t *v0 = va, *v1 = vb;
    GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, E, bits, hist));
    HIP_TRY(hipMemsetAsync(grad_cl, 0, (size_t)cl_floats * sizeof(float), st));
    const dim3 grid((unsigned)cdiv(nchunks, TB / 64), (unsigned)cdiv(C, 64));
    k_msplane_bwd_sum<<<grid, TB, 0, st>>>(k0, v0, wts, grad_out, C, n_levels, E, n_rows, grad_cl, head, tail, own);
    LAUNCH_CHECK();
    k_msplane_bwd_combine<<<grid, TB, 0, st>>>(k0, E, nchunks, head, tail, own, C, grad_cl);
    LAUNCH_CHECK();
    transpose_launch(st, GP, G, grad_cl, 0, 0);
    LAUNCH_CHECK();
    if (grad_pts) {
        transpose_launch(st, P, G, cl, 1, quantise != 0);
        LAUNCH_CHECK();
        k_msplane_bwd_pts<<<(unsigned)cdiv(n, TB / 64), TB, 0, st>>>(cl, pts, X, G, n, grad_out, grad_pts);
        LAUNCH_CHECK();
    }
    return GPCC_OK;
}
