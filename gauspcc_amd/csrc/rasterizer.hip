// rasterizer.hip -- the tile-binned Gaussian splat rasteriser: forward, visible_filter, and the training path (forward + backward)
// (diff-gaussian-rasterization, Scaffold-GS fork; the zip is missing from the reference tree, see
// SURVEY.md App. E; call contract: HAC/gaussian_renderer/__init__.py:199-225, 268-303 and
// TC-GS/SIBR_viewers/src/projects/gaussianviewer/renderer/GaussianView.cpp:535-553, 660-688).
// The inference forward (RD evaluation: render -> PSNR) is gsr_forward; training runs gsr_forward_train + gsr_backward (k_render<true>,
// k_render_backward, k_preprocess_backward: below the forward's kernels).  The _aux forms of the three add the frame's inverse-depth and
// accumulated-opacity maps and their gradients (the AUX instantiations); with no map asked for they are the three, kernel for kernel.
//
// gfx950 mapping:
//   k_preprocess     one lane per Gaussian, coalesced SoA outputs (HBM-bound); counts the tiles the splat can reach (tile_touches: exact tile culling)
//   scan / sort      the library's own wave-ballot radix sort: the Gaussians by depth (4 passes), the duplicates emitted in that order, then by tile (2 passes)
//                    -- the permutation of the reference's single sort on (tile << 32 | depth bits), which GAUSPCC_RASTER_SORT2=0 still runs
//   k_tile_ranges    boundary detection on the sorted keys
//   k_render         one 128-lane workgroup per 16x16 tile, two pixels per lane; batches of 128 Gaussians staged in LDS
//                    (id -> xy, conic+opacity, rgb = 36 B each), every lane blends its pixels front to
//                    back and the workgroup leaves when all 256 pixels are saturated
#include "primitives.hpp"

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int BX = 16, BY = 16;

struct Cam {
    const float *view, *proj;   // the caller's 4 x 4 matrices, read where they lie (device memory): no blocking copies to the host in front of a frame
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
    int W, H, gx, gy;
};

__device__ __forceinline__ float ndc2pix(float v, int S) { return ((v + 1.0f) * (float)S - 1.0f) * 0.5f; }

// Exact tile culling (round 5).  The reference bins a Gaussian into every tile of the 3-sigma bounding square of its larger axis; the blend then
// skips it at every pixel where alpha = op exp(power) < 1 / 255.  A pair (Gaussian, tile) whose `power` stays below -ln(255 op) over the whole
// tile is therefore dead weight in the sort and in the tile's list -- about a third of all pairs (corners of the squares, thin or faint splats).
// q(d) = -power(d) = 0.5 (A dx^2 + C dy^2) + B dx dy is convex with its minimum 0 at the centre, so its minimum over the tile's rectangle of
// pixel centres is 0 when the centre lies inside and is attained on one of the four edges otherwise (a 1-D quadratic each, clamped).  The pair is
// kept when that minimum <= ln(255 op) + margin; the margin leaves every borderline pixel to the exact test in the blend, so the image is
// bit-identical with and without culling (tests/test_gpu_rasterizer.py) and only the lists get shorter.  The margin has an absolute part (2e-3,
// twice k_render's own pre-test) and, since round 6, a part that SCALES WITH THE TERMS: for a long thin splat far from its centre each of the
// three terms of q is ~1e6 and they cancel down to q ~ 5, so the fp32 edge minimum here and the per-pixel power of k_render (another order of
// the same operations) may differ by several ulp of 1e6 -- far more than 2e-3.  8 eps x (|term| summed) bounds both sides' error.
__device__ __forceinline__ float edge_min(float c, float lo, float hi, float Ac, float Bm, float Cv, float inv_Cv)
{   // min over v in [lo, hi] of 0.5 Ac c^2 + Bm c v + 0.5 Cv v^2, less the rounding slack of its evaluation (Ac, Cv > 0).  The minimiser through the
    // reciprocal the caller computed once per Gaussian (four correctly rounded divisions per tile were 40 of this test's ~90 instructions): any v in
    // [lo, hi] gives a value >= the minimum, and an error of an ulp in v moves the value by its square
    const float v = fminf(hi, fmaxf(lo, -Bm * c * inv_Cv));
    const float t0 = 0.5f * Ac * c * c, t1 = Bm * c * v, t2 = 0.5f * Cv * v * v;
    return (t0 + t1 + t2) - 9.6e-7f * (t0 + fabsf(t1) + t2);
}
__device__ __forceinline__ bool tile_touches(float gx_, float gy_, float A, float B, float C, float inv_A, float inv_C, float lim, int tx, int ty)
{
    // d = centre - pixel, pixels tx*16 .. tx*16 + 15 (the last tiles' pixels beyond the image only make the rectangle larger)
    const float dx_hi = gx_ - (float)(tx * BX), dx_lo = dx_hi - (float)(BX - 1);
    const float dy_hi = gy_ - (float)(ty * BY), dy_lo = dy_hi - (float)(BY - 1);
    if (!(lim < __builtin_inff())) return true;     // conics outside the argument (cull_limit): the reference's lists
    if (dx_lo <= 0.0f && dx_hi >= 0.0f && dy_lo <= 0.0f && dy_hi >= 0.0f) return true;
    const float m = fminf(fminf(edge_min(dx_lo, dy_lo, dy_hi, A, B, C, inv_C), edge_min(dx_hi, dy_lo, dy_hi, A, B, C, inv_C)),
                          fminf(edge_min(dy_lo, dx_lo, dx_hi, C, B, A, inv_A), edge_min(dy_hi, dx_lo, dx_hi, C, B, A, inv_A)));
    return !(m > lim);                              // (a NaN anywhere keeps the pair)
}
// the bound on q for a Gaussian of opacity op: +inf for conics the argument above does not cover (never culled), -1 when op < 1 / 255 (never blended)
__device__ __forceinline__ float cull_limit(float A, float B, float C, float op)
{
    if (!(A > 0.0f && C > 0.0f && A * C - B * B > 0.0f)) return __builtin_inff();
    if (op != op) return __builtin_inff();          // a NaN opacity blends as alpha 0.99 (fminf): keep the pair
    if (!(op > 0.0f)) return -1.0f;
    return __logf(255.0f * op) + 2e-3f;
}

constexpr uint32_t REC_BIG = 0x80000000u;
constexpr int RECT_SLOTS = 256;

// One Gaussian of k_preprocess.  Returns the tile count of its bounding square when culling (what the reference calls num_rendered is their sum), else 0;
// *dbits: the depth's bit pattern of a visible Gaussian (visible depths are positive: the patterns order as the values do), 0xFFFFFFFF otherwise.
__device__ __forceinline__ uint32_t preprocess_one(int i, const float *__restrict__ means, const float *__restrict__ scales, const float *__restrict__ rots,
                                                   const float *__restrict__ cov3d_pre, const float *__restrict__ opac, const Cam &cam, int *__restrict__ radii,
                                                   float2 *__restrict__ xy, float *__restrict__ depth, float4 *__restrict__ conic_op,
                                                   uint32_t *__restrict__ tiles_touched, int cull, uint32_t *dbits, uint32_t *cnt_out, uint4 *rec)
{
    radii[i] = 0;
    if (tiles_touched) tiles_touched[i] = 0;
    const float px = means[3 * i], py = means[3 * i + 1], pz = means[3 * i + 2];
    const float *__restrict__ V = cam.view, *__restrict__ M = cam.proj;   // wave-uniform addresses: scalar / broadcast loads
    // transformPoint4x3 / 4x4 with the row-vector (transposed) matrices the Python side passes
    const float tx0 = V[0] * px + V[4] * py + V[8] * pz + V[12];
    const float ty0 = V[1] * px + V[5] * py + V[9] * pz + V[13];
    const float tz = V[2] * px + V[6] * py + V[10] * pz + V[14];
    if (tz <= 0.2f) return 0;  // in_frustum
    const float hx = M[0] * px + M[4] * py + M[8] * pz + M[12];
    const float hy = M[1] * px + M[5] * py + M[9] * pz + M[13];
    const float hw = M[3] * px + M[7] * py + M[11] * pz + M[15];
    const float pw = 1.0f / (hw + 0.0000001f);
    const float prx = hx * pw, pry = hy * pw;
    // 3-D covariance (upper triangle)
    float c[6];
    if (cov3d_pre) {
        for (int k = 0; k < 6; ++k) c[k] = cov3d_pre[6 * i + k];
    } else {
        const float sx = cam.scale_modifier * scales[3 * i], sy = cam.scale_modifier * scales[3 * i + 1], sz = cam.scale_modifier * scales[3 * i + 2];
        const float r = rots[4 * i], x = rots[4 * i + 1], y = rots[4 * i + 2], z = rots[4 * i + 3];
        // R (row-major) from the quaternion (r, x, y, z); M = S * R; Sigma = M^T M
        const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
        const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
        const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
        // Sigma = R diag(s^2) R^T  (== M^T M with glm's column-major M = S * R)
        const float ax = sx * sx, ay = sy * sy, az = sz * sz;
        c[0] = ax * R00 * R00 + ay * R01 * R01 + az * R02 * R02;
        c[1] = ax * R00 * R10 + ay * R01 * R11 + az * R02 * R12;
        c[2] = ax * R00 * R20 + ay * R01 * R21 + az * R02 * R22;
        c[3] = ax * R10 * R10 + ay * R11 * R11 + az * R12 * R12;
        c[4] = ax * R10 * R20 + ay * R11 * R21 + az * R12 * R22;
        c[5] = ax * R20 * R20 + ay * R21 * R21 + az * R22 * R22;
    }
    // 2-D covariance: A Sigma A^T, A = J * Rwc, with the +-1.3 tan(fov) clamp of the view-space position
    const float limx = 1.3f * cam.tan_fovx, limy = 1.3f * cam.tan_fovy;
    const float tx = fminf(limx, fmaxf(-limx, tx0 / tz)) * tz;
    const float ty = fminf(limy, fmaxf(-limy, ty0 / tz)) * tz;
    const float j00 = cam.focal_x / tz, j02 = -(cam.focal_x * tx) / (tz * tz);
    const float j11 = cam.focal_y / tz, j12 = -(cam.focal_y * ty) / (tz * tz);
    const float a0x = j00 * V[0] + j02 * V[2], a0y = j00 * V[4] + j02 * V[6], a0z = j00 * V[8] + j02 * V[10];
    const float a1x = j11 * V[1] + j12 * V[2], a1y = j11 * V[5] + j12 * V[6], a1z = j11 * V[9] + j12 * V[10];
    const float s0x = c[0] * a0x + c[1] * a0y + c[2] * a0z, s0y = c[1] * a0x + c[3] * a0y + c[4] * a0z, s0z = c[2] * a0x + c[4] * a0y + c[5] * a0z;
    const float s1x = c[0] * a1x + c[1] * a1y + c[2] * a1z, s1y = c[1] * a1x + c[3] * a1y + c[4] * a1z, s1z = c[2] * a1x + c[4] * a1y + c[5] * a1z;
    const float cxx = a0x * s0x + a0y * s0y + a0z * s0z + 0.3f;
    const float cxy = a0x * s1x + a0y * s1y + a0z * s1z;
    const float cyy = a1x * s1x + a1y * s1y + a1z * s1z + 0.3f;
    const float det = cxx * cyy - cxy * cxy;
    if (det == 0.0f) return 0;
    const float det_inv = 1.0f / det;
    const float mid = 0.5f * (cxx + cyy);
    const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    const float my_radius = ceilf(3.0f * sqrtf(lam));  // lambda1 >= lambda2
    const float ix = ndc2pix(prx, cam.W), iy = ndc2pix(pry, cam.H);
    const int rx0 = min(cam.gx, max(0, (int)((ix - my_radius) / BX))), ry0 = min(cam.gy, max(0, (int)((iy - my_radius) / BY)));
    const int rx1 = min(cam.gx, max(0, (int)((ix + my_radius + BX - 1) / BX))), ry1 = min(cam.gy, max(0, (int)((iy + my_radius + BY - 1) / BY)));
    const int area = (rx1 - rx0) * (ry1 - ry0);
    if (area == 0) return 0;
    radii[i] = (int)my_radius;
    if ((int)my_radius > 0) *dbits = __float_as_uint(tz);
    if (!tiles_touched) return 0;
    const float4 co = make_float4(cyy * det_inv, -cxy * det_inv, cxx * det_inv, opac[i]);
    uint32_t cnt = (uint32_t)area;
    const int w = rx1 - rx0;
    uint64_t m = area >= 64 ? ~0ull : (1ull << area) - 1ull;   // bit (y - ry0) * w + (x - rx0): the tiles of the square that take the Gaussian
    if (cull) {
        const float lim = cull_limit(co.x, co.y, co.z, co.w);
        const float inv_a = 1.0f / co.x, inv_c = 1.0f / co.z;       // (used only when lim is finite: co.x, co.z > 0 then)
        cnt = 0; m = 0;
        int b = 0;
        for (int y = ry0; y < ry1; ++y)
            for (int x = rx0; x < rx1; ++x, ++b)
                if (tile_touches(ix, iy, co.x, co.y, co.z, inv_a, inv_c, lim, x, y)) { ++cnt; m |= 1ull << (b & 63); }
    }
    tiles_touched[i] = cnt;
    *cnt_out = cnt;
    *rec = make_uint4((uint32_t)m, (uint32_t)(m >> 32), (uint32_t)rx0 | ((uint32_t)ry0 << 16), area > 64 ? REC_BIG : (uint32_t)w);
    xy[i] = make_float2(ix, iy);
    depth[i] = tz;
    conic_op[i] = co;
    return cull ? (uint32_t)area : 0u;
}

// dkeys / dvals / recs (optional, together): the (depth, index) pairs of the two-level sort's first level, written here instead of by a pass of their
// own.  The key's upper word carries the Gaussian's tile count (the sort looks at the lower 32 bits only and moves whole keys), so the counts come out
// of the sort in depth order; recs[i] is what k_duplicate_sorted needs of Gaussian i in ONE 16-byte gather: the square's origin and width and the
// mask of its tiles that take the Gaussian (squares of more than 64 tiles: REC_BIG, that kernel walks the square again).
// rect_total (optional, zeroed by the caller): one atomic add per wave of the bounding squares' tile counts.
__global__ __launch_bounds__(TB) void k_preprocess(int P, const float *__restrict__ means, const float *__restrict__ scales, const float *__restrict__ rots,
                                                   const float *__restrict__ cov3d_pre, const float *__restrict__ opac, Cam cam, int *__restrict__ radii,
                                                   float2 *__restrict__ xy, float *__restrict__ depth, float4 *__restrict__ conic_op,
                                                   uint32_t *__restrict__ tiles_touched, int cull, unsigned long long *__restrict__ rect_total,
                                                   uint64_t *__restrict__ dkeys, uint32_t *__restrict__ dvals, uint4 *__restrict__ recs)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    uint32_t dbits = 0xFFFFFFFFu, area = 0, cnt = 0;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (i < P) {
        area = preprocess_one(i, means, scales, rots, cov3d_pre, opac, cam, radii, xy, depth, conic_op, tiles_touched, cull, &dbits, &cnt, &rec);
        if (dkeys) { dkeys[i] = ((uint64_t)cnt << 32) | dbits; dvals[i] = (uint32_t)i; recs[i] = rec; }
    }
    if (rect_total) {   // RECT_SLOTS partial sums: 73 k wave atomics on ONE address serialise at ~10 ns each (0.7 ms at 4.66 M Gaussians, measured)
        for (int d = 32; d; d >>= 1) area += __shfl_xor(area, d);
        if ((threadIdx.x & 63) == 0 && area) atomicAdd(rect_total + ((blockIdx.x * (TB / 64) + (threadIdx.x >> 6)) & (RECT_SLOTS - 1)), (unsigned long long)area);
    }
}

__global__ __launch_bounds__(RECT_SLOTS) void k_sum_slots(const unsigned long long *__restrict__ slots, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long part[RECT_SLOTS / 64];
    unsigned long long acc = slots[threadIdx.x];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < RECT_SLOTS / 64; ++k) t += part[k];
        *total = t;
    }
}

__global__ __launch_bounds__(TB) void k_duplicate(int P, const float2 *__restrict__ xy, const float *__restrict__ depth, const uint32_t *__restrict__ offs,
                                                  const int *__restrict__ radii, int gx, int gy, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                  const float4 *__restrict__ conic_op, int cull)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= P || radii[i] <= 0) return;
    uint32_t off = offs[i];
    const float r = (float)radii[i];
    const float2 p = xy[i];
    const int rx0 = min(gx, max(0, (int)((p.x - r) / BX))), ry0 = min(gy, max(0, (int)((p.y - r) / BY)));
    const int rx1 = min(gx, max(0, (int)((p.x + r + BX - 1) / BX))), ry1 = min(gy, max(0, (int)((p.y + r + BY - 1) / BY)));
    const uint32_t dbits = __float_as_uint(depth[i]);
    const float4 co = conic_op[i];
    const float lim = cull ? cull_limit(co.x, co.y, co.z, co.w) : 0.0f;
    const float inv_a = 1.0f / co.x, inv_c = 1.0f / co.z;       // as in k_preprocess: the count there and the pairs here come from the same test
    for (int y = ry0; y < ry1; ++y)
        for (int x = rx0; x < rx1; ++x) {
            if (cull && !tile_touches(p.x, p.y, co.x, co.y, co.z, inv_a, inv_c, lim, x, y)) continue;
            keys[off] = ((uint64_t)(uint32_t)(y * gx + x) << 32) | dbits;
            vals[off] = (uint32_t)i;
            ++off;
        }
}

// Two-level form of the (tile | depth) sort (round 5).  The reference sorts the L duplicated (tile << 32 | depth) keys in one radix sort
// (six 8-bit passes over 18 M pairs at 1 M anchors: the largest part of a frame).  A stable sort by depth of the P Gaussians (four passes over
// 5.4 M), the duplicates emitted in THAT order, and a stable sort of the duplicates by tile alone (two passes) give the same permutation:
// within a tile, depth ascending, equal depths in Gaussian order -- exactly what the stable sort of the combined key produces.  (The first
// level's (depth, index) pairs come out of k_preprocess.)
__global__ __launch_bounds__(TB) void k_sorted_counts(int P, const uint64_t *__restrict__ keys, uint32_t *__restrict__ out)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < P) out[i] = (uint32_t)(keys[i] >> 32);
}

__global__ __launch_bounds__(TB) void k_duplicate_sorted(int P, const uint32_t *__restrict__ perm, const uint4 *__restrict__ recs, const float2 *__restrict__ xy,
                                                         const uint32_t *__restrict__ offs, const int *__restrict__ radii, int gx, int gy, uint64_t *__restrict__ keys,
                                                         uint32_t *__restrict__ vals, const float4 *__restrict__ conic_op, int cull)
{
    const int s = blockIdx.x * TB + threadIdx.x;
    if (s >= P) return;
    const uint32_t i = perm[s];
    const uint4 rec = recs[i];
    uint32_t off = offs[s];
    if (!(rec.w & REC_BIG)) {     // invisible Gaussians have an empty mask
        uint64_t m = (uint64_t)rec.x | ((uint64_t)rec.y << 32);
        const uint32_t w = rec.w;
        const uint64_t row_mask = w >= 64u ? ~0ull : (1ull << w) - 1ull;
        for (uint32_t row = (rec.z >> 16) * (uint32_t)gx + (rec.z & 0xFFFFu); m; m = w >= 64u ? 0ull : m >> w, row += (uint32_t)gx)
            for (uint64_t bits = m & row_mask; bits; bits &= bits - 1ull) {
                keys[off] = (uint64_t)(row + (uint32_t)__builtin_ctzll(bits));
                vals[off] = i;
                ++off;
            }
        return;
    }
    const float r = (float)radii[i];
    const float2 p = xy[i];
    const int rx0 = min(gx, max(0, (int)((p.x - r) / BX))), ry0 = min(gy, max(0, (int)((p.y - r) / BY)));
    const int rx1 = min(gx, max(0, (int)((p.x + r + BX - 1) / BX))), ry1 = min(gy, max(0, (int)((p.y + r + BY - 1) / BY)));
    const float4 co = conic_op[i];
    const float lim = cull ? cull_limit(co.x, co.y, co.z, co.w) : 0.0f;
    const float inv_a = 1.0f / co.x, inv_c = 1.0f / co.z;       // as in k_preprocess: the count there and the pairs here come from the same test
    for (int y = ry0; y < ry1; ++y)
        for (int x = rx0; x < rx1; ++x) {
            if (cull && !tile_touches(p.x, p.y, co.x, co.y, co.z, inv_a, inv_c, lim, x, y)) continue;
            keys[off] = (uint64_t)(uint32_t)(y * gx + x);
            vals[off] = i;
            ++off;
        }
}

__global__ __launch_bounds__(TB) void k_tile_ranges(int L, const uint64_t *__restrict__ keys, int shift, uint2 *__restrict__ ranges)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= L) return;
    const uint32_t t = (uint32_t)(keys[i] >> shift);
    if (i == 0) ranges[t].x = 0;
    else {
        const uint32_t pt = (uint32_t)(keys[i - 1] >> shift);
        if (t != pt) { ranges[pt].y = (uint32_t)i; ranges[t].x = (uint32_t)i; }
    }
    if (i == L - 1) ranges[t].y = (uint32_t)L;
}

// One 16 x 16 tile per workgroup of RT = 128 lanes (two waves); a lane blends TWO pixels, (x, y) and (x, y + 8): one fetch of a
// Gaussian from LDS (three broadcast reads) and one pass of the loop's control feed two blends.  The blend is predicated instead of
// three data-dependent `continue`s (no exec-mask juggling), the exponential is one v_exp_f32 on power * log2(e) -- `power` itself is the
// reference's expression, so its sign test is the reference's --, and a wave leaves a batch as soon as all its pixels are saturated.
// Round 4 measured the one-pixel-per-lane form at 36 % of the VALU peak (three LDS waits, a libm exponential and three branches for ~15
// useful VALU instructions per Gaussian and pixel: profiles/r04_render_counters.txt).
constexpr int RT = 128;
// AUX: one more blended channel, the Gaussian's inverse view depth d into D (the invdepth map; alpha comes from the final T)
template <bool AUX>
__device__ __forceinline__ void blend_one(float power, float op, float r, float g, float b, bool &done, float &T, float &C0, float &C1, float &C2, float d, float &D)
{
    const float e = __builtin_amdgcn_exp2f(power * 1.44269504088896341f);
    const float alpha = fminf(0.99f, op * e);
    const bool ok = !done && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
    const float tt = T * (1.0f - alpha);
    const bool sat = ok && tt < 0.0001f;
    done = done || sat;
    const bool upd = ok && !sat;
    const float w = upd ? alpha * T : 0.0f;
    C0 += r * w; C1 += g * w; C2 += b * w;
    if constexpr (AUX) D += d * w;
    T = upd ? tt : T;
}
// the same blend, plus the list position after the last Gaussian blended into the pixel (the training forward)
template <bool AUX>
__device__ __forceinline__ void blend_one_rec(float power, float op, float r, float g, float b, bool &done, float &T, float &C0, float &C1, float &C2,
                                              uint32_t kend, uint32_t &e, float d, float &D)
{
    const float e2 = __builtin_amdgcn_exp2f(power * 1.44269504088896341f);
    const float alpha = fminf(0.99f, op * e2);
    const bool ok = !done && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
    const float tt = T * (1.0f - alpha);
    const bool sat = ok && tt < 0.0001f;
    done = done || sat;
    const bool upd = ok && !sat;
    const float w = upd ? alpha * T : 0.0f;
    C0 += r * w; C1 += g * w; C2 += b * w;
    if constexpr (AUX) D += d * w;
    T = upd ? tt : T;
    e = upd ? kend : e;
}

// dispatch order of the tiles: longest list first (the lists of a frame differ by two orders of magnitude; a long tile that starts last is the
// frame's tail).  The order is a schedule, not a result: lengths in steps of 64 entries, saturating at 16 k, make it ONE radix pass (20-bit keys: three).
__global__ __launch_bounds__(TB) void k_tile_order_keys(const uint2 *__restrict__ ranges, int ntiles, uint64_t *__restrict__ key, uint32_t *__restrict__ idx)
{
    const int t = blockIdx.x * TB + threadIdx.x;
    if (t >= ntiles) return;
    const uint32_t c = ranges[t].y - ranges[t].x;
    key[t] = 255ull - (uint64_t)min(c >> 6, 255u);
    idx[t] = (uint32_t)t;
}

// TRAIN (the training forward, gsr_forward_train): point_list holds the pair's SLOT (its position in the duplicate pass's output, see
// k_render_backward) and the Gaussian is gathered through slot_ids; every in-image pixel leaves its final T and the list position after the last
// Gaussian it blended (0: none).  The blend is the same code: the image is bit-identical to the inference path's.
// AUX (gsr_forward_aux / gsr_forward_train_aux): one more float per list entry through LDS, 1 / depth, and one more accumulator per pixel:
// out_invdepth = sum_i w_i / tz_i (no background term, not normalised) and out_alpha = 1 - T_final, each (H, W), either may be null.
template <bool TRAIN, bool AUX>
__global__ __launch_bounds__(RT) void k_render(const uint2 *__restrict__ ranges, const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ point_list, int W, int H, int gx,
                                            const float2 *__restrict__ xy, const float *__restrict__ colors, const float4 *__restrict__ conic_op,
                                            const float *__restrict__ bg, float *__restrict__ out, const uint32_t *__restrict__ slot_ids, float *__restrict__ final_T,
                                            uint32_t *__restrict__ n_end, const float *__restrict__ depth, float *__restrict__ out_invdepth,
                                            float *__restrict__ out_alpha)
{
    __shared__ float4 s_a[RT];   // x, y, conic.x, conic.y
    __shared__ float4 s_b[RT];   // conic.z, opacity, r, g
    __shared__ float2 s_c[RT];   // b, skip threshold: a Gaussian contributes to a pixel only if thr <= power <= 0
    __shared__ float s_d[AUX ? RT : 1];   // 1 / depth
    const int tile = (int)tile_order[blockIdx.x];
    const int tbx = tile % gx, tby = tile / gx;
    const int pxi = tbx * BX + (threadIdx.x & 15), py0 = tby * BY + (threadIdx.x >> 4), py1 = py0 + 8;
    const bool in0 = pxi < W && py0 < H, in1 = pxi < W && py1 < H;
    const float pxf = (float)pxi, pyf0 = (float)py0, pyf1 = (float)py1;
    const uint2 range = ranges[tile];
    bool done0 = !in0, done1 = !in1;
    float T0 = 1.0f, A0 = 0.f, A1 = 0.f, A2 = 0.f;
    float T1 = 1.0f, B0 = 0.f, B1 = 0.f, B2 = 0.f;
    uint32_t e0 = 0, e1 = 0;
    float D0 = 0.f, D1 = 0.f;
    for (uint32_t b0 = range.x; b0 < range.y; b0 += RT) {
        if (__syncthreads_count(done0 && done1) == RT) break;
        const uint32_t k = b0 + threadIdx.x;
        if (k < range.y) {
            uint32_t id;
            if constexpr (TRAIN) id = slot_ids[point_list[k]];
            else id = point_list[k];
            const float2 p = xy[id];
            const float4 co = conic_op[id];
            s_a[threadIdx.x] = make_float4(p.x, p.y, co.x, co.y);
            s_b[threadIdx.x] = make_float4(co.z, co.w, colors[3 * id], colors[3 * id + 1]);
            // alpha = op * exp(power) >= 1 / 255  <=>  power >= -ln(255 op); a margin keeps the borderline pixels on the exact test below
            // (a NaN opacity blends as alpha 0.99 in the reference -- fminf(0.99, NaN) -- so it must pass the pre-test: threshold -inf)
            s_c[threadIdx.x] = make_float2(colors[3 * id + 2], co.w > 0.0f ? -__logf(255.0f * co.w) - 1e-3f : (co.w != co.w ? -__builtin_inff() : __builtin_inff()));
            if constexpr (AUX) s_d[threadIdx.x] = 1.0f / depth[id];
        } else {
            // behind the list: a Gaussian of opacity 0 (alpha 0 < 1 / 255: never blended), so that the loop below runs in pairs
            s_a[threadIdx.x] = make_float4(0.f, 0.f, 1.f, 0.f); s_b[threadIdx.x] = make_float4(1.f, 0.f, 0.f, 0.f); s_c[threadIdx.x] = make_float2(0.f, __builtin_inff());
            if constexpr (AUX) s_d[threadIdx.x] = 0.0f;
        }
        __syncthreads();
        const int cnt = (int)min((uint32_t)RT, range.y - b0);
        for (int j = 0; j < cnt; j += 2) {
            if (__builtin_amdgcn_ballot_w64(!(done0 && done1)) == 0ull) break;   // the wave's 128 pixels are saturated
            // two Gaussians per trip: their six LDS reads are in flight together
            const float4 a = s_a[j], bq = s_b[j], a2 = s_a[j + 1], bq2 = s_b[j + 1];
            const float2 cb = s_c[j], cb2 = s_c[j + 1];
            float da = 0.f, db = 0.f;
            if constexpr (AUX) { da = s_d[j]; db = s_d[j + 1]; }
            const float dxa = a.x - pxf, dya0 = a.y - pyf0, dya1 = a.y - pyf1;
            const float pa0 = -0.5f * (a.z * dxa * dxa + bq.x * dya0 * dya0) - a.w * dxa * dya0;
            const float pa1 = -0.5f * (a.z * dxa * dxa + bq.x * dya1 * dya1) - a.w * dxa * dya1;
            const float dxb = a2.x - pxf, dyb0 = a2.y - pyf0, dyb1 = a2.y - pyf1;
            const float pb0 = -0.5f * (a2.z * dxb * dxb + bq2.x * dyb0 * dyb0) - a2.w * dxb * dyb0;
            const float pb1 = -0.5f * (a2.z * dxb * dxb + bq2.x * dyb1 * dyb1) - a2.w * dxb * dyb1;
            // a Gaussian whose footprint misses all 128 pixels of the wave (most of a tile's list at the corners of the 3-sigma boxes, and
            // every Gaussian that only touches the tile's other half) costs the twelve instructions above and no exponential
            if (__builtin_amdgcn_ballot_w64((!done0 && !(pa0 < cb.y) && !(pa0 > 0.0f)) || (!done1 && !(pa1 < cb.y) && !(pa1 > 0.0f))) != 0ull) {   // (a NaN power passes, as in the reference's `if (power > 0) continue`)
                if constexpr (TRAIN) {
                    blend_one_rec<AUX>(pa0, bq.y, bq.z, bq.w, cb.x, done0, T0, A0, A1, A2, b0 + (uint32_t)j + 1u, e0, da, D0);
                    blend_one_rec<AUX>(pa1, bq.y, bq.z, bq.w, cb.x, done1, T1, B0, B1, B2, b0 + (uint32_t)j + 1u, e1, da, D1);
                } else {
                    blend_one<AUX>(pa0, bq.y, bq.z, bq.w, cb.x, done0, T0, A0, A1, A2, da, D0);
                    blend_one<AUX>(pa1, bq.y, bq.z, bq.w, cb.x, done1, T1, B0, B1, B2, da, D1);
                }
            }
            if (__builtin_amdgcn_ballot_w64((!done0 && !(pb0 < cb2.y) && !(pb0 > 0.0f)) || (!done1 && !(pb1 < cb2.y) && !(pb1 > 0.0f))) != 0ull) {
                if constexpr (TRAIN) {
                    blend_one_rec<AUX>(pb0, bq2.y, bq2.z, bq2.w, cb2.x, done0, T0, A0, A1, A2, b0 + (uint32_t)j + 2u, e0, db, D0);
                    blend_one_rec<AUX>(pb1, bq2.y, bq2.z, bq2.w, cb2.x, done1, T1, B0, B1, B2, b0 + (uint32_t)j + 2u, e1, db, D1);
                } else {
                    blend_one<AUX>(pb0, bq2.y, bq2.z, bq2.w, cb2.x, done0, T0, A0, A1, A2, db, D0);
                    blend_one<AUX>(pb1, bq2.y, bq2.z, bq2.w, cb2.x, done1, T1, B0, B1, B2, db, D1);
                }
            }
        }
    }
    const size_t plane = (size_t)W * H;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    if (in0) {
        const size_t pix = (size_t)py0 * W + pxi;
        out[pix] = A0 + T0 * bg0; out[plane + pix] = A1 + T0 * bg1; out[2 * plane + pix] = A2 + T0 * bg2;
        if constexpr (TRAIN) { final_T[pix] = T0; n_end[pix] = e0; }
        if constexpr (AUX) {
            if (out_invdepth) out_invdepth[pix] = D0;
            if (out_alpha) out_alpha[pix] = 1.0f - T0;
        }
    }
    if (in1) {
        const size_t pix = (size_t)py1 * W + pxi;
        out[pix] = B0 + T1 * bg0; out[plane + pix] = B1 + T1 * bg1; out[2 * plane + pix] = B2 + T1 * bg2;
        if constexpr (TRAIN) { final_T[pix] = T1; n_end[pix] = e1; }
        if constexpr (AUX) {
            if (out_invdepth) out_invdepth[pix] = D1;
            if (out_alpha) out_alpha[pix] = 1.0f - T1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Backward (training).  The training forward (gsr_forward_train) sorts each pair's SLOT -- its position in k_duplicate_sorted's output, where
// Gaussian perm[s]'s pairs fill offs[s] .. offs[s+1]-1 -- instead of the Gaussian id, so every entry of a tile's list knows its slot.
// k_render_backward writes one record of NREC floats per pair at that slot; k_preprocess_backward sums each Gaussian's contiguous records in slot
// order and chains the sum through the forward's projection.  Every sum has a fixed order: no float atomics, and the gradients are bitwise
// reproducible run to run.
constexpr int NREC = 9;   // per pair: dL/d(r, g, b, opacity, conic.x, conic.y, conic.z, pixel x, pixel y), summed over the tile's pixels

__global__ __launch_bounds__(TB) void k_iota(uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i < n) out[i] = i;
}

// Sum over the 64 lanes of a wave in a fixed order, complete in lane 63: quad swaps, half-row and row mirrors (every lane of a row then holds
// the row's sum -- IEEE addition commutes, so the partners agree bit for bit), then the two row broadcasts.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK, int N>
__device__ __forceinline__ void dpp_add_all(float *v)
{
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<CTRL, ROW_MASK>(v[c]);
}
// step-major over the N values: a DPP read of a register written one instruction earlier costs wait states (s_nop), N independent sums hide them
template <int N>
__device__ __forceinline__ void wave_sum_to_63(float *v)
{
    dpp_add_all<0xB1, 0xF, N>(v);     // quad_perm [1, 0, 3, 2]
    dpp_add_all<0x4E, 0xF, N>(v);     // quad_perm [2, 3, 0, 1]
    dpp_add_all<0x141, 0xF, N>(v);    // row_half_mirror
    dpp_add_all<0x140, 0xF, N>(v);    // row_mirror
    dpp_add_all<0x142, 0xA, N>(v);    // row_bcast15 into rows 1 and 3
    dpp_add_all<0x143, 0xC, N>(v);    // row_bcast31 into rows 2 and 3
}

// One (pixel, Gaussian) step of the walk back to front.  T enters as the transmittance after the Gaussian and leaves as the one in front of it;
// S is the colour blended behind it, normalised by the transmittance behind it.  tb = T_final * <dL/dpixel, bg>.  The decision is the forward's:
// `cand` holds k < n_end and the power test, alpha the forward's expressions; the saturation test needs no repeat (a pair before the pixel's last
// blended one was not saturated).  The gradient passes through min(0.99, .) as if it were not there.
// AUX: inverse depth d is a fourth colour channel with background 0 (gradient gD, running SD, record v[NREC] = sum of gD w); the alpha map's
// gradient gO is already inside tb = T_final * (<dL/dpixel, bg> - gO), since d(1 - T_final) / dalpha = T_final / (1 - alpha).
template <bool AUX>
__device__ __forceinline__ bool grad_one(bool cand, float power, float dx, float dy, float A, float B, float C, float op, float r, float g, float b,
                                         float gr, float gg, float gb, float tb, float &T, float &S0, float &S1, float &S2, float *v, float d, float gD,
                                         float &SD)
{
    const float G = __builtin_amdgcn_exp2f(power * 1.44269504088896341f);
    const float alpha = fminf(0.99f, op * G);
    const bool bl = cand && !(alpha < 1.0f / 255.0f);
    const float inv = __builtin_amdgcn_rcpf(1.0f - alpha);
    const float Ti = T * inv;
    const float w = alpha * Ti;
    float bracket = gr * (r - S0) + gg * (g - S1) + gb * (b - S2);
    if constexpr (AUX) bracket += gD * (d - SD);   // after the colour terms: with gD = 0 the sum is the colour-only one
    const float dLda = Ti * bracket - tb * inv;
    const float dLdp = op * G * dLda;            // dalpha / dpower = op G
    v[0] += bl ? gr * w : 0.0f;
    v[1] += bl ? gg * w : 0.0f;
    v[2] += bl ? gb * w : 0.0f;
    v[3] += bl ? G * dLda : 0.0f;
    v[4] += bl ? -0.5f * dx * dx * dLdp : 0.0f;
    v[5] += bl ? -dx * dy * dLdp : 0.0f;
    v[6] += bl ? -0.5f * dy * dy * dLdp : 0.0f;
    v[7] += bl ? -(A * dx + B * dy) * dLdp : 0.0f;
    v[8] += bl ? -(C * dy + B * dx) * dLdp : 0.0f;
    S0 = bl ? alpha * r + (1.0f - alpha) * S0 : S0;
    S1 = bl ? alpha * g + (1.0f - alpha) * S1 : S1;
    S2 = bl ? alpha * b + (1.0f - alpha) * S2 : S2;
    if constexpr (AUX) {
        v[NREC] += bl ? gD * w : 0.0f;
        SD = bl ? alpha * d + (1.0f - alpha) * SD : SD;
    }
    T = bl ? Ti : T;
    return bl;
}

// One 16 x 16 tile per workgroup of RT lanes, two pixels per lane, as k_render; the list is walked back to front in LDS-staged batches of RT from
// the tile's largest n_end.  Per Gaussian a wave sums its 128 pixels' NREC values (wave_sum_to_63) only when one of its lanes blended it -- the
// forward's ballot skip --, the two waves' sums meet in LDS, and the batch's records go out with plain stores at their slots (wave 0's sum + wave
// 1's, in that order).  Entries behind the largest n_end are never reached: their records are written as zeros.
// AUX (gsr_backward_aux with a map gradient): records of NREC + 1 floats, 1 / depth staged as in k_render<., true>, and the gradients of the
// invdepth and alpha maps (d_invdepth, d_alpha: (H, W), either may be null = zero) walked along with the colour's.
template <bool AUX>
__global__ __launch_bounds__(RT) void k_render_backward(const uint2 *__restrict__ ranges, const uint32_t *__restrict__ tile_order, const uint32_t *__restrict__ slot_list,
                                                        const uint32_t *__restrict__ slot_ids, int W, int H, int gx, const float2 *__restrict__ xy,
                                                        const float *__restrict__ colors, const float4 *__restrict__ conic_op, const float *__restrict__ bg,
                                                        const float *__restrict__ final_T, const uint32_t *__restrict__ n_end, const float *__restrict__ dout,
                                                        float *__restrict__ rec, const float *__restrict__ depth, const float *__restrict__ d_invdepth,
                                                        const float *__restrict__ d_alpha)
{
    constexpr int NR = NREC + (AUX ? 1 : 0);
    __shared__ float4 s_a[RT];   // x, y, conic.x, conic.y
    __shared__ float4 s_b[RT];   // conic.z, opacity, r, g
    __shared__ float2 s_c[RT];   // b, skip threshold (k_render's)
    __shared__ float s_d[AUX ? RT : 1];   // 1 / depth
    __shared__ uint32_t s_slot[RT];
    __shared__ float s_part[2][NR][RT];
    __shared__ uint32_t s_top;
    const int tile = (int)tile_order[blockIdx.x];
    const int tbx = tile % gx, tby = tile / gx;
    const int pxi = tbx * BX + (threadIdx.x & 15), py0 = tby * BY + (threadIdx.x >> 4), py1 = py0 + 8;
    const bool in0 = pxi < W && py0 < H, in1 = pxi < W && py1 < H;
    const float pxf = (float)pxi, pyf0 = (float)py0, pyf1 = (float)py1;
    const uint2 range = ranges[tile];
    const size_t plane = (size_t)W * H;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    float T0 = 1.0f, g00 = 0.f, g01 = 0.f, g02 = 0.f, T1 = 1.0f, g10 = 0.f, g11 = 0.f, g12 = 0.f;
    uint32_t e0 = 0, e1 = 0;
    float gD0 = 0.f, gD1 = 0.f, gO0 = 0.f, gO1 = 0.f;
    if (in0) {
        const size_t pix = (size_t)py0 * W + pxi;
        T0 = final_T[pix]; e0 = n_end[pix]; g00 = dout[pix]; g01 = dout[plane + pix]; g02 = dout[2 * plane + pix];
        if constexpr (AUX) { if (d_invdepth) gD0 = d_invdepth[pix]; if (d_alpha) gO0 = d_alpha[pix]; }
    }
    if (in1) {
        const size_t pix = (size_t)py1 * W + pxi;
        T1 = final_T[pix]; e1 = n_end[pix]; g10 = dout[pix]; g11 = dout[plane + pix]; g12 = dout[2 * plane + pix];
        if constexpr (AUX) { if (d_invdepth) gD1 = d_invdepth[pix]; if (d_alpha) gO1 = d_alpha[pix]; }
    }
    // the alpha map joins the background term: d(1 - T_final) / dalpha_i = T_final / (1 - alpha_i)
    float bgs0 = g00 * bg0 + g01 * bg1 + g02 * bg2;
    if constexpr (AUX) bgs0 -= gO0;
    const float tb0 = T0 * bgs0;
    float bgs1 = g10 * bg0 + g11 * bg1 + g12 * bg2;
    if constexpr (AUX) bgs1 -= gO1;
    const float tb1 = T1 * bgs1;
    if (threadIdx.x == 0) s_top = 0u;
    __syncthreads();
    if (max(e0, e1) > 0u) atomicMax(&s_top, max(e0, e1));
    __syncthreads();
    const uint32_t top = max(s_top, range.x);
    for (uint32_t k = top + threadIdx.x; k < range.y; k += RT) {
        float *__restrict__ r = rec + (size_t)slot_list[k] * NR;
        for (int c = 0; c < NR; ++c) r[c] = 0.0f;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float S00 = 0.f, S01 = 0.f, S02 = 0.f, S10 = 0.f, S11 = 0.f, S12 = 0.f, SD0 = 0.f, SD1 = 0.f;
    for (uint32_t hi = top; hi > range.x;) {
        const uint32_t lo = hi - range.x > (uint32_t)RT ? hi - RT : range.x;
        const int cnt = (int)(hi - lo);
        __syncthreads();   // the previous batch's LDS is read out
        const int t = threadIdx.x;
        if (t < cnt) {
            const uint32_t slot = slot_list[lo + t];
            const uint32_t id = slot_ids[slot];
            const float2 p = xy[id];
            const float4 co = conic_op[id];
            s_slot[t] = slot;
            s_a[t] = make_float4(p.x, p.y, co.x, co.y);
            s_b[t] = make_float4(co.z, co.w, colors[3 * id], colors[3 * id + 1]);
            s_c[t] = make_float2(colors[3 * id + 2], co.w > 0.0f ? -__logf(255.0f * co.w) - 1e-3f : (co.w != co.w ? -__builtin_inff() : __builtin_inff()));
            if constexpr (AUX) s_d[t] = 1.0f / depth[id];   // k_render's expression
        }
        for (int c = 0; c < NR; ++c) { s_part[0][c][t] = 0.0f; s_part[1][c][t] = 0.0f; }
        __syncthreads();
        for (int j = cnt - 1; j >= 0; --j) {
            const uint32_t k = lo + (uint32_t)j;
            const float4 a = s_a[j], bq = s_b[j];
            const float2 cb = s_c[j];
            float dj = 0.f;
            if constexpr (AUX) dj = s_d[j];
            // the forward's expressions, operation for operation (-ffp-contract=off): the same power, so the same decisions
            const float dxa = a.x - pxf, dya0 = a.y - pyf0, dya1 = a.y - pyf1;
            const float pa0 = -0.5f * (a.z * dxa * dxa + bq.x * dya0 * dya0) - a.w * dxa * dya0;
            const float pa1 = -0.5f * (a.z * dxa * dxa + bq.x * dya1 * dya1) - a.w * dxa * dya1;
            const bool c0 = k < e0 && !(pa0 < cb.y) && !(pa0 > 0.0f);
            const bool c1 = k < e1 && !(pa1 < cb.y) && !(pa1 > 0.0f);
            if (__builtin_amdgcn_ballot_w64(c0 || c1) == 0ull) continue;
            float v[NR];
            for (int c = 0; c < NR; ++c) v[c] = 0.0f;
            const bool b0 = grad_one<AUX>(c0, pa0, dxa, dya0, a.z, a.w, bq.x, bq.y, bq.z, bq.w, cb.x, g00, g01, g02, tb0, T0, S00, S01, S02, v, dj, gD0, SD0);
            const bool b1 = grad_one<AUX>(c1, pa1, dxa, dya1, a.z, a.w, bq.x, bq.y, bq.z, bq.w, cb.x, g10, g11, g12, tb1, T1, S10, S11, S12, v, dj, gD1, SD1);
            if (__builtin_amdgcn_ballot_w64(b0 || b1) == 0ull) continue;
            wave_sum_to_63<NR>(v);
            if (lane == 63)
                for (int c = 0; c < NR; ++c) s_part[wave][c][j] = v[c];
        }
        __syncthreads();
        if (t < cnt) {
            float *__restrict__ r = rec + (size_t)s_slot[t] * NR;
            for (int c = 0; c < NR; ++c) r[c] = s_part[0][c][t] + s_part[1][c][t];
        }
        hi = lo;
    }
}

// One lane per Gaussian in depth order (position s of the first-level sort: its records are the contiguous slots offs[s] .. offs[s+1]-1), summed
// in slot order; then the chain back through k_preprocess's math: pixel centre -> NDC -> means3D; conic -> 2-D covariance -> J and the view
// rotation -> 3-D covariance -> scales (with scale_modifier) and the raw quaternion, or cov3D_precomp.  A coordinate clamped at +-1.3 tan(fov)
// enters J as a constant; Gaussians with radius 0 get exactly zero.
// AUX: records of NREC + 1 floats; the last, dL/d(1 / tz), joins the view-depth gradient as -(sum) / tz^2, after the Jacobian's terms.
template <bool AUX>
__global__ __launch_bounds__(TB) void k_preprocess_backward(int P, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ offs, const float *__restrict__ rec,
                                                            const float *__restrict__ means, const float *__restrict__ scales, const float *__restrict__ rots,
                                                            const float *__restrict__ cov3d_pre, Cam cam, const int *__restrict__ radii,
                                                            float *__restrict__ g_means3D, float *__restrict__ g_means2D, float *__restrict__ g_colors,
                                                            float *__restrict__ g_opac, float *__restrict__ g_scales, float *__restrict__ g_rots,
                                                            float *__restrict__ g_cov3D)
{
    const int s = blockIdx.x * TB + threadIdx.x;
    if (s >= P) return;
    constexpr int NR = NREC + (AUX ? 1 : 0);
    const uint32_t i = perm[s];
    float acc[NR];
    for (int c = 0; c < NR; ++c) acc[c] = 0.0f;
    float gm0 = 0.f, gm1 = 0.f, gm2 = 0.f, gnx = 0.f, gny = 0.f;
    float gc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
    if (radii[i] > 0) {
        for (uint32_t q = offs[s], qe = offs[s + 1]; q < qe; ++q)
            for (int c = 0; c < NR; ++c) acc[c] += rec[(size_t)q * NR + c];
        // k_preprocess's forward values
        const float px = means[3 * i], py = means[3 * i + 1], pz = means[3 * i + 2];
        const float *__restrict__ V = cam.view, *__restrict__ M = cam.proj;
        const float tx0 = V[0] * px + V[4] * py + V[8] * pz + V[12];
        const float ty0 = V[1] * px + V[5] * py + V[9] * pz + V[13];
        const float tz = V[2] * px + V[6] * py + V[10] * pz + V[14];
        const float hx = M[0] * px + M[4] * py + M[8] * pz + M[12];
        const float hy = M[1] * px + M[5] * py + M[9] * pz + M[13];
        const float hw = M[3] * px + M[7] * py + M[11] * pz + M[15];
        const float pw = 1.0f / (hw + 0.0000001f);
        float c[6], R[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, sc[3] = {0.f, 0.f, 0.f};
        float qr = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
        if (cov3d_pre) {
            for (int k = 0; k < 6; ++k) c[k] = cov3d_pre[6 * i + k];
        } else {
            sc[0] = cam.scale_modifier * scales[3 * i]; sc[1] = cam.scale_modifier * scales[3 * i + 1]; sc[2] = cam.scale_modifier * scales[3 * i + 2];
            qr = rots[4 * i]; qx = rots[4 * i + 1]; qy = rots[4 * i + 2]; qz = rots[4 * i + 3];
            R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); R[0][1] = 2.f * (qx * qy - qr * qz); R[0][2] = 2.f * (qx * qz + qr * qy);
            R[1][0] = 2.f * (qx * qy + qr * qz); R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); R[1][2] = 2.f * (qy * qz - qr * qx);
            R[2][0] = 2.f * (qx * qz - qr * qy); R[2][1] = 2.f * (qy * qz + qr * qx); R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
            const float ax = sc[0] * sc[0], ay = sc[1] * sc[1], az = sc[2] * sc[2];
            c[0] = ax * R[0][0] * R[0][0] + ay * R[0][1] * R[0][1] + az * R[0][2] * R[0][2];
            c[1] = ax * R[0][0] * R[1][0] + ay * R[0][1] * R[1][1] + az * R[0][2] * R[1][2];
            c[2] = ax * R[0][0] * R[2][0] + ay * R[0][1] * R[2][1] + az * R[0][2] * R[2][2];
            c[3] = ax * R[1][0] * R[1][0] + ay * R[1][1] * R[1][1] + az * R[1][2] * R[1][2];
            c[4] = ax * R[1][0] * R[2][0] + ay * R[1][1] * R[2][1] + az * R[1][2] * R[2][2];
            c[5] = ax * R[2][0] * R[2][0] + ay * R[2][1] * R[2][1] + az * R[2][2] * R[2][2];
        }
        const float limx = 1.3f * cam.tan_fovx, limy = 1.3f * cam.tan_fovy;
        const float txtz = tx0 / tz, tytz = ty0 / tz;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz;
        const float ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
        const bool clx = txtz < -limx || txtz > limx, cly = tytz < -limy || tytz > limy;
        const float fx = cam.focal_x, fy = cam.focal_y;
        const float j00 = fx / tz, j02 = -(fx * tx) / (tz * tz);
        const float j11 = fy / tz, j12 = -(fy * ty) / (tz * tz);
        const float a0x = j00 * V[0] + j02 * V[2], a0y = j00 * V[4] + j02 * V[6], a0z = j00 * V[8] + j02 * V[10];
        const float a1x = j11 * V[1] + j12 * V[2], a1y = j11 * V[5] + j12 * V[6], a1z = j11 * V[9] + j12 * V[10];
        const float s0x = c[0] * a0x + c[1] * a0y + c[2] * a0z, s0y = c[1] * a0x + c[3] * a0y + c[4] * a0z, s0z = c[2] * a0x + c[4] * a0y + c[5] * a0z;
        const float s1x = c[0] * a1x + c[1] * a1y + c[2] * a1z, s1y = c[1] * a1x + c[3] * a1y + c[4] * a1z, s1z = c[2] * a1x + c[4] * a1y + c[5] * a1z;
        const float cxx = a0x * s0x + a0y * s0y + a0z * s0z + 0.3f;
        const float cxy = a0x * s1x + a0y * s1y + a0z * s1z;
        const float cyy = a1x * s1x + a1y * s1y + a1z * s1z + 0.3f;
        const float det = cxx * cyy - cxy * cxy;
        const float id2 = 1.0f / (det * det);
        // pixel centre -> NDC (ix = ((ndc + 1) W - 1) / 2) -> clip -> means3D
        gnx = acc[7] * (0.5f * (float)cam.W); gny = acc[8] * (0.5f * (float)cam.H);
        const float ghx = gnx * pw, ghy = gny * pw, ghw = -(gnx * hx + gny * hy) * pw * pw;
        gm0 = ghx * M[0] + ghy * M[1] + ghw * M[3];
        gm1 = ghx * M[4] + ghy * M[5] + ghw * M[7];
        gm2 = ghx * M[8] + ghy * M[9] + ghw * M[11];
        // conic (cyy, -cxy, cxx) / det -> 2-D covariance
        const float gA = acc[4], gB = acc[5], gC = acc[6];
        const float ga = (-cyy * cyy * gA + cxy * cyy * gB - cxy * cxy * gC) * id2;
        const float gb = (2.0f * cxy * cyy * gA - (cxx * cyy + cxy * cxy) * gB + 2.0f * cxx * cxy * gC) * id2;
        const float gd = (-cxy * cxy * gA + cxx * cxy * gB - cxx * cxx * gC) * id2;
        // cxx = a0' S a0 + 0.3, cxy = a0' S a1, cyy = a1' S a1 + 0.3 -> the rows a0, a1 of J W and the 3-D covariance (off-diagonals: both uses)
        const float ga0x = 2.0f * ga * s0x + gb * s1x, ga0y = 2.0f * ga * s0y + gb * s1y, ga0z = 2.0f * ga * s0z + gb * s1z;
        const float ga1x = gb * s0x + 2.0f * gd * s1x, ga1y = gb * s0y + 2.0f * gd * s1y, ga1z = gb * s0z + 2.0f * gd * s1z;
        gc[0] = ga * a0x * a0x + gb * a0x * a1x + gd * a1x * a1x;
        gc[1] = 2.0f * ga * a0x * a0y + gb * (a0x * a1y + a0y * a1x) + 2.0f * gd * a1x * a1y;
        gc[2] = 2.0f * ga * a0x * a0z + gb * (a0x * a1z + a0z * a1x) + 2.0f * gd * a1x * a1z;
        gc[3] = ga * a0y * a0y + gb * a0y * a1y + gd * a1y * a1y;
        gc[4] = 2.0f * ga * a0y * a0z + gb * (a0y * a1z + a0z * a1y) + 2.0f * gd * a1y * a1z;
        gc[5] = ga * a0z * a0z + gb * a0z * a1z + gd * a1z * a1z;
        // J -> view-space position (a clamped coordinate is a constant in J)
        const float gj00 = ga0x * V[0] + ga0y * V[4] + ga0z * V[8], gj02 = ga0x * V[2] + ga0y * V[6] + ga0z * V[10];
        const float gj11 = ga1x * V[1] + ga1y * V[5] + ga1z * V[9], gj12 = ga1x * V[2] + ga1y * V[6] + ga1z * V[10];
        const float tz2 = tz * tz, tz3 = tz2 * tz;
        float gtz = -fx / tz2 * gj00 + 2.0f * fx * tx / tz3 * gj02 - fy / tz2 * gj11 + 2.0f * fy * ty / tz3 * gj12;
        if constexpr (AUX) gtz += -acc[NREC] / tz2;   // the invdepth map: d(1 / tz) / dtz
        const float gtx = clx ? 0.0f : -fx / tz2 * gj02, gty = cly ? 0.0f : -fy / tz2 * gj12;
        gm0 += gtx * V[0] + gty * V[1] + gtz * V[2];
        gm1 += gtx * V[4] + gty * V[5] + gtz * V[6];
        gm2 += gtx * V[8] + gty * V[9] + gtz * V[10];
        if (!cov3d_pre) {
            // Sigma = R diag(s^2) R': dL/d(s_m^2) = (R' G R)_mm, dL/dR = 2 G R diag(s^2), G the symmetric gradient of Sigma
            const float G[3][3] = {{gc[0], 0.5f * gc[1], 0.5f * gc[2]}, {0.5f * gc[1], gc[3], 0.5f * gc[4]}, {0.5f * gc[2], 0.5f * gc[4], gc[5]}};
            float GR[3][3], gR[3][3];
            for (int r = 0; r < 3; ++r)
                for (int m = 0; m < 3; ++m) GR[r][m] = G[r][0] * R[0][m] + G[r][1] * R[1][m] + G[r][2] * R[2][m];
            for (int m = 0; m < 3; ++m) {
                const float gam = R[0][m] * GR[0][m] + R[1][m] * GR[1][m] + R[2][m] * GR[2][m];
                gs[m] = gam * 2.0f * sc[m] * cam.scale_modifier;
                const float am = sc[m] * sc[m];
                for (int r = 0; r < 3; ++r) gR[r][m] = 2.0f * am * GR[r][m];
            }
            gq[0] = 2.0f * (-qz * gR[0][1] + qy * gR[0][2] + qz * gR[1][0] - qx * gR[1][2] - qy * gR[2][0] + qx * gR[2][1]);
            gq[1] = 2.0f * (qy * gR[0][1] + qz * gR[0][2] + qy * gR[1][0] - 2.0f * qx * gR[1][1] - qr * gR[1][2] + qz * gR[2][0] + qr * gR[2][1] - 2.0f * qx * gR[2][2]);
            gq[2] = 2.0f * (-2.0f * qy * gR[0][0] + qx * gR[0][1] + qr * gR[0][2] + qx * gR[1][0] + qz * gR[1][2] - qr * gR[2][0] + qz * gR[2][1] - 2.0f * qy * gR[2][2]);
            gq[3] = 2.0f * (-2.0f * qz * gR[0][0] - qr * gR[0][1] + qx * gR[0][2] + qr * gR[1][0] - 2.0f * qz * gR[1][1] + qy * gR[1][2] + qx * gR[2][0] + qy * gR[2][1]);
        }
    }
    g_means3D[3 * i] = gm0; g_means3D[3 * i + 1] = gm1; g_means3D[3 * i + 2] = gm2;
    g_means2D[3 * i] = gnx; g_means2D[3 * i + 1] = gny; g_means2D[3 * i + 2] = 0.0f;
    g_colors[3 * i] = acc[0]; g_colors[3 * i + 1] = acc[1]; g_colors[3 * i + 2] = acc[2];
    g_opac[i] = acc[3];
    if (cov3d_pre) {
        for (int k = 0; k < 6; ++k) g_cov3D[6 * i + k] = gc[k];
    } else {
        for (int k = 0; k < 3; ++k) g_scales[3 * i + k] = gs[k];
        for (int k = 0; k < 4; ++k) g_rots[4 * i + k] = gq[k];
    }
}

int make_cam(Cam *cam, int W, int H, const float *view_dev, const float *proj_dev, float tan_fovx, float tan_fovy, float scale_modifier)
{
    cam->view = view_dev; cam->proj = proj_dev;
    cam->tan_fovx = tan_fovx; cam->tan_fovy = tan_fovy;
    cam->focal_x = (float)W / (2.0f * tan_fovx); cam->focal_y = (float)H / (2.0f * tan_fovy);
    cam->scale_modifier = scale_modifier;
    cam->W = W; cam->H = H; cam->gx = (W + BX - 1) / BX; cam->gy = (H + BY - 1) / BY;
    return GPCC_OK;
}

// The frame state gsr_forward_train hands to gsr_backward: GSR_STATE_WORDS host words, the fields below in this order (word 0 = L ... word 13 = n_end;
// words 14 and 15 are zero unless the frame was rendered with a map: the per-Gaussian view depth, kept with the frame, and which maps).
constexpr uint64_t AUX_INVDEPTH = 1, AUX_ALPHA = 2;
struct FrameState {
    uint64_t L, P, W, H;
    const float2 *xy;
    const float4 *conic_op;
    const uint32_t *perm, *offs;
    const uint2 *ranges;
    const uint32_t *tile_order, *slots, *slot_ids;
    const float *final_T;
    const uint32_t *n_end;
    const float *depth;
    uint64_t aux;
};
static_assert(sizeof(FrameState) == GSR_STATE_WORDS * 8, "the frame state is the sixteen 64-bit words of gsr_forward_train's state[]");
void store_state(const FrameState &s, uint64_t *state) { memcpy(state, &s, sizeof s); }
FrameState load_state(const uint64_t *state) { FrameState s; memcpy(&s, state, sizeof s); return s; }

// The buffers of a frame that the backward reads again (and the ping-pong halves of the sorts that fill them), with their element counts.  The
// training frame takes them from the caller, once; the inference frame from the arena, per attempt, with npix = 0 (final_T and n_end unused).
struct FrameBufs {
    float2 *xy;
    float4 *conic_op;
    uint32_t *perm_a, *perm_b, *offs, *ord_a, *ord_b, *n_end;
    uint2 *ranges;
    float *final_T;
    float *depth;   // the training frame with a map (ndepth = P1), else nothing: the frame's depths live in the arena
};
template <class Taker> void take_frame_bufs(Taker &c, FrameBufs &b, size_t P1, size_t ntiles, size_t npix, size_t ndepth)
{
    b.xy = c.template take<float2>(P1); b.conic_op = c.template take<float4>(P1); b.perm_a = c.template take<uint32_t>(P1); b.perm_b = c.template take<uint32_t>(P1);
    b.offs = c.template take<uint32_t>(P1 + 1); b.ranges = c.template take<uint2>(ntiles); b.ord_a = c.template take<uint32_t>(ntiles); b.ord_b = c.template take<uint32_t>(ntiles);
    b.final_T = c.template take<float>(npix); b.n_end = c.template take<uint32_t>(npix);
    if (ndepth) b.depth = c.template take<float>(ndepth);
}

// What differs between the two frames.  Training: the frame state lives in memory the caller hands out through `alloc` (so that it outlives the
// call and any other call on the context) and its addresses go to `state`; the tile sort carries slots (k_iota) with the Gaussian ids in slot_ids,
// and k_render<true> leaves final_T / n_end.  Only the scratch of the sorts stays in ctx->arena.
struct FrameMode {
    bool train;
    gsr_alloc_fn alloc;
    void *alloc_user;
    uint64_t *state;
    float *out_invdepth, *out_alpha;   // the maps of the _aux entry points, (H, W) each; both null: the frame as it was before them
};

// One frame, from the camera to the image: gsr_forward and gsr_forward_train after their argument checks.
int render_frame(gpcc_ctx *ctx, const FrameMode &m, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                 const float *opacities, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                 const float *projmatrix, float tan_fovx, float tan_fovy, float *out_color, int *radii, int64_t *num_rendered_out, hipStream_t st)
{
    Cam cam;
    GP_TRY(make_cam(&cam, W, H, viewmatrix, projmatrix, tan_fovx, tan_fovy, scale_modifier));
    const int ntiles = cam.gx * cam.gy;
    const size_t P1 = (size_t)std::max(P, 1);
    static const bool sort2 = dev_env_int("GAUSPCC_RASTER_SORT2", 1) != 0;
    static const int cull = dev_env_int("GAUSPCC_RASTER_CULL", 1) != 0 ? 1 : 0;   // exact tile culling (tile_touches); 0: the reference's lists
    static const bool stats = dev_env_int("GAUSPCC_RASTER_STATS", 0) != 0;
    const bool two_level = m.train || sort2;   // the single sort on (tile << 32 | depth bits) exists for the inference frame only
    const bool aux = m.out_invdepth || m.out_alpha;
    FrameBufs b = {};
    if (m.train)   // frame state sized by P, the tiles and the pixels: one block from the caller
        GP_TRY(caller_block(m.alloc, m.alloc_user, "gsr_forward_train: frame state",
                            [&](Carver &c) { take_frame_bufs(c, b, P1, ntiles, (size_t)W * H, aux ? P1 : 0); }));
    uint32_t *slot_ids = nullptr, *sa = nullptr, *sb = nullptr;   // training, sized by the pair count: slot -> Gaussian, and the sorted slots (the sort ping-pongs)
    size_t want = P1 * 112 + (size_t)ntiles * (m.train ? 32 : 8) + ((size_t)8 << 20);
    uint32_t L = 0;
    // the two counts a frame reads back mid-way land in pinned memory (copies into stack variables are staged by the runtime, one blocking hop each)
    GP_TRY(ctx->hstage.reserve(64));
    volatile uint32_t *hL = reinterpret_cast<volatile uint32_t *>(ctx->hstage.p);
    volatile unsigned long long *hrect = reinterpret_cast<volatile unsigned long long *>(ctx->hstage.p + 8);
    for (int attempt = 0; attempt < 2; ++attempt) {
        GP_TRY(ctx->arena.reserve(want + (size_t)L * 40));
        ctx->arena.reset();
        if (!m.train) {   // `want` covers what P sizes and the ranges; the tile order's pair comes out of the slack, or of a second attempt
            take_frame_bufs(ctx->arena, b, P1, ntiles, 0, 0);
            if (!b.xy || !b.conic_op || !b.perm_a || !b.perm_b || !b.offs || !b.ranges) return fail(GPCC_ERR_NOMEM, "rasteriser workspace");
            if (!b.ord_a || !b.ord_b) { want += (size_t)ntiles * 32; continue; }
        }
        TAKE(depth, float, P1); TAKE(touched, uint32_t, P1 + 1);
        if (b.depth) depth = b.depth;   // a training frame with a map keeps its depths for the backward
        TAKE(rect_total, unsigned long long, RECT_SLOTS + 1);      // the slots of k_preprocess, then their sum
        TAKE(dka, uint64_t, P1); TAKE(dkb, uint64_t, P1); TAKE(recs, uint4, P1);
        HIP_TRY(hipMemsetAsync(b.ranges, 0, sizeof(uint2) * (size_t)ntiles, st));
        HIP_TRY(hipMemsetAsync(rect_total, 0, 8 * (RECT_SLOTS + 1), st));
        unsigned long long rect_host = 0;
        const uint32_t *perm = two_level ? b.perm_a : nullptr;   // Gaussians in depth order (two-level sort)
        const uint32_t *offs = two_level ? b.offs : touched;
        if (P > 0) {
            k_preprocess<<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, means3D, scales, rotations, cov3D_precomp, opacities, cam, radii, b.xy, depth, b.conic_op, touched, cull,
                                                               cull ? rect_total : nullptr, two_level ? dka : nullptr, two_level ? b.perm_a : nullptr,
                                                               two_level ? recs : nullptr);
            LAUNCH_CHECK();
            if (cull) { k_sum_slots<<<1, RECT_SLOTS, 0, st>>>(rect_total, rect_total + RECT_SLOTS); LAUNCH_CHECK(); }
            if (two_level) {
                uint64_t *k0 = dka, *k1 = dkb; uint32_t *v0 = b.perm_a, *v1 = b.perm_b;
                GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, P, 32));
                k_sorted_counts<<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, k0, b.offs);
                LAUNCH_CHECK();
                GP_TRY(exclusive_scan_u32(ctx, st, b.offs, b.offs, P, b.offs + P));
                perm = v0;
            } else {
                GP_TRY(exclusive_scan_u32(ctx, st, touched, touched, P, touched + P));
            }
            HIP_TRY(hipMemcpyAsync(const_cast<uint32_t *>(hL), offs + P, 4, hipMemcpyDeviceToHost, st));
            if (cull) HIP_TRY(hipMemcpyAsync(const_cast<unsigned long long *>(hrect), rect_total + RECT_SLOTS, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            L = *hL;
            if (cull) rect_host = *hrect;
        }
        if (stats && !m.train)
            fprintf(stderr, "[gauspcc] rasteriser: %u (Gaussian, tile) pairs sorted and blended, %llu in the bounding squares\n", L, cull ? rect_host : (unsigned long long)L);
        if (num_rendered_out) *num_rendered_out = cull ? (int64_t)rect_host : (int64_t)L;   // the reference's count: every tile of every bounding square
        uint32_t *vals_sorted = nullptr;   // what the tile sort carried: Gaussian ids, or (training) slots
        if (L > 0) {
            if (m.train && !slot_ids)      // once: a second attempt keeps the block of the first
                GP_TRY(caller_block(m.alloc, m.alloc_user, "gsr_forward_train: pair state", [&](Carver &c) {
                    slot_ids = c.take<uint32_t>(L); sa = c.take<uint32_t>(L); sb = c.take<uint32_t>(L);
                }));
            uint64_t *ka = ctx->arena.take<uint64_t>(L), *kb = ctx->arena.take<uint64_t>(L);
            uint32_t *va = m.train ? sa : ctx->arena.take<uint32_t>(L), *vb = m.train ? sb : ctx->arena.take<uint32_t>(L);
            if (!ka || !kb || !va || !vb || ctx->arena.cap - ctx->arena.off < (size_t)L * 2 + ((size_t)2 << 20)) { want += (size_t)L * 4; continue; }  // grow and redo
            int tbits = 1;
            while ((1 << tbits) < ntiles) ++tbits;
            uint64_t *k0 = ka, *k1 = kb; uint32_t *v0 = va, *v1 = vb;
            if (two_level) {
                k_duplicate_sorted<<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, perm, recs, b.xy, offs, radii, cam.gx, cam.gy, ka, m.train ? slot_ids : va, b.conic_op, cull);
                LAUNCH_CHECK();
                if (m.train) { k_iota<<<(unsigned)cdiv(L, TB), TB, 0, st>>>(L, va); LAUNCH_CHECK(); }
                GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, L, tbits));   // stable on the same keys: one permutation, carrying ids or slots
                k_tile_ranges<<<(unsigned)cdiv(L, TB), TB, 0, st>>>((int)L, k0, 0, b.ranges);
            } else {
                k_duplicate<<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, b.xy, depth, offs, radii, cam.gx, cam.gy, ka, va, b.conic_op, cull);
                LAUNCH_CHECK();
                GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, L, 32 + tbits));
                k_tile_ranges<<<(unsigned)cdiv(L, TB), TB, 0, st>>>((int)L, k0, 32, b.ranges);
            }
            LAUNCH_CHECK();
            vals_sorted = v0;
        }
        uint32_t *tile_order = nullptr;
        {
            uint64_t *oka = ctx->arena.take<uint64_t>(ntiles), *okb = ctx->arena.take<uint64_t>(ntiles);
            if (!oka || !okb) { want += (size_t)ntiles * 32; continue; }
            k_tile_order_keys<<<(unsigned)cdiv(ntiles, TB), TB, 0, st>>>(b.ranges, ntiles, oka, b.ord_a);
            LAUNCH_CHECK();
            uint64_t *k0 = oka, *k1 = okb; uint32_t *v0 = b.ord_a, *v1 = b.ord_b;
            GP_TRY(radix_sort_u64(ctx, st, &k0, &k1, &v0, &v1, ntiles, 8));
            tile_order = v0;
        }
        if (m.train && aux)
            k_render<true, true><<<(unsigned)ntiles, RT, 0, st>>>(b.ranges, tile_order, vals_sorted, W, H, cam.gx, b.xy, colors_precomp, b.conic_op, background,
                                                                  out_color, slot_ids, b.final_T, b.n_end, depth, m.out_invdepth, m.out_alpha);
        else if (m.train)
            k_render<true, false><<<(unsigned)ntiles, RT, 0, st>>>(b.ranges, tile_order, vals_sorted, W, H, cam.gx, b.xy, colors_precomp, b.conic_op, background,
                                                                   out_color, slot_ids, b.final_T, b.n_end, nullptr, nullptr, nullptr);
        else if (aux)
            k_render<false, true><<<(unsigned)ntiles, RT, 0, st>>>(b.ranges, tile_order, vals_sorted, W, H, cam.gx, b.xy, colors_precomp, b.conic_op, background,
                                                                   out_color, nullptr, nullptr, nullptr, depth, m.out_invdepth, m.out_alpha);
        else
            k_render<false, false><<<(unsigned)ntiles, RT, 0, st>>>(b.ranges, tile_order, vals_sorted, W, H, cam.gx, b.xy, colors_precomp, b.conic_op, background,
                                                                    out_color, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        LAUNCH_CHECK();
        HIP_TRY(hipStreamSynchronize(st));
        if (m.train)
            store_state(FrameState{L, (uint64_t)P, (uint64_t)W, (uint64_t)H, b.xy, b.conic_op, perm, offs, b.ranges, tile_order, vals_sorted, slot_ids, b.final_T, b.n_end,
                                   b.depth, (m.out_invdepth ? AUX_INVDEPTH : 0) | (m.out_alpha ? AUX_ALPHA : 0)},
                        m.state);
        return device_error_check(ctx);
    }
    return fail(GPCC_ERR_NOMEM, "rasteriser workspace");
}

// the argument checks gsr_forward and gsr_forward_train share
int check_frame_args(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp, const float *opacities,
                     const float *scales, const float *rotations, const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                     const float *out_color, const int *radii)
{
    if (!ctx || !background || !viewmatrix || !projmatrix || !out_color) return fail(GPCC_ERR_ARG, "null argument");
    if (P > 0 && (!means3D || !colors_precomp || !opacities || !radii)) return fail(GPCC_ERR_ARG, "null argument");
    if (P > 0 && !cov3D_precomp && (!scales || !rotations)) return fail(GPCC_ERR_ARG, "provide scales + rotations or cov3D_precomp");
    if (W <= 0 || H <= 0) return fail(GPCC_ERR_ARG, "bad image size");
    return GPCC_OK;
}

}  // namespace

extern "C" int gsr_visible_filter(gpcc_ctx *ctx, int P, int W, int H, const float *means3D, const float *scales, float scale_modifier,
                                  const float *rotations, const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                                  float tan_fovx, float tan_fovy, int prefiltered, int *radii, void *stream)
{
    (void)prefiltered;
    if (!ctx || !means3D || !viewmatrix || !projmatrix || !radii) return fail(GPCC_ERR_ARG, "null argument");
    if (!cov3D_precomp && (!scales || !rotations)) return fail(GPCC_ERR_ARG, "provide scales + rotations or cov3D_precomp");
    if (P <= 0) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    Cam cam;
    GP_TRY(make_cam(&cam, W, H, viewmatrix, projmatrix, tan_fovx, tan_fovy, scale_modifier));
    k_preprocess<<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, means3D, scales, rotations, cov3D_precomp, nullptr, cam, radii, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_forward_aux(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                               const float *opacities, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                               const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy, int prefiltered, float *out_color,
                               int *radii, float *out_invdepth, float *out_alpha, int64_t *num_rendered_out, void *stream)
{
    (void)prefiltered;
    GP_TRY(check_frame_args(ctx, P, background, W, H, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, out_color, radii));
    HIP_TRY(hipSetDevice(ctx->device));
    return render_frame(ctx, FrameMode{false, nullptr, nullptr, nullptr, out_invdepth, out_alpha}, P, background, W, H, means3D, colors_precomp, opacities, scales,
                        scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, out_color, radii, num_rendered_out, (hipStream_t)stream);
}

extern "C" int gsr_forward(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                           const float *opacities, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                           const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy, int prefiltered, float *out_color,
                           int *radii, int64_t *num_rendered_out, void *stream)
{
    return gsr_forward_aux(ctx, P, background, W, H, means3D, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix,
                           tan_fovx, tan_fovy, prefiltered, out_color, radii, nullptr, nullptr, num_rendered_out, stream);
}

// The training forward: gsr_forward's two-level path with the frame state the backward needs kept (FrameMode).
extern "C" int gsr_forward_train_aux(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                                     const float *opacities, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                     const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy, int prefiltered, float *out_color,
                                     int *radii, float *out_invdepth, float *out_alpha, gsr_alloc_fn alloc, void *alloc_user, uint64_t *state,
                                     int64_t *num_rendered_out, void *stream)
{
    (void)prefiltered;
    if (!alloc || !state) return fail(GPCC_ERR_ARG, "null argument");
    GP_TRY(check_frame_args(ctx, P, background, W, H, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, out_color, radii));
    for (int k = 0; k < GSR_STATE_WORDS; ++k) state[k] = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    return render_frame(ctx, FrameMode{true, alloc, alloc_user, state, out_invdepth, out_alpha}, P, background, W, H, means3D, colors_precomp, opacities, scales,
                        scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, out_color, radii, num_rendered_out, (hipStream_t)stream);
}

extern "C" int gsr_forward_train(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                                 const float *opacities, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                 const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy, int prefiltered, float *out_color,
                                 int *radii, gsr_alloc_fn alloc, void *alloc_user, uint64_t *state, int64_t *num_rendered_out, void *stream)
{
    return gsr_forward_train_aux(ctx, P, background, W, H, means3D, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix,
                                 projmatrix, tan_fovx, tan_fovy, prefiltered, out_color, radii, nullptr, nullptr, alloc, alloc_user, state, num_rendered_out, stream);
}

extern "C" int gsr_backward_aux(gpcc_ctx *ctx, const uint64_t *state, int P, const float *background, int W, int H, const float *means3D,
                                const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                                const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy, const int *radii,
                                const float *dL_dout, const float *dL_dinvdepth, const float *dL_dalpha, gsr_alloc_fn alloc, void *alloc_user,
                                float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacities, float *dL_dscales, float *dL_drotations,
                                float *dL_dcov3D, void *stream)
{
    (void)opacities;
    if (!ctx || !state || !background || !viewmatrix || !projmatrix || !dL_dout || !alloc) return fail(GPCC_ERR_ARG, "null argument");
    const FrameState s = load_state(state);
    if (s.P != (uint64_t)P || s.W != (uint64_t)W || s.H != (uint64_t)H) return fail(GPCC_ERR_ARG, "frame state of another frame");
    if ((dL_dinvdepth && !(s.aux & AUX_INVDEPTH)) || (dL_dalpha && !(s.aux & AUX_ALPHA)))
        return fail(GPCC_ERR_ARG, "gradient of a map the frame was not rendered with");
    const bool aux = dL_dinvdepth || dL_dalpha;
    if (W <= 0 || H <= 0) return fail(GPCC_ERR_ARG, "bad image size");
    if (P <= 0) return GPCC_OK;
    if (!means3D || !colors_precomp || !radii || !dL_dmeans3D || !dL_dmeans2D || !dL_dcolors || !dL_dopacities) return fail(GPCC_ERR_ARG, "null argument");
    if (cov3D_precomp ? !dL_dcov3D : (!scales || !rotations || !dL_dscales || !dL_drotations)) return fail(GPCC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    Cam cam;
    GP_TRY(make_cam(&cam, W, H, viewmatrix, projmatrix, tan_fovx, tan_fovy, scale_modifier));
    const int ntiles = cam.gx * cam.gy;
    float *rec = nullptr;
    if (s.L > 0) {
        GP_TRY(caller_alloc(alloc, alloc_user, (size_t)s.L * (NREC + (aux ? 1 : 0)) * sizeof(float), &rec, "gsr_backward: records"));
        if (aux)
            k_render_backward<true><<<(unsigned)ntiles, RT, 0, st>>>(s.ranges, s.tile_order, s.slots, s.slot_ids, W, H, cam.gx, s.xy, colors_precomp, s.conic_op,
                                                                     background, s.final_T, s.n_end, dL_dout, rec, s.depth, dL_dinvdepth, dL_dalpha);
        else
            k_render_backward<false><<<(unsigned)ntiles, RT, 0, st>>>(s.ranges, s.tile_order, s.slots, s.slot_ids, W, H, cam.gx, s.xy, colors_precomp, s.conic_op,
                                                                      background, s.final_T, s.n_end, dL_dout, rec, nullptr, nullptr, nullptr);
        LAUNCH_CHECK();
    }
    if (aux)
        k_preprocess_backward<true><<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, s.perm, s.offs, rec, means3D, scales, rotations, cov3D_precomp, cam, radii, dL_dmeans3D,
                                                                          dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D);
    else
        k_preprocess_backward<false><<<(unsigned)cdiv(P, TB), TB, 0, st>>>(P, s.perm, s.offs, rec, means3D, scales, rotations, cov3D_precomp, cam, radii, dL_dmeans3D,
                                                                           dL_dmeans2D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_backward(gpcc_ctx *ctx, const uint64_t *state, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                            const float *opacities, const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                            const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy, const int *radii, const float *dL_dout,
                            gsr_alloc_fn alloc, void *alloc_user, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacities,
                            float *dL_dscales, float *dL_drotations, float *dL_dcov3D, void *stream)
{
    return gsr_backward_aux(ctx, state, P, background, W, H, means3D, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix,
                            projmatrix, tan_fovx, tan_fovy, radii, dL_dout, nullptr, nullptr, alloc, alloc_user, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacities,
                            dL_dscales, dL_drotations, dL_dcov3D, stream);
}
