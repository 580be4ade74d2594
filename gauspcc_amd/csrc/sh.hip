// sh.hip -- view-dependent colour from spherical-harmonic coefficients, the per-Gaussian pass in front of the rasteriser's kernels and
// its backward behind them (diff_gaussian_rasterization's computeColorFromSH, forward and backward; utils/sh_utils.py's eval_sh):
//   gsr_sh_forward    colours (P, 3) from coefficients, either from means3D and the camera centre (+0.5, clamp at 0) or from given directions
//   gsr_sh_backward   gradients for the coefficients and for means3D or the directions
//
// Arithmetic (include/gauspcc.h states the contract): float32, one IEEE operation per step, no fused multiply-add anywhere in this
// file; the basis polynomials and the sum over k are written out below in the order the contract fixes, once, in functions that the
// kernels of every memory path share.  The real basis with the Condon-Shortley sign folded into the constants; degree 4 is written for
// unit directions (r = 1), as eval_sh has it.
//
// Memory path: a Gaussian's coefficients are up to 75 floats that lie together, so a lane that walked its own row would touch a new
// 64-byte sector with almost every load while its neighbours' loads land a row apart.  Instead one wave owns 64 consecutive
// Gaussians and copies the part of their rows that holds active coefficients (`span` floats from each row's start) into LDS with
// consecutive lanes on consecutive addresses -- 16-byte loads when the rows are dense, whole float4s and 16-byte aligned, 4-byte
// loads otherwise -- into rows padded to an odd stride, from which every lane then reads its own row without bank conflicts.  The
// backward writes dL_dsh the same way round: each lane puts its row into LDS, the wave stores the block with consecutive lanes on
// consecutive addresses.  Rows whose strides do not allow this (a span above MAX_SPAN floats, a zero or negative stride, a gradient
// layout that is not a dense row) are read and written by their own lane directly.  Which path runs never changes a value: the
// arithmetic starts from registers that hold the same numbers.
// Every output element has exactly one owner; no atomics, no reductions.
#include "common.hpp"

#include <math.h>

using namespace gpcc;

namespace {

constexpr int WAVE = 64;
constexpr int MAX_SPAN = 96;             // floats of one row staged through LDS (degree 4: 75); 64 rows of 97 floats are 24.3 KiB

// 1/2 sqrt(1/pi); sqrt(3/(4 pi)); 1/2 sqrt(15/pi), 1/4 sqrt(5/pi), 1/4 sqrt(15/pi); 1/4 sqrt(35/(2 pi)), 1/2 sqrt(105/pi),
// 1/4 sqrt(21/(2 pi)), 1/4 sqrt(7/pi), 1/4 sqrt(105/pi); 3/4 sqrt(35/pi), 3/4 sqrt(35/(2 pi)), 3/4 sqrt(5/pi), 3/4 sqrt(5/(2 pi)),
// 3/16 sqrt(1/pi), 3/8 sqrt(5/pi), 3/16 sqrt(35/pi): doubles rounded to float32
constexpr float C0 = 0.28209479177387814f;
constexpr float C1 = 0.4886025119029199f;
constexpr float C2A = 1.0925484305920792f, C2C = 0.31539156525252005f, C2E = 0.5462742152960396f;
constexpr float C3A = 0.5900435899266435f, C3B = 2.890611442640554f, C3C = 0.4570457994644658f, C3D = 0.3731763325901154f, C3F = 1.445305721320277f;
constexpr float C4A = 2.5033429417967046f, C4B = 1.7701307697799304f, C4C = 0.9461746957575601f, C4D = 0.6690465435572892f, C4E = 0.10578554691520431f,
                C4G = 0.47308734787878004f, C4I = 0.6258357354491761f;

constexpr int sh_count(int degree) { return (degree + 1) * (degree + 1); }

// The shared second-order and higher products of a direction, in the contract's order.
struct Dir {
    float x, y, z;
    float xx, yy, zz, xy, yz, xz;
    float xmy, p, q, r, s, xyz, u, v, zz7;
    template <int D> __host__ __device__ __forceinline__ void set(float x_, float y_, float z_)
    {
        x = x_; y = y_; z = z_;
        if constexpr (D >= 2) {
            xx = x * x; yy = y * y; zz = z * z;
            xy = x * y; yz = y * z; xz = x * z;
            xmy = xx - yy;
        }
        if constexpr (D >= 3) {
            p = 3.0f * xx - yy;
            q = (4.0f * zz - xx) - yy;
            r = (2.0f * zz - 3.0f * xx) - 3.0f * yy;
            s = xx - 3.0f * yy;
            xyz = xy * z;
        }
        if constexpr (D >= 4) {
            zz7 = 7.0f * zz;
            u = zz7 - 1.0f;
            v = zz7 - 3.0f;
        }
    }
};

// basis_k(d), k < (D + 1)^2
template <int D> __host__ __device__ __forceinline__ void sh_basis(const Dir &d, float *b)
{
    b[0] = C0;
    if constexpr (D >= 1) {
        b[1] = -C1 * d.y;
        b[2] = C1 * d.z;
        b[3] = -C1 * d.x;
    }
    if constexpr (D >= 2) {
        b[4] = C2A * d.xy;
        b[5] = -C2A * d.yz;
        b[6] = C2C * ((2.0f * d.zz - d.xx) - d.yy);
        b[7] = -C2A * d.xz;
        b[8] = C2E * d.xmy;
    }
    if constexpr (D >= 3) {
        b[9] = -C3A * (d.y * d.p);
        b[10] = C3B * d.xyz;
        b[11] = -C3C * (d.y * d.q);
        b[12] = C3D * (d.z * d.r);
        b[13] = -C3C * (d.x * d.q);
        b[14] = C3F * (d.z * d.xmy);
        b[15] = -C3A * (d.x * d.s);
    }
    if constexpr (D >= 4) {
        b[16] = C4A * (d.xy * d.xmy);
        b[17] = -C4B * (d.yz * d.p);
        b[18] = C4C * (d.xy * d.u);
        b[19] = -C4D * (d.yz * d.v);
        b[20] = C4E * (d.zz * (35.0f * d.zz - 30.0f) + 3.0f);
        b[21] = -C4D * (d.xz * d.v);
        b[22] = C4G * (d.xmy * d.u);
        b[23] = -C4B * (d.xz * d.s);
        b[24] = C4I * (d.xx * d.s - d.yy * d.p);
    }
}

// value_c = sum_k basis_k sh[k][c], k ascending from the DC term
template <int D> __host__ __device__ __forceinline__ void sh_value(const float (*sh)[3], const Dir &d, float *val)
{
    constexpr int K = sh_count(D);
    float b[K];
    sh_basis<D>(d, b);
    _Pragma("unroll") for (int c = 0; c < 3; ++c) {
        float acc = b[0] * sh[0][c];
#pragma unroll
        for (int k = 1; k < K; ++k) acc = acc + b[k] * sh[k][c];
        val[c] = acc;
    }
}

// dL/dd = sum_k (d basis_k / dd) t_k with t_k = (sh[k][0] g_0 + sh[k][1] g_1) + sh[k][2] g_2, k ascending from 1; a component whose
// derivative is identically zero adds no term, and each sum starts with its first term (k = 3, 1, 2 for x, y, z), not with a zero:
// nothing in the chain is an addition the compiler could drop, so the sign of a zero result is the chain's own.  Degree 0 has no
// term: exactly +0.  Each derivative is a constant times a polynomial, as the basis is.
template <int D> __host__ __device__ __forceinline__ void sh_dir_grad(const float (*sh)[3], const Dir &d, const float *g, float *out)
{
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;   // overwritten by the first term of each sum
    bool hx = false, hy = false, hz = false;
    float t;
#define SH_T(k) t = (sh[k][0] * g[0] + sh[k][1] * g[1]) + sh[k][2] * g[2]
#define SH_X(e) do { const float v_ = (e) * t; gx = hx ? gx + v_ : v_; hx = true; } while (0)
#define SH_Y(e) do { const float v_ = (e) * t; gy = hy ? gy + v_ : v_; hy = true; } while (0)
#define SH_Z(e) do { const float v_ = (e) * t; gz = hz ? gz + v_ : v_; hz = true; } while (0)
    if constexpr (D >= 1) {
        SH_T(1); SH_Y(-C1);
        SH_T(2); SH_Z(C1);
        SH_T(3); SH_X(-C1);
    }
    if constexpr (D >= 2) {
        SH_T(4); SH_X(C2A * d.y); SH_Y(C2A * d.x);
        SH_T(5); SH_Y(-C2A * d.z); SH_Z(-C2A * d.y);
        SH_T(6); SH_X((-2.0f * C2C) * d.x); SH_Y((-2.0f * C2C) * d.y); SH_Z((4.0f * C2C) * d.z);
        SH_T(7); SH_X(-C2A * d.z); SH_Z(-C2A * d.x);
        SH_T(8); SH_X((2.0f * C2E) * d.x); SH_Y((-2.0f * C2E) * d.y);
    }
    if constexpr (D >= 3) {
        SH_T(9); SH_X(-C3A * (6.0f * d.xy)); SH_Y(-C3A * (3.0f * d.xmy));
        SH_T(10); SH_X(C3B * d.yz); SH_Y(C3B * d.xz); SH_Z(C3B * d.xy);
        SH_T(11); SH_X(-C3C * (-2.0f * d.xy)); SH_Y(-C3C * (d.q - 2.0f * d.yy)); SH_Z(-C3C * (8.0f * d.yz));
        SH_T(12); SH_X(C3D * (-6.0f * d.xz)); SH_Y(C3D * (-6.0f * d.yz)); SH_Z(C3D * (d.r + 4.0f * d.zz));
        SH_T(13); SH_X(-C3C * (d.q - 2.0f * d.xx)); SH_Y(-C3C * (-2.0f * d.xy)); SH_Z(-C3C * (8.0f * d.xz));
        SH_T(14); SH_X(C3F * (2.0f * d.xz)); SH_Y(C3F * (-2.0f * d.yz)); SH_Z(C3F * d.xmy);
        SH_T(15); SH_X(-C3A * (3.0f * d.xmy)); SH_Y(-C3A * (-6.0f * d.xy));
    }
    if constexpr (D >= 4) {
        const float t19 = 21.0f * d.zz - 3.0f;
        SH_T(16); SH_X(C4A * (d.y * d.p)); SH_Y(C4A * (d.x * d.s));
        SH_T(17); SH_X(-C4B * (6.0f * d.xyz)); SH_Y(-C4B * (d.z * (3.0f * d.xmy))); SH_Z(-C4B * (d.y * d.p));
        SH_T(18); SH_X(C4C * (d.y * d.u)); SH_Y(C4C * (d.x * d.u)); SH_Z(C4C * (14.0f * d.xyz));
        SH_T(19); SH_Y(-C4D * (d.z * d.v)); SH_Z(-C4D * (d.y * t19));
        SH_T(20); SH_Z(C4E * (d.z * (140.0f * d.zz - 60.0f)));
        SH_T(21); SH_X(-C4D * (d.z * d.v)); SH_Z(-C4D * (d.x * t19));
        SH_T(22); SH_X(C4G * (2.0f * (d.x * d.u))); SH_Y(C4G * (-2.0f * (d.y * d.u))); SH_Z(C4G * (14.0f * (d.z * d.xmy)));
        SH_T(23); SH_X(-C4B * (d.z * (3.0f * d.xmy))); SH_Y(-C4B * (-6.0f * d.xyz)); SH_Z(-C4B * (d.x * d.s));
        SH_T(24); SH_X(C4I * (4.0f * (d.x * d.s))); SH_Y(C4I * (-4.0f * (d.y * d.p)));
    }
#undef SH_T
#undef SH_X
#undef SH_Y
#undef SH_Z
    (void)t; (void)hx; (void)hy; (void)hz;
    out[0] = gx; out[1] = gy; out[2] = gz;
}

// d = (mean - campos) / |mean - campos|; a squared length of exactly 0 gives d = 0 (NaN compares unequal and goes through the division)
__host__ __device__ __forceinline__ void view_dir(const float *mean, const float *campos, float *d, float &len, bool &at_centre)
{
    const float dx = mean[0] - campos[0], dy = mean[1] - campos[1], dz = mean[2] - campos[2];
    const float l2 = (dx * dx + dy * dy) + dz * dz;
    len = sqrtf(l2);
    at_centre = l2 == 0.0f;
    if (at_centre) { d[0] = 0.0f; d[1] = 0.0f; d[2] = 0.0f; }
    else { d[0] = dx / len; d[1] = dy / len; d[2] = dz / len; }
}

// One Gaussian forward.  vec: its mean (view: the direction comes from campos) or its direction.
template <int D> __host__ __device__ __forceinline__ void gaussian_forward(const float (*sh)[3], const float *vec, const float *campos, bool view,
                                                                            float *colour, uint8_t *clamped)
{
    float dir[3] = {vec[0], vec[1], vec[2]}, len = 1.0f;
    bool at_centre;
    if (view) view_dir(vec, campos, dir, len, at_centre);
    Dir d;
    d.set<D>(dir[0], dir[1], dir[2]);
    float val[3];
    sh_value<D>(sh, d, val);
    _Pragma("unroll") for (int c = 0; c < 3; ++c) {
        if (view) {
            const float v = val[c] + 0.5f;
            const bool neg = v < 0.0f;
            clamped[c] = neg ? 1 : 0;
            colour[c] = neg ? 0.0f : v;
        } else {
            colour[c] = val[c];
        }
    }
}

// One Gaussian backward: gsh[k][c] for k < (D + 1)^2 and the gradient of vec.
template <int D> __host__ __device__ __forceinline__ void gaussian_backward(const float (*sh)[3], const float *vec, const float *campos, bool view,
                                                                             const uint8_t *clamped, const float *dcolour, float (*gsh)[3], float *gvec)
{
    constexpr int K = sh_count(D);
    float dir[3] = {vec[0], vec[1], vec[2]}, len = 1.0f;
    bool at_centre = false;
    if (view) view_dir(vec, campos, dir, len, at_centre);
    Dir d;
    d.set<D>(dir[0], dir[1], dir[2]);
    float g[3];
    bool off[3];
    _Pragma("unroll") for (int c = 0; c < 3; ++c) {
        off[c] = view && clamped[c];
        g[c] = off[c] ? 0.0f : dcolour[c];
    }
    float b[K];
    sh_basis<D>(d, b);
#pragma unroll
    for (int k = 0; k < K; ++k)
        _Pragma("unroll") for (int c = 0; c < 3; ++c) gsh[k][c] = off[c] ? 0.0f : b[k] * g[c];
    float gd[3];
    sh_dir_grad<D>(sh, d, g, gd);
    if (D == 0 || (view && at_centre)) {
        gvec[0] = 0.0f; gvec[1] = 0.0f; gvec[2] = 0.0f;
    } else if (!view) {
        gvec[0] = gd[0]; gvec[1] = gd[1]; gvec[2] = gd[2];
    } else {
        // (I - d d^T) / len applied to dL/dd
        const float dot = (gd[0] * dir[0] + gd[1] * dir[1]) + gd[2] * dir[2];
        gvec[0] = (gd[0] - dir[0] * dot) / len;
        gvec[1] = (gd[1] - dir[1] * dot) / len;
        gvec[2] = (gd[2] - dir[2] * dot) / len;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Memory paths

enum { PATH_DIRECT = 0, PATH_STAGED = 1, PATH_STAGED_VEC = 2 };

struct Layout {
    int64_t coef, chan, row;             // strides in floats
    int span;                            // floats from a row's start that hold every active (forward) / every (gradient) entry
    int pad;                             // LDS row stride, odd
    int path;
    int step_rows, step_off;             // one step of a lane through the block (64 floats, or 256 on the 16-byte path) = step_rows rows + step_off floats
};

// (r, o) -> the position `step` floats further on; step_off < span, so one conditional subtraction normalises: no loop, no divergence
__device__ __forceinline__ void advance(const Layout &L, int &r, int &o)
{
    r += L.step_rows;
    o += L.step_off;
    const bool wrap = o >= L.span;
    o = wrap ? o - L.span : o;
    r = wrap ? r + 1 : r;
}

// global -> LDS: rows row0 .. row0 + nrows - 1, `span` floats each, to LDS rows of `pad` floats
__device__ __forceinline__ void stage_in(const float *__restrict__ base, const Layout &L, int64_t row0, int nrows, float *lds)
{
    const int lane = threadIdx.x;
    if (L.path == PATH_STAGED_VEC) {
        // dense rows: the block is nrows * span contiguous floats from a 16-byte aligned address, span a multiple of 4
        const float4 *src = reinterpret_cast<const float4 *>(base + row0 * L.row);
        int r = (4 * lane) / L.span, o = (4 * lane) % L.span;
        for (int i = lane; r < nrows; i += WAVE) {
            const float4 v = src[i];
            float *dst = lds + r * L.pad + o;
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            advance(L, r, o);
        }
    } else {
        int r = lane / L.span, o = lane % L.span;
        while (r < nrows) {
            lds[r * L.pad + o] = base[(row0 + r) * L.row + o];
            advance(L, r, o);
        }
    }
}

// LDS -> global, the mirror of stage_in
__device__ __forceinline__ void stage_out(float *__restrict__ base, const Layout &L, int64_t row0, int nrows, const float *lds)
{
    const int lane = threadIdx.x;
    if (L.path == PATH_STAGED_VEC) {
        float4 *dst = reinterpret_cast<float4 *>(base + row0 * L.row);
        int r = (4 * lane) / L.span, o = (4 * lane) % L.span;
        for (int i = lane; r < nrows; i += WAVE) {
            const float *src = lds + r * L.pad + o;
            dst[i] = make_float4(src[0], src[1], src[2], src[3]);
            advance(L, r, o);
        }
    } else {
        int r = lane / L.span, o = lane % L.span;
        while (r < nrows) {
            base[(row0 + r) * L.row + o] = lds[r * L.pad + o];
            advance(L, r, o);
        }
    }
}

// A lane's coefficients into registers: from its LDS row or, on the direct path, from global memory.
template <int K> __device__ __forceinline__ void load_row(const float *__restrict__ sh, const Layout &L, int64_t i, const float *lds, float (*reg)[3])
{
    if (L.path != PATH_DIRECT) {
        const float *row = lds + (int)threadIdx.x * L.pad;
        const int cs = (int)L.coef, hs = (int)L.chan;
#pragma unroll
        for (int k = 0; k < K; ++k)
            _Pragma("unroll") for (int c = 0; c < 3; ++c) reg[k][c] = row[k * cs + c * hs];
    } else {
        const float *row = sh + i * L.row;
#pragma unroll
        for (int k = 0; k < K; ++k)
            _Pragma("unroll") for (int c = 0; c < 3; ++c) reg[k][c] = row[k * L.coef + c * L.chan];
    }
}

template <int D> __global__ __launch_bounds__(WAVE) void k_sh_fwd(int P, const float *__restrict__ sh, Layout L, const float *__restrict__ means,
                                                                   const float *__restrict__ campos, const float *__restrict__ dirs,
                                                                   float *__restrict__ colours, uint8_t *__restrict__ clamped)
{
    constexpr int K = sh_count(D);
    extern __shared__ float lds[];
    const int64_t row0 = (int64_t)blockIdx.x * WAVE;
    const int nrows = (int)(P - row0 < WAVE ? P - row0 : WAVE);
    if (L.path != PATH_DIRECT) {
        stage_in(sh, L, row0, nrows, lds);
        __syncthreads();
    }
    const int lane = threadIdx.x;
    if (lane >= nrows) return;
    const int64_t i = row0 + lane;
    float reg[K][3];
    load_row<K>(sh, L, i, lds, reg);
    const float *vp = (means ? means : dirs) + 3 * i;
    const float vec[3] = {vp[0], vp[1], vp[2]};
    float cam[3] = {0.0f, 0.0f, 0.0f};
    if (means) { cam[0] = campos[0]; cam[1] = campos[1]; cam[2] = campos[2]; }
    float col[3];
    uint8_t cl[3] = {0, 0, 0};
    gaussian_forward<D>(reg, vec, cam, means != nullptr, col, cl);
    colours[3 * i + 0] = col[0]; colours[3 * i + 1] = col[1]; colours[3 * i + 2] = col[2];
    if (means) { clamped[3 * i + 0] = cl[0]; clamped[3 * i + 1] = cl[1]; clamped[3 * i + 2] = cl[2]; }
}

template <int D> __global__ __launch_bounds__(WAVE) void k_sh_bwd(int P, int M, const float *__restrict__ sh, Layout L, const float *__restrict__ means,
                                                                   const float *__restrict__ campos, const float *__restrict__ dirs,
                                                                   const uint8_t *__restrict__ clamped, const float *__restrict__ dcolours,
                                                                   float *__restrict__ gsh_out, Layout G, float *__restrict__ gvec_out)
{
    constexpr int K = sh_count(D);
    extern __shared__ float lds[];
    const int64_t row0 = (int64_t)blockIdx.x * WAVE;
    const int nrows = (int)(P - row0 < WAVE ? P - row0 : WAVE);
    const int lane = threadIdx.x;
    const bool live = lane < nrows;
    const int64_t i = row0 + lane;
    if (L.path != PATH_DIRECT) {
        stage_in(sh, L, row0, nrows, lds);
        __syncthreads();
    }
    float gsh[K][3];
    if (live) {
        float reg[K][3];
        load_row<K>(sh, L, i, lds, reg);
        const float *vp = (means ? means : dirs) + 3 * i;
        const float vec[3] = {vp[0], vp[1], vp[2]};
        float cam[3] = {0.0f, 0.0f, 0.0f};
        uint8_t cl[3] = {0, 0, 0};
        if (means) {
            cam[0] = campos[0]; cam[1] = campos[1]; cam[2] = campos[2];
            cl[0] = clamped[3 * i + 0]; cl[1] = clamped[3 * i + 1]; cl[2] = clamped[3 * i + 2];
        }
        const float dc[3] = {dcolours[3 * i + 0], dcolours[3 * i + 1], dcolours[3 * i + 2]};
        float gvec[3];
        gaussian_backward<D>(reg, vec, cam, means != nullptr, cl, dc, gsh, gvec);
        if (gvec_out) { gvec_out[3 * i + 0] = gvec[0]; gvec_out[3 * i + 1] = gvec[1]; gvec_out[3 * i + 2] = gvec[2]; }
    }
    if (!gsh_out) return;
    if (G.path != PATH_DIRECT) {
        __syncthreads();                 // every lane has its coefficients in registers: the LDS rows are free
        if (live) {
            float *row = lds + lane * G.pad;
            const int cs = (int)G.coef, hs = (int)G.chan;
#pragma unroll
            for (int k = 0; k < K; ++k)
                _Pragma("unroll") for (int c = 0; c < 3; ++c) row[k * cs + c * hs] = gsh[k][c];
            for (int k = K; k < M; ++k)
                _Pragma("unroll") for (int c = 0; c < 3; ++c) row[k * cs + c * hs] = 0.0f;
        }
        __syncthreads();
        stage_out(gsh_out, G, row0, nrows, lds);
    } else if (live) {
        float *row = gsh_out + i * G.row;
#pragma unroll
        for (int k = 0; k < K; ++k)
            _Pragma("unroll") for (int c = 0; c < 3; ++c) row[k * G.coef + c * G.chan] = gsh[k][c];
        for (int k = K; k < M; ++k)
            _Pragma("unroll") for (int c = 0; c < 3; ++c) row[k * G.coef + c * G.chan] = 0.0f;
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// How `count` coefficients of a row are reached.  dense_only: the staged path must cover a whole dense row (the gradient's: every
// float of the span is an entry, so storing the span stores nothing else).
Layout make_layout(const float *base, int count, int64_t coef, int64_t chan, int64_t row, bool dense_only)
{
    Layout L = {coef, chan, row, 0, 1, PATH_DIRECT, 0, 0};
    if (coef <= 0 || chan <= 0 || coef > MAX_SPAN || chan > MAX_SPAN) return L;
    const int64_t span = (int64_t)(count - 1) * coef + 2 * chan + 1;
    if (span > MAX_SPAN) return L;
    if (dense_only && (!((coef == 3 && chan == 1) || (coef == 1 && chan == count)) || row < span)) return L;
    L.span = (int)span;
    L.pad = (int)span | 1;
    L.path = (row == span && span % 4 == 0 && aligned16(base)) ? PATH_STAGED_VEC : PATH_STAGED;
    const int step = L.path == PATH_STAGED_VEC ? 4 * WAVE : WAVE;
    L.step_rows = step / L.span;
    L.step_off = step % L.span;
    return L;
}

size_t lds_bytes(const Layout &a, const Layout &b)
{
    const int pa = a.path != PATH_DIRECT ? a.pad : 0, pb = b.path != PATH_DIRECT ? b.pad : 0;
    return (size_t)WAVE * (pa > pb ? pa : pb) * sizeof(float);
}

int check_common(const char *who, gpcc_ctx *ctx, int P, int degree, const float *sh, const float *means3D, const float *campos, const float *dirs)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "%s: null context", who);
    if (P < 0) return fail(GPCC_ERR_ARG, "%s: P = %d", who, P);
    if (degree < 0 || degree > 4) return fail(GPCC_ERR_ARG, "%s: degree %d (served: 0..4)", who, degree);
    if (P == 0) return GPCC_OK;
    if (!sh) return fail(GPCC_ERR_ARG, "%s: null coefficients", who);
    if ((means3D != nullptr) == (dirs != nullptr)) return fail(GPCC_ERR_ARG, "%s: exactly one of means3D and dirs", who);
    if (means3D && !campos) return fail(GPCC_ERR_ARG, "%s: means3D without campos", who);
    return GPCC_OK;
}

}  // namespace

extern "C" int gsr_sh_forward(gpcc_ctx *ctx, int P, int degree, const float *sh, int64_t coef_stride, int64_t chan_stride, int64_t row_stride,
                              const float *means3D, const float *campos, const float *dirs, float *colors, uint8_t *clamped, void *stream)
{
    GP_TRY(check_common("gsr_sh_forward", ctx, P, degree, sh, means3D, campos, dirs));
    if (P == 0) return GPCC_OK;
    if (!colors || (means3D && !clamped)) return fail(GPCC_ERR_ARG, "gsr_sh_forward: null output");
    const Layout L = make_layout(sh, sh_count(degree), coef_stride, chan_stride, row_stride, false);
    const Layout none = {0, 0, 0, 0, 1, PATH_DIRECT, 0, 0};
    HIP_TRY(hipSetDevice(ctx->device));
    const unsigned groups = (unsigned)cdiv(P, WAVE);
    const size_t lds = lds_bytes(L, none);
    hipStream_t st = (hipStream_t)stream;
    switch (degree) {
    case 0: k_sh_fwd<0><<<groups, WAVE, lds, st>>>(P, sh, L, means3D, campos, dirs, colors, clamped); break;
    case 1: k_sh_fwd<1><<<groups, WAVE, lds, st>>>(P, sh, L, means3D, campos, dirs, colors, clamped); break;
    case 2: k_sh_fwd<2><<<groups, WAVE, lds, st>>>(P, sh, L, means3D, campos, dirs, colors, clamped); break;
    case 3: k_sh_fwd<3><<<groups, WAVE, lds, st>>>(P, sh, L, means3D, campos, dirs, colors, clamped); break;
    default: k_sh_fwd<4><<<groups, WAVE, lds, st>>>(P, sh, L, means3D, campos, dirs, colors, clamped); break;
    }
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsr_sh_backward(gpcc_ctx *ctx, int P, int degree, int M, const float *sh, int64_t coef_stride, int64_t chan_stride, int64_t row_stride,
                               const float *means3D, const float *campos, const float *dirs, const uint8_t *clamped, const float *dL_dcolors,
                               float *dL_dsh, int64_t grad_coef_stride, int64_t grad_chan_stride, int64_t grad_row_stride, float *dL_dmeans3D,
                               float *dL_ddirs, void *stream)
{
    GP_TRY(check_common("gsr_sh_backward", ctx, P, degree, sh, means3D, campos, dirs));
    if (M < sh_count(degree)) return fail(GPCC_ERR_ARG, "gsr_sh_backward: M = %d holds no degree %d", M, degree);
    if (P == 0) return GPCC_OK;
    if (!dL_dcolors || (means3D && !clamped)) return fail(GPCC_ERR_ARG, "gsr_sh_backward: null argument");
    if ((means3D && dL_ddirs) || (dirs && dL_dmeans3D)) return fail(GPCC_ERR_ARG, "gsr_sh_backward: the gradient of the vector that was not given");
    float *gvec = means3D ? dL_dmeans3D : dL_ddirs;
    if (!dL_dsh && !gvec) return GPCC_OK;
    const Layout L = make_layout(sh, sh_count(degree), coef_stride, chan_stride, row_stride, false);
    Layout G = {0, 0, 0, 0, 1, PATH_DIRECT, 0, 0};
    if (dL_dsh) G = make_layout(dL_dsh, M, grad_coef_stride, grad_chan_stride, grad_row_stride, true);
    HIP_TRY(hipSetDevice(ctx->device));
    const unsigned groups = (unsigned)cdiv(P, WAVE);
    const size_t lds = lds_bytes(L, G);
    hipStream_t st = (hipStream_t)stream;
#define SH_BWD(D) k_sh_bwd<D><<<groups, WAVE, lds, st>>>(P, M, sh, L, means3D, campos, dirs, clamped, dL_dcolors, dL_dsh, G, gvec)
    switch (degree) {
    case 0: SH_BWD(0); break;
    case 1: SH_BWD(1); break;
    case 2: SH_BWD(2); break;
    case 3: SH_BWD(3); break;
    default: SH_BWD(4); break;
    }
#undef SH_BWD
    LAUNCH_CHECK();
    return GPCC_OK;
}
