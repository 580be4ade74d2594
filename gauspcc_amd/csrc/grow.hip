// grow.hip -- anchor growing (HAC-family densification, e.g. HAC/scene/gaussian_model.py:823-911):
//   gpcc_scatter_max  torch_scatter.scatter_max in row form (one index per row of C columns), deterministic
//   gpcc_grow_voxels  one grid level of anchor_growing: quantise, unique voxels, drop the anchored ones, per-voxel feature maximum
// The contracts are in include/gauspcc.h.
//
// The maximum.  The contract picks, per (slot, column), the largest value (a NaN above everything, -0.0 equal to +0.0) and among equal
// values the smallest row j.  That is the maximum of a total order, so it is encoded as one 64-bit integer per element:
//   key = ord(value) << 32 | (2^32 - 1 - j),  ord = the float's order as an unsigned word (every NaN the top word, both zeros one word)
// and any reduction order gives the same winner.  The rows are sorted by destination first (the stable radix_sort_u64), so a
// destination's rows are one run; k_segmax gives each lane group GR consecutive sorted rows, reduces each run in registers and adds
// one integer atomicMax per run and column.  A run longer than GR is split between groups whose partial maxima meet in that atomicMax:
// at most len / GR + 2 of them per word, so one destination holding every row costs what evenly spread rows cost.  No float atomics;
// the value written is read back from src[winner], so its bits (-0.0, a NaN's payload) are those of the winning row.
//
// gpcc_grow_voxels, all on the caller's stream, two read-backs:
//   k_quant            g = rint(x * inv) per axis, the candidates' integer box and an invalid-input flag (integer atomics)
//   read-back 1        box and flag: a bad input returns GPCC_ERR_ARG before anything is written; the box picks the key path
//   keys + sort        span <= 2^21 per axis: one packed key of (g - lo) (only the bits the spans need; anchors outside the box get a
//                      sentinel and sort last); otherwise two stable sorts, z then (x, y), of the sign-flipped coordinates
//   k_mark             first row of each voxel; kept = no anchor voxel equal to it (binary search in the sorted anchor voxels)
//   scans, k_uk, k_segid   output rank of each kept voxel and, per sorted row, the output row it feeds (or none)
//   read-back 2        U, the number of new anchors; then the caller's allocator gives the outputs
//   k_emit_anchor, k_segmax, k_final   anchors (float)g * size, the features' maximum
#include "primitives.hpp"

#include <float.h>
#include <limits.h>

using namespace gpcc;

namespace {

constexpr int TB = 256;
constexpr int GR = 256;                 // sorted rows one lane group walks in k_segmax
constexpr uint64_t SKIP = ~0ull;        // segment id of a row that feeds no output
constexpr int H_LO = 0, H_HI = 3, H_BAD = 6, H_NVALID = 7, H_COUNT = 8, H_WORDS = 16;

__device__ __forceinline__ uint32_t ord_word(float v)
{
    if (v != v) return 0xFFFFFFFFu;
    const uint32_t b = v == 0.0f ? 0u : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint64_t elem_key(float v, uint32_t j) { return (uint64_t)ord_word(v) << 32 | (uint64_t)(0xFFFFFFFFu - j); }

// ------------------------------------------------------------------ the segmented maximum (shared by both exports)
// seg[i]: destination of sorted row i (SKIP: none), perm[i]: its row j, tab row = rows ? rows[j] : j.  Lanes: 2^lw columns times
// 64 >> lw groups; blockIdx.y = column tile.
__global__ __launch_bounds__(TB) void k_segmax(const uint64_t *__restrict__ seg, const uint32_t *__restrict__ perm, const int64_t *__restrict__ rows,
                                               const float *__restrict__ tab, int64_t C, int64_t M, int lw, unsigned long long *__restrict__ buf)
{
    const int lane = threadIdx.x & 63, W = 1 << lw;
    const int64_t wave = ((int64_t)blockIdx.x * TB + threadIdx.x) >> 6;
    const int64_t g = wave * (64 >> lw) + (lane >> lw);
    const int64_t c = (int64_t)blockIdx.y * W + (lane & (W - 1));
    const int64_t b = g * GR;
    if (b >= M || c >= C) return;
    const int64_t e = b + GR < M ? b + GR : M;
    uint64_t cur = SKIP;
    unsigned long long best = 0;
    for (int64_t i = b; i < e; i += 8) {
        uint64_t s[8];
        uint32_t j[8];
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool in = i + k < e;
            s[k] = in ? seg[i + k] : SKIP;
            j[k] = in ? perm[i + k] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t r = rows ? rows[j[k]] : (int64_t)j[k];
            v[k] = s[k] != SKIP ? tab[r * C + c] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (s[k] != cur) {
                if (cur != SKIP) atomicMax(&buf[cur * C + c], best);
                cur = s[k];
                best = 0;
            }
            if (s[k] != SKIP) { const unsigned long long q = elem_key(v[k], j[k]); best = q > best ? q : best; }
        }
    }
    if (cur != SKIP) atomicMax(&buf[cur * C + c], best);
}

// out[s, c] and arg[s, c] from the winners.  init: include-self initial values (may alias out); init == nullptr: torch_scatter's own
// output, initialised to -FLT_MAX and then masked to 0 where it still equals -FLT_MAX.  buf == nullptr: every slot is empty.
__global__ __launch_bounds__(TB) void k_final(const unsigned long long *__restrict__ buf, int64_t total, int64_t C, int64_t M, const float *__restrict__ tab,
                                              const int64_t *__restrict__ rows, const float *init, float *out, int64_t *__restrict__ arg)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= total) return;
    const unsigned long long k = buf ? buf[i] : 0ull;
    int64_t j = M;
    float v = init ? init[i] : -FLT_MAX;
    if (k) {
        const int64_t w = (int64_t)(0xFFFFFFFFu - (uint32_t)k), c = i % C;
        const float x = tab[(rows ? rows[w] : w) * C + c];
        if (x != x || !(v != v || v > x)) { v = x; j = w; }
    }
    if (!init && v == -FLT_MAX) v = 0.0f;
    out[i] = v;
    if (arg) arg[i] = j;
}

// ------------------------------------------------------------------ gpcc_scatter_max
// flag when an index leaves [0, S); the keys and values for the sort
__global__ __launch_bounds__(TB) void k_scatter_keys(const int64_t *__restrict__ index, int64_t M, int64_t S, uint64_t *__restrict__ key,
                                                     uint32_t *__restrict__ val, int *__restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    const int64_t s = index[i];
    if (s < 0 || s >= S) atomicOr(&hdr[H_BAD], 1);
    key[i] = (uint64_t)s;
    val[i] = (uint32_t)i;
}

__global__ void k_hdr_init(int *hdr)
{
    const int t = threadIdx.x;
    if (t < H_WORDS) hdr[t] = t < H_HI ? INT_MAX : (t < H_BAD ? INT_MIN : 0);
}

int bit_width(uint64_t v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

int log2_lanes(int64_t C)
{
    int lw = 0;
    while ((1 << lw) < C && lw < 6) ++lw;
    return lw;
}

int launch_segmax(hipStream_t st, const uint64_t *seg, const uint32_t *perm, const int64_t *rows, const float *tab, int64_t C, int64_t M,
                  unsigned long long *buf)
{
    const int lw = log2_lanes(C);
    const int64_t groups = cdiv(M, GR), waves = cdiv(groups, 64 >> lw), tiles = cdiv(C, 1 << lw);
    if (tiles > 65535) return fail(GPCC_ERR_ARG, "grow: %lld columns", (long long)C);
    k_segmax<<<dim3((unsigned)cdiv(waves, TB / 64), (unsigned)tiles), TB, 0, st>>>(seg, perm, rows, tab, C, M, lw, buf);
    LAUNCH_CHECK();
    return GPCC_OK;
}

int read_hdr(gpcc_ctx *ctx, hipStream_t st, const int *hdr, int words, int **host)
{
    GP_TRY(ctx->hstage.reserve(64));
    *host = reinterpret_cast<int *>(ctx->hstage.p);
    HIP_TRY(hipMemcpyAsync(*host, hdr, 4 * (size_t)words, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}

// ------------------------------------------------------------------ gpcc_grow_voxels
struct Box { int lo[3], hi[3]; };

// g = rint(x * inv) as int32 (round half to even; x * inv one rounded product); bad: non-finite or outside int32, or a row outside
// [0, nrows).  box: the integer box of the points (null for the anchors).
__global__ __launch_bounds__(TB) void k_quant(const float *__restrict__ xyz, int64_t n, float inv, const int64_t *__restrict__ rows, int64_t nrows,
                                              int4 *__restrict__ q, int *__restrict__ hdr, int with_box)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    bool bad = false;
    if (i < n) {
        int g[3];
        for (int a = 0; a < 3; ++a) {
            const float r = rintf(xyz[3 * i + a] * inv);
            const bool ok = r >= -2147483648.0f && r < 2147483648.0f;
            bad |= !ok;
            g[a] = ok ? (int)r : 0;
            lo[a] = g[a];
            hi[a] = g[a];
        }
        if (rows) { const int64_t r = rows[i]; bad |= r < 0 || r >= nrows; }
        q[i] = make_int4(g[0], g[1], g[2], 0);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&hdr[H_BAD], 1);
    if (!with_box) return;
    for (int a = 0; a < 3; ++a) {
        for (int m = 32; m > 0; m >>= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], m)); hi[a] = max(hi[a], __shfl_xor(hi[a], m)); }
    }
    if ((threadIdx.x & 63) == 0 && lo[0] != INT_MAX) {
        for (int a = 0; a < 3; ++a) { atomicMin(&hdr[H_LO + a], lo[a]); atomicMax(&hdr[H_HI + a], hi[a]); }
    }
}

// packed key of (g - lo) with bz, by bits for z and y; anchors (sentinel != 0) outside the box get the sentinel and are not counted
__global__ __launch_bounds__(TB) void k_keys_packed(const int4 *__restrict__ q, int64_t n, Box box, int by, int bz, uint64_t sentinel,
                                                    uint64_t *__restrict__ key, uint32_t *__restrict__ val, int *__restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    bool in = false;
    if (i < n) {
        const int4 g = q[i];
        in = g.x >= box.lo[0] && g.x <= box.hi[0] && g.y >= box.lo[1] && g.y <= box.hi[1] && g.z >= box.lo[2] && g.z <= box.hi[2];
        const uint64_t k = (uint64_t)((uint32_t)g.x - (uint32_t)box.lo[0]) << (by + bz) | (uint64_t)((uint32_t)g.y - (uint32_t)box.lo[1]) << bz |
                           (uint64_t)((uint32_t)g.z - (uint32_t)box.lo[2]);
        key[i] = in ? k : sentinel;
        val[i] = (uint32_t)i;
    }
    if (sentinel) {
        const uint64_t m = __ballot(in);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&hdr[H_NVALID], __popcll(m));
    }
}

__device__ __forceinline__ uint32_t flip(int v) { return (uint32_t)v ^ 0x80000000u; }

// general path: pass 0 keys z (values = the row), pass 1 keys (x, y) of the rows in the order pass 0 left (values carried)
__global__ __launch_bounds__(TB) void k_keys_axis(const int4 *__restrict__ q, int64_t n, const uint32_t *__restrict__ order, uint64_t *__restrict__ key,
                                                  uint32_t *__restrict__ val, int *__restrict__ hdr, int count)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (!order) {
        key[i] = flip(q[i].z);
        val[i] = (uint32_t)i;
    } else {
        const int4 g = q[order[i]];
        key[i] = (uint64_t)flip(g.x) << 32 | flip(g.y);
    }
    if (count && i == 0) atomicAdd(&hdr[H_NVALID], (int)n);
}

__global__ __launch_bounds__(TB) void k_gather4(const int4 *__restrict__ q, const uint32_t *__restrict__ order, int64_t n, int4 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) out[i] = q[order[i]];
}

__device__ __forceinline__ bool lex_less(int4 a, int4 b) { return a.x != b.x ? a.x < b.x : (a.y != b.y ? a.y < b.y : a.z < b.z); }
__device__ __forceinline__ bool same(int4 a, int4 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

__global__ __launch_bounds__(TB) void k_mark(const int4 *__restrict__ cs, int64_t M, const int4 *__restrict__ as, const int *__restrict__ hdr,
                                             uint32_t *__restrict__ u, uint32_t *__restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    const int4 g = cs[i];
    const bool first = i == 0 || !same(g, cs[i - 1]);
    bool hit = false;
    if (first) {
        int64_t lo = 0, hi = hdr[H_NVALID];   // first anchor voxel not below g
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (lex_less(as[mid], g)) lo = mid + 1;
            else hi = mid;
        }
        hit = lo < hdr[H_NVALID] && same(as[lo], g);
    }
    u[i] = first;
    keep[i] = first && !hit;
}

// uk[unique rank] = output row of the voxel or -1; the count of kept voxels into the header
__global__ __launch_bounds__(TB) void k_uk(const uint32_t *__restrict__ u, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ ru,
                                           const uint32_t *__restrict__ rk, int64_t M, int *__restrict__ uk, int *__restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    if (u[i]) uk[ru[i]] = keep[i] ? (int)rk[i] : -1;
    if (i == M - 1) hdr[H_COUNT] = (int)(rk[i] + keep[i]);
}

__global__ __launch_bounds__(TB) void k_segid(const uint32_t *__restrict__ u, const uint32_t *__restrict__ ru, const int *__restrict__ uk, int64_t M,
                                              uint64_t *__restrict__ seg)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M) return;
    const int o = uk[ru[i] + u[i] - 1];
    seg[i] = o < 0 ? SKIP : (uint64_t)o;
}

__global__ __launch_bounds__(TB) void k_emit_anchor(const int4 *__restrict__ cs, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ rk,
                                                    int64_t M, float size, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= M || !keep[i]) return;
    const int4 g = cs[i];
    const int64_t o = rk[i];
    out[3 * o] = (float)g.x * size;
    out[3 * o + 1] = (float)g.y * size;
    out[3 * o + 2] = (float)g.z * size;
}

// sort (key, val) on `bits`; the sorted arrays end up in *k, *v
int sort_pairs(gpcc_ctx *ctx, hipStream_t st, uint64_t **k, uint64_t **kt, uint32_t **v, uint32_t **vt, int64_t n, int bits, uint32_t *hist)
{
    return radix_sort_u64(ctx, st, k, kt, v, vt, n, bits < 1 ? 1 : bits, hist);
}

}  // namespace

// Workspace (one alloc call): 24 m bytes for the sort, 8 S C for the maxima, the sort's digit table and 256 bytes.
extern "C" int gpcc_scatter_max(gpcc_ctx *ctx, const float *src, const int64_t *index, int64_t m, int64_t c, int64_t dim_size, int include_self,
                                float *out, int64_t *arg, gsr_alloc_fn alloc, void *alloc_user, void *stream)
{
    if (!ctx) return fail(GPCC_ERR_ARG, "gpcc_scatter_max: null context");
    if (m < 0 || m >= ((int64_t)1 << 31)) return fail(GPCC_ERR_ARG, "gpcc_scatter_max: m = %lld outside [0, 2^31)", (long long)m);
    if (c < 1 || dim_size < 0 || (dim_size > 0 && c > (((int64_t)1 << 40) / dim_size)))
        return fail(GPCC_ERR_ARG, "gpcc_scatter_max: c = %lld, dim_size = %lld", (long long)c, (long long)dim_size);
    if (m > 0 && dim_size == 0) return fail(GPCC_ERR_ARG, "gpcc_scatter_max: an index outside [0, 0)");
    if (dim_size == 0) return GPCC_OK;
    if (!out || (m > 0 && (!src || !index || !alloc))) return fail(GPCC_ERR_ARG, "gpcc_scatter_max: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = dim_size * c;
    if (m == 0) {
        k_final<<<(unsigned)cdiv(total, TB), TB, 0, st>>>(nullptr, total, c, 0, nullptr, nullptr, include_self ? out : nullptr, out, arg);
        LAUNCH_CHECK();
        return GPCC_OK;
    }
    int *hdr;
    uint64_t *ka;
    uint32_t *va, *hist;
    unsigned long long *buf;
    GP_TRY(caller_block(alloc, alloc_user, "gpcc_scatter_max", [&](Carver &c) {
        hdr = c.take<int>(H_WORDS); ka = c.take<uint64_t>(2 * m); va = c.take<uint32_t>(2 * m); hist = c.take<uint32_t>(radix_sort_hist_words(m));
        buf = c.take<unsigned long long>(total);
    }));
    uint64_t *kb = ka + m;
    uint32_t *vb = va + m;

    k_hdr_init<<<1, 64, 0, st>>>(hdr);
    LAUNCH_CHECK();
    k_scatter_keys<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(index, m, dim_size, ka, va, hdr);
    LAUNCH_CHECK();
    int *h = nullptr;
    GP_TRY(read_hdr(ctx, st, hdr, H_WORDS, &h));
    if (h[H_BAD]) return fail(GPCC_ERR_ARG, "gpcc_scatter_max: an index outside [0, %lld)", (long long)dim_size);
    uint64_t *k0 = ka, *k1 = kb;
    uint32_t *v0 = va, *v1 = vb;
    GP_TRY(sort_pairs(ctx, st, &k0, &k1, &v0, &v1, m, bit_width((uint64_t)(dim_size - 1)), hist));
    HIP_TRY(hipMemsetAsync(buf, 0, 8 * (size_t)total, st));
    GP_TRY(launch_segmax(st, k0, v0, nullptr, src, c, m, buf));
    k_final<<<(unsigned)cdiv(total, TB), TB, 0, st>>>(buf, total, c, m, src, nullptr, include_self ? out : nullptr, out, arg);
    LAUNCH_CHECK();
    return GPCC_OK;
}

// Allocations, in this order: (1) the workspace, at most 84 m + 56 n bytes plus the sort's digit table and 1 KiB; after the second
// read-back and only when U > 0, (2) the outputs, anchors (U, 3) at offset 0 and features (U, c) at align256(12 U), and (3) 8 U c bytes of
// per-column maxima.
extern "C" int gpcc_grow_voxels(gpcc_ctx *ctx, const float *xyz, int64_t m, const int64_t *rows, const float *feats, int64_t nrows, int64_t c,
                                const float *anchors, int64_t n, float inv, float size, int64_t *count_out, gsr_alloc_fn alloc, void *alloc_user,
                                void *stream)
{
    if (!ctx || !count_out) return fail(GPCC_ERR_ARG, "gpcc_grow_voxels: null context or count");
    *count_out = 0;
    if (m < 0 || m >= ((int64_t)1 << 31) || n < 0 || n >= ((int64_t)1 << 31))
        return fail(GPCC_ERR_ARG, "gpcc_grow_voxels: m = %lld, n = %lld outside [0, 2^31)", (long long)m, (long long)n);
    if (c < 1 || nrows < 0 || (!rows && nrows < m)) return fail(GPCC_ERR_ARG, "gpcc_grow_voxels: c = %lld, %lld feature rows", (long long)c, (long long)nrows);
    if (m == 0 && n == 0) return GPCC_OK;
    if ((m > 0 && (!xyz || !feats)) || (n > 0 && !anchors) || !alloc) return fail(GPCC_ERR_ARG, "gpcc_grow_voxels: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;

    const int64_t mx = m > n ? m : n;
    int *hdr, *uk;
    int4 *gq, *aq, *cs, *as;
    uint64_t *ka, *seg;
    uint32_t *va, *hist, *u, *keep, *ru, *rk;
    GP_TRY(caller_block(alloc, alloc_user, "gpcc_grow_voxels", [&](Carver &c) {
        hdr = c.take<int>(H_WORDS); gq = c.take<int4>(m); aq = c.take<int4>(n); cs = c.take<int4>(m); as = c.take<int4>(n);
        ka = c.take<uint64_t>(2 * mx); va = c.take<uint32_t>(2 * mx); hist = c.take<uint32_t>(radix_sort_hist_words(mx));
        u = c.take<uint32_t>(m); keep = c.take<uint32_t>(m); ru = c.take<uint32_t>(m); rk = c.take<uint32_t>(m);
        uk = c.take<int>(m); seg = c.take<uint64_t>(m);
    }));
    uint64_t *kb = ka + mx;
    uint32_t *vb = va + mx;

    k_hdr_init<<<1, 64, 0, st>>>(hdr);
    LAUNCH_CHECK();
    if (m > 0) k_quant<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(xyz, m, inv, rows, nrows, gq, hdr, 1);
    if (n > 0) k_quant<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(anchors, n, inv, nullptr, 0, aq, hdr, 0);
    LAUNCH_CHECK();
    int *h = nullptr;
    GP_TRY(read_hdr(ctx, st, hdr, H_WORDS, &h));   // synchronisation 1
    if (h[H_BAD]) return fail(GPCC_ERR_ARG, "gpcc_grow_voxels: a non-finite coordinate, one outside int32 after rounding, or a row outside [0, %lld)",
                              (long long)nrows);
    if (m == 0) return GPCC_OK;
    Box box;
    int bits[3];
    bool packed = true;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = h[H_LO + a];
        box.hi[a] = h[H_HI + a];
        const int64_t span = (int64_t)box.hi[a] - box.lo[a];
        packed &= span < ((int64_t)1 << 21);
        bits[a] = bit_width((uint64_t)span);
    }

    uint32_t *cperm = nullptr;
    if (packed) {
        const int tb = bits[0] + bits[1] + bits[2];
        uint64_t *k0 = ka, *k1 = kb;
        uint32_t *v0 = va, *v1 = vb;
        if (n > 0) {
            k_keys_packed<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(aq, n, box, bits[1], bits[2], (uint64_t)1 << tb, ka, va, hdr);
            LAUNCH_CHECK();
            GP_TRY(sort_pairs(ctx, st, &k0, &k1, &v0, &v1, n, tb + 1, hist));
            k_gather4<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(aq, v0, n, as);
            LAUNCH_CHECK();
        }
        k0 = ka; k1 = kb; v0 = va; v1 = vb;
        k_keys_packed<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(gq, m, box, bits[1], bits[2], 0, ka, va, hdr);
        LAUNCH_CHECK();
        GP_TRY(sort_pairs(ctx, st, &k0, &k1, &v0, &v1, m, tb, hist));
        cperm = v0;
    } else {
        for (int side = 0; side < 2; ++side) {   // anchors first: the candidates' permutation must survive in the shared buffers
            const int64_t cnt = side == 0 ? n : m;
            if (cnt == 0) continue;
            const int4 *q = side == 0 ? aq : gq;
            uint64_t *k0 = ka, *k1 = kb;
            uint32_t *v0 = va, *v1 = vb;
            k_keys_axis<<<(unsigned)cdiv(cnt, TB), TB, 0, st>>>(q, cnt, nullptr, k0, v0, hdr, side == 0);
            LAUNCH_CHECK();
            GP_TRY(sort_pairs(ctx, st, &k0, &k1, &v0, &v1, cnt, 32, hist));
            k_keys_axis<<<(unsigned)cdiv(cnt, TB), TB, 0, st>>>(q, cnt, v0, k0, nullptr, hdr, 0);
            LAUNCH_CHECK();
            GP_TRY(sort_pairs(ctx, st, &k0, &k1, &v0, &v1, cnt, 64, hist));
            if (side == 0) {
                k_gather4<<<(unsigned)cdiv(n, TB), TB, 0, st>>>(aq, v0, n, as);
                LAUNCH_CHECK();
            } else {
                cperm = v0;
            }
        }
    }
    k_gather4<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(gq, cperm, m, cs);
    LAUNCH_CHECK();
    k_mark<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(cs, m, as, hdr, u, keep);
    LAUNCH_CHECK();
    GP_TRY(exclusive_scan_pair_u32(ctx, st, u, ru, keep, rk, m));
    k_uk<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(u, keep, ru, rk, m, uk, hdr);
    LAUNCH_CHECK();
    k_segid<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(u, ru, uk, m, seg);
    LAUNCH_CHECK();
    GP_TRY(read_hdr(ctx, st, hdr, H_WORDS, &h));   // synchronisation 2
    const int64_t U = h[H_COUNT];
    GP_TRY(device_error_check(ctx));
    *count_out = U;
    if (U == 0) return GPCC_OK;
    const size_t feat_at = align256(12 * U) / sizeof(float);   // the features' segment ends the block unpadded
    float *anchor_out;
    unsigned long long *buf;
    GP_TRY(caller_alloc(alloc, alloc_user, sizeof(float) * (feat_at + U * c), &anchor_out, "gpcc_grow_voxels: outputs"));
    GP_TRY(caller_alloc(alloc, alloc_user, sizeof(unsigned long long) * U * c, &buf, "gpcc_grow_voxels: maxima"));
    float *feat_out = anchor_out + feat_at;
    HIP_TRY(hipMemsetAsync(buf, 0, 8 * (size_t)(U * c), st));
    k_emit_anchor<<<(unsigned)cdiv(m, TB), TB, 0, st>>>(cs, keep, rk, m, size, anchor_out);
    LAUNCH_CHECK();
    GP_TRY(launch_segmax(st, seg, cperm, rows, feats, c, m, buf));
    k_final<<<(unsigned)cdiv(U * c, TB), TB, 0, st>>>(buf, U * c, c, m, feats, rows, nullptr, feat_out, nullptr);
    LAUNCH_CHECK();
    return GPCC_OK;
}
