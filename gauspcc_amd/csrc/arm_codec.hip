// arm_codec.hip -- the bitstream of CAT-3DGS's tri-plane latents under its auto-regressive model (CAT-3DGS/scene/gaussian_model.py:
// encode_triplane / decode_triplane; the format is this library's own):
//   gsac_arm_encode     every level of one plane: alphabet, (mu, scale) per latent, the chunked coder -> bytes and chunk byte counts
//   gsac_arm_decode     the wavefront decoder: one workgroup per channel, one lane and one coder state per strip of columns
//   gsac_arm_cdf_rows   the integer CDF rows themselves (tests, two-step callers)
//
// Model.  (mu, s) of latent (c, h, w) are what gsarm_rate_forward returns (arm_dev.hpp: the same device functions), quantised as the
// reference's RangeCoder does: mu_q = rint(16 mu) / 16, s_q = max(rint(16 s) / 16, 1 / 16).  Alphabet: A = ceil(max |y|) + 2, L = 2 A + 1
// symbols, index i = y + A.  A row has L + 1 entries: e_0 = 0, e_L = 1, e_j = F(j - A - 0.5) with the rate term's Laplace CDF F in
// float32, integerised as the attribute coder does: rint(e_j (65536 - L)) + j modulo 2^16 (every symbol keeps a count).
//
// Chunks.  A channel's plane is cut into K = ceil(W / S) vertical strips of S columns; strip k of channel c is one chunk (symbols by
// row, then by column inside the strip), chunks in (channel, strip) order; a chunk's bytes are the torchac-compatible carry-less
// stream of its symbols (rangecoder.hip's lane-per-chunk encoder; == gsac_host_encode_u16 on the chunk's rows).
//
// Encode is parallel: one pass finds A per level, one pass (a lane per latent) evaluates the MLP and writes the two integers the
// coder needs in chunk order, the lane-per-chunk coder does the rest.
//
// Decode is serial in the causal context and parallel across strips and channels.  A latent needs rows h - 2, h - 1 at columns
// w - 2 .. w + 2 and row h at w - 2, w - 1.  At step T lane k decodes the whole segment of row h = (T - k) / 2 when T - k is even
// and 0 <= h < H: the strip to its right is one row behind, the strip to its left one row ahead, so every context entry was decoded
// in an earlier step or earlier in the lane's own segment.  K + 2 H - 2 steps, a workgroup barrier behind each; decoded rows are
// exchanged through the output plane itself (global memory: written before the barrier, read behind it by lanes of the same
// workgroup).  No grid barrier, no waiting between workgroups, no spin loop; the step loop's bounds are workgroup-uniform.
// Inside a segment the 5 x 5 window slides in registers: two loads per latent (the new column of rows h - 2 and h - 1), and these
// rows are complete before the segment starts; the byte window is three words in registers refilled a word ahead: no load sits
// between two dependent symbols.
// The symbol comes from the closed-form inverse of the Laplace CDF, then a bounded search (gallop + bisection, at most ~2 log2 L
// entries) against the integer entries evaluated in registers: there is no table in memory.
// Bounds: bytes past a chunk's count read as zero, the symbol index stays in [0, L - 1], every store is to the lane's own segment:
// a wrong payload decodes to some grid and touches nothing outside its buffers.
#include "arm_dev.hpp"
#include "coder_tail.hpp"
#include "primitives.hpp"
#include "rangecoder_dev.hpp"

using namespace gpcc;
using namespace gpcc::armdev;

namespace {

constexpr int A_MAX = 1024;               // the reference's MAX_AC_MAX_VAL
constexpr int S_MIN = 4;
constexpr int K_MAX = 1024;               // strips of a channel: lanes of one workgroup
constexpr float QSTEP = 16.f, QINV = 0.0625f;

struct Lv {
    float *y;                             // the level's latents (encode: read; decode: written)
    int C, H, W, S, K, A;
    int n;                                // C * H * W
    int tile0;                            // encode: the level's first tile of latents in the launch
    uint32_t chunk0;                      // the level's first chunk in the call's chunk list
    uint32_t word0;                       // encode: the level's first coder word
};

__device__ __forceinline__ float quant_mu(float mu) { return __builtin_rintf(mu * QSTEP) * QINV; }
__device__ __forceinline__ float quant_scale(float s) { return fmaxf(__builtin_rintf(s * QSTEP) * QINV, QINV); }

// entry j (0 <= j < L) of the integer row of (mu_q, s_q); entry L is 2^16
__device__ __forceinline__ uint32_t cdf_entry(float mu_q, float s_q, int A, int L, int j)
{
    if (j == 0) return 0u;
    const float t = (float)(j - A) - 0.5f;
    return (uint32_t)((int)__builtin_rintf(laplace_cdf(t - mu_q, s_q) * (float)(65536 - L)) + j) & 0xFFFFu;
}

__global__ __launch_bounds__(256) void k_arm_rows(const float *__restrict__ mu, const float *__restrict__ scale, int64_t n, int A, uint16_t *__restrict__ rows)
{
    const int L = 2 * A + 1, lp = L + 1;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n * lp) return;
    const int64_t r = q / lp;
    const int j = (int)(q - r * lp);
    rows[q] = j == L ? (uint16_t)0 : (uint16_t)cdf_entry(mu[r], scale[r], A, L, j);
}

// per level: the bits of max |y| (non-negative floats order as their bits) and whether a latent is not an integer
__global__ __launch_bounds__(256) void k_arm_absmax(const Lv *__restrict__ lv, int n_levels, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t red[2];
    for (int v = 0; v < n_levels; ++v) {
        const float *y = lv[v].y;
        const int n = lv[v].n;
        uint32_t mx = 0u, bad = 0u;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            const float a = fabsf(y[i]);
            bad |= (uint32_t)!(a == __builtin_rintf(a) && a < 1.0e9f);   // a NaN or an infinity is no integer either
            mx = max(mx, a == a ? __float_as_uint(a) : 0x7F800000u);
        }
        if (threadIdx.x == 0) { red[0] = 0u; red[1] = 0u; }
        __syncthreads();
        atomicMax(&red[0], mx);
        atomicOr(&red[1], bad);
        __syncthreads();
        if (threadIdx.x == 0) { atomicMax(&stats[2 * v], red[0]); atomicOr(&stats[2 * v + 1], red[1]); }
        __syncthreads();
    }
}

// encode pre-pass: a lane per latent; the symbol's (low | (high - 1) << 16) word goes to its place in chunk order
template <class N>
__global__ __launch_bounds__(N::TB) void k_arm_pack(Net net, const float *__restrict__ P, const Lv *__restrict__ lv, int n_levels,
                                                    uint32_t *__restrict__ lohi, uint32_t *__restrict__ flag)
{
    int v = 0;
    while (v < n_levels - 1 && (int)blockIdx.x >= lv[v + 1].tile0) ++v;
    const Lv L = lv[v];
    const int e = ((int)blockIdx.x - L.tile0) * N::TB + (int)threadIdx.x;
    if (e >= L.n) return;
    const int nl = N::nl(net);
    float h[N::NL + 1][N::W];
    const float x = load_ctx(L.y, e, true, L.H, L.W, h[0]);
    mlp_fwd<N>(net, P, h);
    const float mu = h[nl][0], s = scale_of(h[nl][1]);
    if (!(fabsf(mu) <= 3.0e38f && fabsf(s) <= 3.0e38f)) atomicOr(flag, 1u);
    const float mu_q = quant_mu(mu), s_q = quant_scale(s);
    const int nsym = 2 * L.A + 1;
    const int i = min(max((int)x + L.A, 0), nsym - 1);   // (in range by the alphabet's definition)
    const uint32_t lo = cdf_entry(mu_q, s_q, L.A, nsym, i);
    const uint32_t hi = i == nsym - 1 ? 0x10000u : cdf_entry(mu_q, s_q, L.A, nsym, i + 1);
    const int w = e % L.W, hh = (e / L.W) % L.H, c = e / (L.W * L.H);
    const int k = w / L.S, wk = min(L.S, L.W - k * L.S);
    const uint32_t t = (uint32_t)(hh * wk + (w - k * L.S)), nch = (uint32_t)(L.C * L.K);
    lohi[(size_t)L.word0 + (size_t)t * nch + (uint32_t)(c * L.K + k)] = (lo & 0xFFFFu) | ((hi - 1u) << 16);
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// A lane's window on its chunk's bytes: big-endian words wi, wi + 1, wi + 2 in registers, zeros past the chunk's end.  The word a refill
// loads is first needed a whole word of bits later, so no load sits between one symbol and the next.
struct BitWin {
    const uint8_t *p;
    uint32_t nb, wi, w0, w1, w2;
    __device__ __forceinline__ uint32_t word(uint32_t i) const
    {
        const uint64_t o = 4ull * i;
        uint32_t v = 0u;
        if (o + 4u <= (uint64_t)nb) {
            __builtin_memcpy(&v, p + o, 4);
            v = __builtin_bswap32(v);
        } else {
            for (uint32_t b = 0; b < 4u; ++b)
                if (o + b < (uint64_t)nb) v |= (uint32_t)p[o + b] << (24u - 8u * b);
        }
        return v;
    }
    __device__ __forceinline__ void init(const uint8_t *bytes, uint32_t n) { p = bytes; nb = n; wi = 0u; w0 = word(0u); w1 = word(1u); w2 = word(2u); }
    // the 32 bits at bit position `bit` (its word is wi)
    __device__ __forceinline__ uint32_t peek(uint64_t bit) const { const uint32_t s = (uint32_t)bit & 31u; return s ? (w0 << s) | (w1 >> (32u - s)) : w0; }
    // the position moved on by fewer than 64 bits: at most two words leave
    __device__ __forceinline__ void advance(uint64_t bit)
    {
        const uint32_t want = (uint32_t)(bit >> 5);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (wi < want) { w0 = w1; w1 = w2; ++wi; w2 = word(wi + 2u); }
    }
};

template <class N, int TB>
__global__ __launch_bounds__(TB) void k_arm_decode(Net net, const float *__restrict__ P, const Lv *__restrict__ lv, int n_levels,
                                                   const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ off, const uint32_t *__restrict__ cnt)
{
    int v = 0, c = (int)blockIdx.x;
    while (v < n_levels - 1 && c >= lv[v].C) { c -= lv[v].C; ++v; }
    const Lv L = lv[v];
    // (the level's record comes in through vector loads; as scalars, the step loop's bounds are workgroup-uniform for the compiler too)
    const int H = uni(L.H), W = uni(L.W), A = uni(L.A), S = uni(L.S), K = uni(L.K), nsym = 2 * A + 1, nl = N::nl(net);
    const int k = (int)threadIdx.x;
    const bool own = k < K;
    const int w0 = k * S, w1 = min(W, w0 + S);
    // (no __restrict__: other lanes of the workgroup write what this one reads a barrier later; global, not flat: a flat load's wait would
    //  also wait for the scalar loads of the weights)
    typedef __attribute__((address_space(1))) float gfloat;
    gfloat *y = (gfloat *)(L.y + (int64_t)c * H * W);
    const uint32_t chunk = L.chunk0 + (uint32_t)(c * K + (own ? k : 0));
    const uint8_t *p = bytes + off[chunk];
    const uint32_t nb = own ? cnt[chunk] : 0u;
    BitWin in;
    in.init(p, nb);
    uint32_t low = 0u, d = 0xFFFFFFFFu, x = in.w0;
    uint64_t bit = 32;
    in.advance(bit);
    auto at = [&](int hh, int ww) -> float { return hh >= 0 && ww >= 0 && ww < W ? y[(int64_t)hh * W + ww] : 0.f; };
    const int steps = K + 2 * H - 2;
    for (int T = 0; T < steps; ++T) {
        const int r = T - k, hh = r >> 1;
        if (own && r >= 0 && !(r & 1) && hh < H) {
            float a[5], b[5], c0 = at(hh, w0 - 2), c1 = at(hh, w0 - 1);
#pragma unroll
            for (int i = 0; i < 5; ++i) { a[i] = at(hh - 2, w0 - 2 + i); b[i] = at(hh - 1, w0 - 2 + i); }
            for (int w = w0; w < w1; ++w) {
                const float a5 = at(hh - 2, w + 3), b5 = at(hh - 1, w + 3);   // the window's next column: rows complete before this step
                float h[N::NL + 1][N::W];
#pragma unroll
                for (int i = 0; i < 5; ++i) { h[0][i] = a[i]; h[0][5 + i] = b[i]; }
                h[0][10] = c0; h[0][11] = c1;
                // the weights are read again for every latent (scalar loads that hit the scalar cache): hoisted out of the loops, a thousand
                // loop-invariant scalars would live in spilled registers
                int again = 0;
                asm volatile("" : "+s"(again));
                mlp_fwd<N>(net, P + again, h);
                const float mu_q = quant_mu(h[nl][0]), s_q = quant_scale(scale_of(h[nl][1]));
                // the scaled lower bound of symbol m; the symbol is the highest m with bound(m) <= x
                auto bound = [&](int m) -> uint32_t { return m == 0 ? 0u : scale_d(d, cdf_entry(mu_q, s_q, A, nsym, m)); };
                // a start from the closed-form inverse: entry ~ e (65536 - L) + m, twice (the second pass knows m)
                int m = A;
                const float pr = ((float)x + 0.5f) / ((float)d + 1.0f) * 65536.f;
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    const float e = fminf(fmaxf((pr - (float)m) / (float)(65536 - nsym), 1.0e-7f), 1.0f - 1.0e-7f);
                    const float t = e < 0.5f ? mu_q + s_q * __logf(2.f * e) : mu_q - s_q * __logf(2.f * (1.f - e));
                    const float g = floorf(t + (float)A + 0.5f);
                    m = g >= 0.f ? (g <= (float)(nsym - 1) ? (int)g : nsym - 1) : 0;   // (a NaN gives 0)
                }
                // bracket [lo_i, hi_i): bound(lo_i) <= x < bound(hi_i) (bound(0) = 0; index nsym stands for the span itself), then bisect
                int lo_i, hi_i;
                uint32_t blo = bound(m), bhi = 0u;
                bool have_hi = false;
                if (blo <= x) {
                    lo_i = m; hi_i = nsym;
                    for (int step = 1; lo_i + step < nsym; step <<= 1) {
                        const uint32_t t = bound(lo_i + step);
                        if (t <= x) { lo_i += step; blo = t; } else { hi_i = lo_i + step; bhi = t; have_hi = true; break; }
                    }
                } else {
                    hi_i = m; bhi = blo; have_hi = true; lo_i = 0; blo = 0u;
                    for (int step = 1; hi_i - step > 0; step <<= 1) {
                        const uint32_t t = bound(hi_i - step);
                        if (t <= x) { lo_i = hi_i - step; blo = t; break; }
                        hi_i -= step; bhi = t;
                    }
                }
                while (lo_i + 1 < hi_i) {
                    const int mid = (lo_i + hi_i) >> 1;
                    const uint32_t t = bound(mid);
                    if (t <= x) { lo_i = mid; blo = t; } else { hi_i = mid; bhi = t; have_hi = true; }
                }
                const int sym = lo_i;                              // in [0, nsym - 1] by construction
                const uint32_t d1 = (sym == nsym - 1 || !have_hi ? d : bhi - 1u) - blo;
                const float yv = (float)(sym - A);
                y[(int64_t)hh * W + w] = yv;
                uint32_t kbits;
                rc_renorm(low, d, x, blo, d1, in.peek(bit), kbits);
                bit += (uint64_t)(kbits & 63u);
                in.advance(bit);
#pragma unroll
                for (int i = 0; i < 4; ++i) { a[i] = a[i + 1]; b[i] = b[i + 1]; }
                a[4] = a5; b[4] = b5;
                c0 = c1; c1 = yv;
            }
        }
        __syncthreads();
    }
}

// the levels of one call: shapes, strips and where their chunks start
struct Call {
    Net net;
    bool spec;
    Levels lev;
    std::vector<Lv> lv;
    uint32_t nch = 0, kmax = 0, max_syms = 0;
    int64_t words = 0;
    int tiles = 0;
};

int make_call(const char *who, int n_levels, float *const *y, const int *C, const int *H, const int *W, const int *S, const int *A,
              int n_layers, const int *dims, Call &c)
{
    GP_TRY(make_net(who, n_layers, dims, c.net, c.spec));
    GP_TRY(make_levels(who, n_levels, y, C, H, W, c.lev));
    if (n_levels < 1 || !S) return fail(GPCC_ERR_ARG, "%s: no level", who);
    const int tb = c.spec ? Spec::TB : Any::TB;
    for (int v = 0; v < n_levels; ++v) {
        if (S[v] < S_MIN) return fail(GPCC_ERR_ARG, "%s: level %d: strips of %d columns (at least %d)", who, v, S[v], S_MIN);
        const int64_t K = cdiv(W[v], S[v]);
        if (K > K_MAX) return fail(GPCC_ERR_ARG, "%s: level %d: %lld strips (at most %d: widen them)", who, v, (long long)K, K_MAX);
        if (A && (A[v] < 2 || A[v] > A_MAX)) return fail(GPCC_ERR_RANGE, "%s: level %d: alphabet bound %d outside [2, %d]", who, v, A[v], A_MAX);
        Lv l = {};
        l.y = y[v]; l.C = C[v]; l.H = H[v]; l.W = W[v]; l.S = S[v]; l.K = (int)K; l.A = A ? A[v] : 0; l.n = (int)c.lev.n[v];
        l.tile0 = c.tiles; l.chunk0 = c.nch; l.word0 = (uint32_t)c.words;
        const int64_t syms = (int64_t)H[v] * std::min(S[v], W[v]);
        c.tiles += (int)cdiv(l.n, tb);
        c.words += (int64_t)C[v] * K * syms;
        if ((int64_t)c.nch + (int64_t)C[v] * K > ((int64_t)1 << 24) || c.words >= ((int64_t)1 << 31) || syms >= ((int64_t)1 << 28))
            return fail(GPCC_ERR_ARG, "%s: too many chunks or symbols in one call", who);
        c.nch += (uint32_t)(C[v] * K);
        c.kmax = std::max(c.kmax, (uint32_t)K);
        c.max_syms = std::max(c.max_syms, (uint32_t)syms);
        c.lv.push_back(l);
    }
    return GPCC_OK;
}

}  // namespace

extern "C" int gsac_arm_cdf_rows(gpcc_ctx *ctx, const float *mu, const float *scale, int64_t n, int A, uint16_t *rows_out, void *stream)
{
    if (!ctx || !mu || !scale || !rows_out) return fail(GPCC_ERR_ARG, "gsac_arm_cdf_rows: null argument");
    if (A < 1 || A > A_MAX) return fail(GPCC_ERR_RANGE, "gsac_arm_cdf_rows: alphabet bound %d outside [1, %d]", A, A_MAX);
    if (n <= 0) return GPCC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    k_arm_rows<<<(unsigned)cdiv(n * (2 * A + 2), 256), 256, 0, (hipStream_t)stream>>>(mu, scale, n, A, rows_out);
    LAUNCH_CHECK();
    return GPCC_OK;
}

extern "C" int gsac_arm_encode(gpcc_ctx *ctx, int n_levels, const float *const *y, const int *channels, const int *heights, const int *widths,
                               const int *strips, const float *params, int n_layers, const int *dims, int *alphabet_out, const uint8_t **bytes_out,
                               int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream)
{
    const char *who = "gsac_arm_encode";
    const CoderOut out = {bytes_out, nbytes_out, cnt_out, nchunks_out};
    if (!ctx || !params || !alphabet_out || out.null()) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    Call c;
    GP_TRY(make_call(who, n_levels, const_cast<float *const *>(y), channels, heights, widths, strips, nullptr, n_layers, dims, c));
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int nch = (int)c.nch;
    const uint32_t sstride = rc_scratch_stride(c.max_syms);
    GP_TRY(ctx->arena.reserve((size_t)c.words * 4 + 2 * (size_t)nch * sstride + (size_t)nch * 64 + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(dlv, Lv, n_levels); TAKE(stats, uint32_t, 2 * n_levels + 1);
    TAKE(lohi, uint32_t, c.words); TAKE(dch, RcChunk, nch); TAKE(dcnt, uint32_t, nch + 1); TAKE(doff, uint32_t, nch + 1);
    TAKE(scratch, uint8_t, (size_t)nch * sstride); TAKE(payload, uint8_t, (size_t)nch * sstride);
    // the alphabets: A = ceil(max |y|) + 2 per level
    HIP_TRY(hipMemcpyAsync(dlv, c.lv.data(), sizeof(Lv) * (size_t)n_levels, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(stats, 0, 4 * (2 * (size_t)n_levels + 1), st));
    k_arm_absmax<<<(unsigned)std::min<int64_t>(cdiv(c.lev.largest, 256), 512), 256, 0, st>>>(dlv, n_levels, stats);
    LAUNCH_CHECK();
    std::vector<uint32_t> hs(2 * (size_t)n_levels);
    HIP_TRY(hipMemcpyAsync(hs.data(), stats, 4 * hs.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int v = 0; v < n_levels; ++v) {
        float mx;
        memcpy(&mx, &hs[2 * (size_t)v], 4);
        if (hs[2 * (size_t)v + 1]) return fail(GPCC_ERR_RANGE, "%s: level %d holds a latent that is not an integer", who, v);
        if (mx > (float)(A_MAX - 2)) return fail(GPCC_ERR_RANGE, "%s: level %d: max |y| = %g, the alphabet bound would exceed %d", who, v, (double)mx, A_MAX);
        c.lv[(size_t)v].A = alphabet_out[v] = (int)ceilf(mx) + 2;
    }
    std::vector<RcChunk> chunks((size_t)nch);
    for (const Lv &l : c.lv)
        for (int ch = 0; ch < l.C; ++ch)
            for (int k = 0; k < l.K; ++k) {
                const uint32_t id = (uint32_t)(ch * l.K + k);
                chunks[(size_t)l.chunk0 + id] = RcChunk{l.word0 + id, (uint32_t)(l.C * l.K), (uint32_t)(l.H * std::min(l.S, l.W - k * l.S)), 0, 0, 0};
            }
    HIP_TRY(hipMemcpyAsync(dlv, c.lv.data(), sizeof(Lv) * (size_t)n_levels, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dch, chunks.data(), sizeof(RcChunk) * (size_t)nch, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));       // (the host vectors are pageable)
    uint32_t *flag = stats + 2 * n_levels;
    if (c.spec) k_arm_pack<Spec><<<c.tiles, Spec::TB, 0, st>>>(c.net, params, dlv, n_levels, lohi, flag);
    else k_arm_pack<Any><<<c.tiles, Any::TB, 0, st>>>(c.net, params, dlv, n_levels, lohi, flag);
    LAUNCH_CHECK();
    GP_TRY(encode_tail(ctx, st, lohi, dch, nch, scratch, sstride, dcnt, doff, payload, out));
    uint32_t bad = 0;
    HIP_TRY(hipMemcpy(&bad, flag, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(GPCC_ERR_RANGE, "%s: the ARM gives a mu or a scale that is not finite: no stream is written", who);
    return GPCC_OK;
}

extern "C" int gsac_arm_decode(gpcc_ctx *ctx, int n_levels, float *const *y_out, const int *channels, const int *heights, const int *widths,
                               const int *strips, const int *alphabets, const float *params, int n_layers, const int *dims, const uint8_t *bytes,
                               int64_t nbytes, const int32_t *cnt, int64_t nchunks, void *stream)
{
    const char *who = "gsac_arm_decode";
    if (!ctx || !params || !alphabets || !cnt || (!bytes && nbytes)) return fail(GPCC_ERR_ARG, "%s: null argument", who);
    Call c;
    GP_TRY(make_call(who, n_levels, y_out, channels, heights, widths, strips, alphabets, n_layers, dims, c));
    if (nchunks != (int64_t)c.nch) return fail(GPCC_ERR_FORMAT, "%s: %lld chunk counts, the levels have %u chunks", who, (long long)nchunks, c.nch);
    if (nbytes < 0 || nbytes >= ((int64_t)1 << 32)) return fail(GPCC_ERR_FORMAT, "%s: byte stream must be shorter than 4 GiB", who);
    const int nch = (int)c.nch;
    std::vector<uint32_t> tab(2 * (size_t)nch);   // offsets, then counts
    uint64_t run = 0;
    for (int i = 0; i < nch; ++i) {
        if (cnt[i] < 0) return fail(GPCC_ERR_FORMAT, "%s: negative chunk size", who);
        tab[(size_t)i] = (uint32_t)run;
        tab[(size_t)nch + i] = (uint32_t)cnt[i];
        run += (uint64_t)cnt[i];
        if (run > (uint64_t)nbytes) return fail(GPCC_ERR_FORMAT, "%s: chunk sizes exceed the byte stream", who);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    GP_TRY(ctx->arena.reserve((size_t)nbytes + 8 * (size_t)nch + ((size_t)4 << 20)));
    ctx->arena.reset();
    TAKE(dlv, Lv, n_levels); TAKE(db, uint8_t, nbytes + 16); TAKE(dtab, uint32_t, 2 * (size_t)nch);
    HIP_TRY(hipMemcpyAsync(dlv, c.lv.data(), sizeof(Lv) * (size_t)n_levels, hipMemcpyHostToDevice, st));
    if (nbytes) HIP_TRY(hipMemcpyAsync(db, bytes, (size_t)nbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dtab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    unsigned blocks = 0;
    for (const Lv &l : c.lv) blocks += (unsigned)l.C;
    const uint32_t *doff = dtab, *dcnt = dtab + nch;
#define ARM_DECODE(N, TB) k_arm_decode<N, TB><<<blocks, TB, 0, st>>>(c.net, params, dlv, n_levels, db, doff, dcnt)
    if (c.spec) { if (c.kmax <= 64) ARM_DECODE(Spec, 64); else if (c.kmax <= 256) ARM_DECODE(Spec, 256); else ARM_DECODE(Spec, 1024); }
    else { if (c.kmax <= 64) ARM_DECODE(Any, 64); else if (c.kmax <= 256) ARM_DECODE(Any, 256); else ARM_DECODE(Any, 1024); }
#undef ARM_DECODE
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    return GPCC_OK;
}
