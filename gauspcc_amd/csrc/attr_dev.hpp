// attr_dev.hpp -- device code of the attribute coders that more than one translation unit uses (attributes.hip, cat_chain.hip): the entry function of
// the torchac-style Normal rows, the wave's bit reader, the scalar helpers of the decoding wave and the check of a stream's symbol range.
#pragma once
#include "common.hpp"

namespace {

// lower[idx][j] of TC-GS / CAT-3DGS's encoder_gaussian (TC-GS/utils/encodings.py:92-99):
//     Normal(mean, scale).cdf((samples - 0.5) * Q),   samples = arange(min, max + 2).to(float)
// torch.distributions.Normal.cdf is 0.5 * (1 + erf((value - loc) * scale.reciprocal() / sqrt(2))).  ONE definition, as gaussian_cdf_entry (attributes.hip): the
// table kernel, the encoder's pre-pass and the decoder's windows all call it.  The float32 steps, in the order torch's device kernels take them (every one
// rounded on its own: the intrinsics below are never contracted into a fused multiply-add):
//   1  sample = (float(min + j) - 0.5f) * Q         the caller's `samples - 0.5` (exact) and its product with Q
//   2  d      = sample - mean                       the subtraction
//   3  r      = 1.0f / scale                        Tensor.reciprocal: a correctly rounded division
//   4  t      = d * r                               the product
//   5  u      = t * (1.0f / float(sqrt(2.0)))       ATen divides a device tensor by a host scalar as a product with the scalar's reciprocal
//                                                   (BinaryDivTrueKernel.cu: `inv_b = accscalar_t(1.0) / b`, accscalar_t = float): 0x3F3504F3
//   6  e      = erff(u)                             the device library's erff, the function torch's erf kernel calls
//   7  a      = 1.0f + e                            the add
//   8  entry  = 0.5f * a                            the halving (exact)
// No clamp on scale: TC-GS clamps to 1e-9 before the call, as its callers here do.
__device__ __forceinline__ float normal_cdf_entry(float mean, float scale, float q, int min_value, int j)
{
    const float inv_sqrt2 = __fdiv_rn(1.0f, (float)1.4142135623730951);
    const float sample = __fmul_rn(__fsub_rn((float)(min_value + j), 0.5f), q);
    const float d = __fsub_rn(sample, mean);
    const float r = __fdiv_rn(1.0f, scale);
    const float t = __fmul_rn(d, r);
    const float u = __fmul_rn(t, inv_sqrt2);
    return __fmul_rn(0.5f, __fadd_rn(1.0f, erff(u)));
}

// the parameters of an element under normal_cdf_entry: the table (one entry per element) and one element's row
struct NormalTable { const float *mean, *scale, *q; int min_value; };
struct NormalRow { float mean, scale, q; int min_value; };

__device__ __forceinline__ uint32_t cdf_int(const NormalRow &row, int m, float scale)
{
    return (uint32_t)((int)__builtin_rintf(normal_cdf_entry(row.mean, row.scale, row.q, row.min_value, m) * scale) + m);
}

// Bit reader of a wave: the chunk's bytes come in 64 words at a time -- lane j loads big-endian word j of the current block, one coalesced load per
// 2 048 bits -- and the coder draws the next word with v_readlane.  (Until round 5 every refill was a load of its own whose latency, ~1 us from HBM
// and never less than an L1 round trip, sat in the symbol chain every 32 bits.)  Bytes past the chunk's end read as zero and are never loaded.
// The state is wave-uniform and kept in scalar registers (readfirstlane): the range arithmetic of the caller runs on the scalar unit.
struct WaveBits {
    const uint8_t *p;     // first byte of the current block of 64 words
    int32_t rem;          // bytes of the chunk from p on
    uint32_t words;       // per lane: word `lane` of the block
    uint32_t widx;        // next word of the block to hand out (64: block exhausted)
    uint32_t nw;
    uint64_t buf;
    uint32_t n;
    __device__ __forceinline__ void load_block()
    {
        const int lane = threadIdx.x & 63;
        const int32_t left = rem - 4 * lane;          // bytes of the chunk at this lane's word
        uint32_t w = 0u;
        if (left >= 4) {
            __builtin_memcpy(&w, p + 4 * lane, 4);
            w = __builtin_bswap32(w);
        } else if (left > 0) {                        // the chunk's last, partial word: byte by byte (nothing behind the chunk is touched)
            for (int b = 0; b < left; ++b) w |= (uint32_t)p[4 * lane + b] << (24 - 8 * b);
        }
        words = w;
        widx = 0u;
    }
    __device__ __forceinline__ uint32_t next_word()
    {
        if (widx == 64u) { p += 256; rem -= 256; load_block(); }
        widx = (uint32_t)__builtin_amdgcn_readfirstlane((int)widx);
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)words, (int)widx);
        widx += 1u;
        return w;
    }
    __device__ __forceinline__ void init(const uint8_t *base, uint32_t nbytes) { p = base; rem = (int32_t)nbytes; buf = 0; n = 0; load_block(); nw = next_word(); }
    __device__ __forceinline__ uint32_t take(uint32_t k)
    {
        if (n <= 32) {
            buf |= (uint64_t)nw << (32 - n);
            n += 32;
            nw = next_word();
        }
        const uint32_t r = (uint32_t)((buf >> 1) >> (63 - k));
        buf <<= k;
        n -= k;
        buf = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(buf >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)buf);
        n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
        return r;
    }
};

__device__ __forceinline__ int clz32(uint32_t x) { return x ? __clz((int)x) : 32; }
// value of lane `l` (wave-uniform index) as a scalar: v_readlane_b32 -- the result lives in an SGPR, so what is computed from it (the coder's range
// update) runs on the scalar unit beside the other waves' VALU work; __shfl with a uniform index is a ds_bpermute whose result is a VGPR
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int64_t uniform64(int64_t v) { return (int64_t)(((uint64_t)uniform((uint32_t)((uint64_t)v >> 32)) << 32) | uniform((uint32_t)v)); }
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(l)); }

}  // namespace

namespace gpcc {
// The symbol range [min, max] of a stream as its `.b` file stores it, two floats -> min and the row length max - min + 2.  The floats come off
// disk: NaN, infinities, values that do not fit an int and alphabets that int16 symbols cannot index are format errors.
static int symbol_range(float min_value, float max_value, int *mn, int *lp)
{
    if (!(min_value >= -1.0e9f && min_value <= 1.0e9f) || !(max_value >= -1.0e9f && max_value <= 1.0e9f))
        return fail(GPCC_ERR_FORMAT, "bad symbol range [%g, %g]", (double)min_value, (double)max_value);
    const int64_t lp64 = (int64_t)(int)max_value - (int)min_value + 2;
    if (lp64 < 2 || lp64 > 32767) return fail(GPCC_ERR_FORMAT, "bad symbol range [%d, %d]", (int)min_value, (int)max_value);
    *mn = (int)min_value; *lp = (int)lp64;
    return GPCC_OK;
}
}  // namespace gpcc
