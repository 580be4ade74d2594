// coder_tail.hpp -- the tail every chunked encoder shares (attributes.hip has the definition): from the packed (low, high) words to
// context-owned host bytes and per-chunk byte counts.
#pragma once
#include "rangecoder.hpp"

// where an encoder leaves its result: payload and chunk byte counts in the context's pinned buffers, valid until the context's next call
struct CoderOut {
    const uint8_t **bytes; int64_t *nbytes; const int32_t **cnt; int64_t *nchunks;
    bool null() const { return !bytes || !nbytes || !cnt || !nchunks; }
};

int encode_tail(gpcc_ctx *ctx, hipStream_t st, const uint32_t *lohi, const gpcc::RcChunk *dch, int nch, uint8_t *scratch, uint32_t sstride, uint32_t *dcnt,
                uint32_t *doff, uint8_t *payload, CoderOut out, const int32_t *mm = nullptr, int nslices = 0, float *min_out = nullptr,
                float *max_out = nullptr);
