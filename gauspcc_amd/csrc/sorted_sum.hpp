// sorted_sum.hpp -- the sum and combine passes of a backward that scatters without float atomics (the grid encoder's embedding gradient,
// gridencoder.hip; the tri-plane's plane gradient, triplane.hip).  The caller has written one (row key, slot) entry per contribution and
// sorted the entries stably by key (primitives.hpp: radix_sort_u64), so every row's contributions are one run in ascending slot order:
//   sum        one worker per chunk of CHUNK sorted entries sums each run it holds in order.  A run wholly inside the chunk goes straight
//              to its row; a chunk's first run continued from the previous chunk leaves a head partial, a run that starts in it and
//              continues leaves a tail partial and makes the chunk that row's owner.
//   combine    each owner adds the following chunks' head partials to its tail partial in chunk order, then the total to the row.
// Keys >= n_rows are the sentinel of unused contributions (they sort last and are skipped).  Every row is written by exactly one worker and
// summed in an order fixed by the sorted keys alone: bitwise reproducible.  A worker is whatever owns one accumulator set: a thread with F
// channels in registers (grid encoder) or one lane per channel of a wave that walks the chunk together (tri-plane).
#pragma once
#include <stdint.h>

namespace gpcc {

// Acc: zero(), add(i) (sorted entry i into the accumulators), to_head(t), to_tail(t) (the accumulators as chunk t's partial), to_row(row).
template <int CHUNK, class Acc>
__device__ __forceinline__ void sorted_chunk_sum(const uint64_t *__restrict__ keys, int64_t t, int64_t E, uint32_t n_rows, Acc &a, uint8_t *__restrict__ own)
{
    const int64_t i0 = t * CHUNK;
    const int64_t i1 = min(i0 + (int64_t)CHUNK, E);
    uint32_t row = (uint32_t)keys[i0];
    bool first = true, starts = i0 == 0 || (uint32_t)keys[i0 - 1] != row;
    uint8_t owner = 0;
    a.zero();
    auto flush = [&](bool cont) {
        if (row >= n_rows) return;
        if (first && !starts) a.to_head(t);
        else if (cont) { a.to_tail(t); owner = 1; }
        else a.to_row(row);
    };
    for (int64_t i = i0; i < i1; ++i) {
        const uint32_t k = (uint32_t)keys[i];
        if (k != row) {
            flush(false);
            row = k; first = false; starts = true;
            a.zero();
        }
        if (row < n_rows) a.add(i);
    }
    flush(i1 < E && (uint32_t)keys[i1] == row);
    own[t] = owner;
}

// The owners' walk.  Chunk j's partials are head[j * stride + ch] / tail[j * stride + ch], ch < F; put(row, s) receives the F totals.
// Partials are read WALK chunks at a time, so that a long run waits on memory once per WALK chunks.
template <int CHUNK, int F, int WALK, class Put>
__device__ __forceinline__ void sorted_combine(const uint64_t *__restrict__ keys, int64_t E, int64_t nchunks, int64_t t, const float *__restrict__ head,
                                               const float *__restrict__ tail, int64_t stride, const uint8_t *__restrict__ own, Put put)
{
    if (t >= nchunks || !own[t]) return;
    const uint32_t row = (uint32_t)keys[min((t + 1) * CHUNK, E) - 1];
    float s[F];
    for (int ch = 0; ch < F; ++ch) s[ch] = tail[t * stride + ch];
    for (int64_t j0 = t + 1; j0 < nchunks; j0 += WALK) {
        float h[WALK][F];
        bool more[WALK];
#pragma unroll
        for (int u = 0; u < WALK; ++u) {
            const int64_t j = j0 + u, nxt = (j + 1) * CHUNK;
            for (int ch = 0; ch < F; ++ch) h[u][ch] = j < nchunks ? head[j * stride + ch] : 0.0f;
            more[u] = j < nchunks && nxt < E && (uint32_t)keys[nxt] == row;
        }
        bool done = false;
#pragma unroll
        for (int u = 0; u < WALK; ++u) {
            if (done) break;
            for (int ch = 0; ch < F; ++ch) s[ch] += h[u][ch];
            done = !more[u];
        }
        if (done) break;
    }
    put(row, s);
}

}  // namespace gpcc
