// codec_shared.hpp -- what gpcc_encode / gpcc_decode (codec.hip), their batched forms (codec_batch.hip) and the training frame
// (train.hip) have in common: the Conv-ReLU-ResNet-ResNet trunk, the encoder's teacher-forced network over its two level sets, the
// decoder's per-level chain up to each head, the container's header fields and per-stream tables, the retry helpers of the entry
// points.  What differs between the callers comes in as data or as a callable.  Definitions: codec_shared.hip.
#pragma once
#include <functional>
#include <vector>

#include "fused.hpp"
#include "network.hpp"
#include "octree.hpp"
#include "primitives.hpp"

namespace gpcc {

struct Trunk { float *x, *a, *b; };

// Conv-ReLU-ResNet-ResNet (network_ue_4stage_conv.py:17-33; kit/nn.py:18-22).  Result in t.a.
static inline int run_trunk(gpcc_ctx *ctx, int level, hipStream_t st, const gpcc_model *m, int conv0, const Trunk &t, const ConvTiles &tiles, int64_t n, const PairPlan *plan = nullptr,
              float *P = nullptr)
{
    ConvBatch cb = {}; cb.C = m->C;
    auto one = [&](const float *in, int ci, const float *res, float *out) {
        cb.job[0] = ConvJob{in, m->conv[ci], res, out};
        if (plan) return plan_conv(st, *plan, cb.job[0], P, 1);
        return sparse_conv(ctx, level, st, cb, 1, tiles, n, 1);
    };
    GP_TRY(conv_chain_begin(ctx, st));
    GP_TRY(one(t.x, conv0, nullptr, t.a));
    GP_TRY(one(t.a, conv0 + 1, nullptr, t.b));
    GP_TRY(one(t.b, conv0 + 2, t.a, t.x));
    GP_TRY(one(t.x, conv0 + 3, nullptr, t.b));
    GP_TRY(one(t.b, conv0 + 4, t.x, t.a));
    GP_TRY(conv_chain_end(ctx, st));
    return GPCC_OK;
}

static inline void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static inline uint32_t get32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// encode keeps the whole tree resident: ~3 nodes per point, per node its cell map (27 x 4 B) + tile lists (~150 B) + ~12
// feature rows of 128 B + level arrays; grown and retried when a cloud needs more
static inline size_t arena_estimate(int64_t n, int K) { return (size_t)n * 3 * (size_t)(4 * 125 + 300 + 12 * 128 + 96) + (size_t)n * 64 + (size_t)K * 4096 + ((size_t)64 << 20); }
// developer / test knob GAUSPCC_ARENA_SCALE: scales the first workspace estimate of every call, so that the grow-and-retry path (a level
// of the tree, the tile pool, the rank pass on the second stream or a feature buffer running out of arena) can be driven on purpose
size_t arena_scaled(size_t want);
// one line on stderr (GAUSPCC_FUSED_QUIET silences it): a persistent small-level launch timed out, the decode runs again launch per layer
void fused_timeout_notice(const gpcc_ctx *ctx);
// error returns leave nothing in flight on the context's other streams (x: the decoder's transfer stream, null in an encode)
struct SideGuard { hipStream_t s, x; ~SideGuard() { (void)hipStreamSynchronize(s); if (x) (void)hipStreamSynchronize(x); } };

// ---------------------------------------------------------------------------------------------------------------- encoder
// Tile lists of every level of T in one pool, built top-down from the cell maps (tiles.hip; one stream sync for the pool size).  A
// level's list is the same in the prior and in the target set -- tile entries are row indices inside the level -- so the two sets
// are two views of the pool: levels 0..L-2 and 1..L-1.  root / cell_root: the level above the base level and its cell map (a forest's
// root level: forest.hpp), null for one scene.  pairs_dev: nullable (tiles_build).  Needs T.L > 1.
int tile_sets(gpcc_ctx *ctx, hipStream_t st, const Tree &T, const Level *root, const int32_t *cell_root, int k, unsigned long long *pairs_dev, TilePool *pool, ConvTiles *setP,
              ConvTiles *setC);

// The teacher-forced network of an encode (T.L > 1): every level is independent of the others, so all parent levels are concatenated
// into one "prior set" P (levels 0..L-2) and all coded levels into one "target set" C (levels 1..L-1), and each of the 18 network
// layers is ONE launch over a set.  The heads leave one packed (c_low, c_high) word per symbol in lohi, at the slots the caller's
// position kernel gives every row of C.
struct EncodeNet {
    const Tree *T;
    const Level *root; const int32_t *cell_root;   // tile_sets
    unsigned long long *pairs_dev;                 // [MAXLV] pair counters
    uint32_t *lohi;
    double *bits;                                  // nullable: 16 accumulators of the ideal code length (HeadArgs::bits)
    // The second stream's work, queued behind the first trunk's launches (the device then has milliseconds of convolutions in hand, so
    // the host time of the ~190 small launches is free): the raster ranks of every level -- their temporaries come from the top of the
    // arena (Arena::flip), which nothing else in an encode uses -- and then the coder slot of stage 0 (pos) and the stage stride (slots)
    // of every row of C.  Their first reader is the head of stage 0, eighteen convolutions away.
    std::function<int(hipStream_t)> ranks;
    std::function<int(hipStream_t, uint32_t *pos, uint32_t *slots)> set_pos;
    HostTrace *ht; const char *trace;              // label prefix of the host trace ("enc" / "benc")
};
int encode_network(gpcc_ctx *ctx, const gpcc_model *m, hipStream_t st, hipStream_t sd, const EncodeNet &a);

// The lanes of every stream of a call, in the order the streams are appended: one descriptor per lane.
struct LaneList {
    std::vector<RcChunk> chunks;
    uint32_t max_syms = 1;
    size_t table_bound = 0;   // most bytes the chunk tables can take
};
// appends the lanes of stream si: nc symbols cut by pl, its packed words from slot first_slot on
int lanes_append(LaneList *ll, int si, int64_t first_slot, int64_t nc, const RcPlan &pl);

// byte count of chunk c of the stream whose lanes are [c0, c1) of the lane byte counts (a chunk: two lanes; the last may have one)
static inline uint32_t chunk_bytes(const uint32_t *hcnt, int c0, int c1, uint32_t c) { const int l = c0 + 2 * (int)c; return hcnt[l] + (l + 1 < c1 ? hcnt[l + 1] : 0u); }
// what a stream takes in the container, from its lanes' byte counts.  fits: no chunk is larger than the staged decoder's window
// (rangecoder.hpp: rc_window_fits) -- the caller decides what an oversize chunk means.  chunked = false (the reference layout): no table.
struct StreamSize { size_t pay = 0, tab = 0; uint32_t max_chunk = 0; bool fits = true; };
StreamSize stream_size(const uint32_t *hcnt, int c0, int c1, int si, bool chunked);
// the stream's length field and chunk table at o; returns their bytes (the payload behind them is in place already)
size_t stream_head_put(uint8_t *o, const uint32_t *hcnt, int c0, int c1, const StreamSize &z, bool chunked);
// header of a chunked container: magic, version, chunk size, posq, levels, level sizes, points; returns its bytes
size_t chunked_header_put(uint8_t *o, int version, int chunk_log2, uint16_t posq, int L, const int64_t *level_nodes, int64_t npts);
// base block (count, raster-order coordinates minus `origin`, occupancies) and the stream count; returns their bytes
size_t base_block_put(uint8_t *o, int64_t bn, const int32_t *xyz, const int64_t origin[3], const uint8_t *occ, int nstreams);
// pairs of the two sets from the per-level counters (the conv launches are tagged 0 = prior set, 1 = target set)
void sum_set_pairs(const unsigned long long *per_level, int L, unsigned long long set_pairs[2]);

// ---------------------------------------------------------------------------------------------------------------- decoder
struct BaseNode { uint64_t mk, rk; uint8_t occ; };
// a scene's bn base nodes (container bytes), moved by t into a frame whose coordinates are below lim, appended in Morton order.
// who: prefix of the error texts ("" or "scene 3: ").
int base_nodes_append(const uint8_t *bxyz, const uint8_t *bocc, int64_t bn, const int64_t t[3], int64_t lim, const char *who, std::vector<BaseNode> *out);

// a level's arrays, carved back to back from the arena's bottom: level_expand_rank zeroes them with ONE memset over the recorded span
int alloc_level(gpcc_ctx *ctx, Level *lv, int64_t n, int lvl);

// prior trunk of level g (np rows, occupancy occ) on st, buffers from the arena's top: one persistent launch when the level has a pair
// plan and fmode == 1 (*any_fused is then set), else embedding + five launches (on the plan, when there is one).  *pA: the result.
int dec_parent_trunk(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, const uint8_t *occ, int64_t np, const ConvTiles &tilesP, const PairPlan &planP, int64_t planP_np,
                     int fmode, float **pA, bool *any_fused);
// the child level's convolution lists from its parent's cell map (side stream): a pair plan (small levels) or a tile list
int dec_child_lists(gpcc_ctx *ctx, hipStream_t sd, const gpcc_model *m, const Level *cur, const int32_t *cellP, const Level *chi, int32_t *cellC, bool child_plan,
                    unsigned long long *pairs_dev, PairPlan *planC, ConvTiles *tilesC);

// How the nodes of a coded level map to coder rows.  One scene: a node's symbol slot is its raster rank and its CDF row follows from
// the rank, llog and nlanes (rc_interleaved).  A batch's merged level brings both per node (forest.hpp: forest_cdf_pos).
struct LevelCoder {
    const uint32_t *spos, *cpos;     // symbol slot / CDF row of every node; null: from the raster rank
    uint32_t nlanes; int llog;       // lanes per stream (all scenes), log2 symbols per lane
    const RcChunk *chunks;           // [4][nlanes] lane descriptors
    uint32_t win_bytes[4];           // longest byte window of a lane, per stage
    bool dual; int coder;            // RcPlan::dual; RC_CODER_*
};
// work buffers of a coded level's chain, from the arena's top
struct ChildBufs { float *cX, *cA, *cB, *cU, *P; uint16_t *cdf; size_t cdf_bytes; uint8_t *sym[4]; };
// pcap: rows of the plan's product buffer (0: no plan); lane_syms: most symbols of a lane; sym_bytes: of each symbol array
int child_bufs_take(gpcc_ctx *ctx, const gpcc_model *m, int64_t nc, int64_t pcap, uint32_t nlanes, int64_t lane_syms, int64_t sym_bytes, ChildBufs *b);
// the level's whole chain in one persistent launch (fused.hip)
int dec_child_fused(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, const PairPlan &planC, const float *pA, int64_t np, const Level &chi, const uint8_t *dbytes,
                    const LevelCoder &lc, const ChildBufs &b);
// launch per layer: child features and target trunk (-> b.cA) ...
int dec_child_trunk(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, const float *pA, const Level &chi, const ConvTiles &tilesC, const PairPlan *planC, const ChildBufs &b);
// ... then stage s up to and including its head (-> the stage's CDF rows in b.cdf); the coder step is the caller's
int dec_child_stage(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, int s, const Level &chi, const ConvTiles &tilesC, const PairPlan *planC, const LevelCoder &lc,
                    const ChildBufs &b);
static inline int stage_row_bytes(int s) { return STAGE_M[s] == 2 ? 2 : STAGE_M[s] == 4 ? 8 : 32; }   // compact CDF row

}  // namespace gpcc
