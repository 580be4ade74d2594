// codec_shared.hip -- the definitions behind codec_shared.hpp: one copy of the network chain for the solo codec (codec.hip), the
// batched one (codec_batch.hip) and the training frame (train.hip).  Nothing here knows which of them is calling.
#include <algorithm>

#include "codec_shared.hpp"

namespace gpcc {

size_t arena_scaled(size_t want)
{
    static const double scale = [] { const char *e = getenv("GAUSPCC_ARENA_SCALE"); const double v = e ? atof(e) : 1.0; return v > 0.0 ? v : 1.0; }();
    return scale == 1.0 ? want : std::max<size_t>((size_t)((double)want * scale), (size_t)1 << 20);
}

void fused_timeout_notice(const gpcc_ctx *ctx)
{
    static const bool loud = getenv("GAUSPCC_FUSED_QUIET") == nullptr;
    if (loud) fprintf(stderr, "[gauspcc] a persistent small-level launch timed out on device %d; the launch-per-layer path serves this context's next %d decodes\n", ctx->device, ctx->fused_rearm_after);
}

// ---------------------------------------------------------------------------------------------------------------- encoder
int tile_sets(gpcc_ctx *ctx, hipStream_t st, const Tree &T, const Level *root, const int32_t *cell_root, int k, unsigned long long *pairs_dev, TilePool *pool, ConvTiles *setP,
              ConvTiles *setC)
{
    const int L = T.L, NPc = cell_map_entries(k);
    TileLevel tl[MAXLV];
    int64_t pb[MAXLV] = {0}, cb[MAXLV] = {0};   // first row of level d in P, of level d + 1 in C
    const int32_t *cell_prev = cell_root;
    for (int d = 0; d < L; ++d) {
        int32_t *own = nullptr;
        if (d + 1 < L) { TAKE(cm, int32_t, (int64_t)NPc * T.lv[d].n); own = cm; }   // the last level has no level below it
        tl[d] = TileLevel{&T.lv[d], d ? &T.lv[d - 1] : root, cell_prev, own};
        cell_prev = own;
        if (d + 1 < L) { pb[d + 1] = pb[d] + T.lv[d].n; cb[d + 1] = cb[d] + T.lv[d + 1].n; }
    }
    const int64_t nC = cb[L - 1];
    const int R = conv_pick_rows(nC, k), H = conv_pick_height(nC, R);
    GP_TRY(tiles_build(ctx, st, tl, L, k, R, H, pool, pairs_dev));
    GP_TRY(tiles_view(ctx, st, *pool, 0, L - 1, pb, setP));
    GP_TRY(tiles_view(ctx, st, *pool, 1, L, cb, setC));
    return GPCC_OK;
}

namespace {

// Per-row metadata of the two concatenated sets, every level in one launch.  Level d lives in the prior set P at rows
// pb[d].. (d <= L-2) and in the target set C at rows cbase[d].. (d >= 1).
struct SetLevels {
    int L;
    uint32_t n[MAXLV], pb[MAXLV], cbase[MAXLV];
    const uint8_t *occ[MAXLV];
    const uint64_t *rkey[MAXLV];
    const uint32_t *parent[MAXLV];
};

// occupancy of both sets, raster keys and global parent rows of C: what the network needs (no ranks)
__global__ __launch_bounds__(256) void k_set_rows(SetLevels S, int64_t nP, int64_t nC, uint8_t *__restrict__ occP, uint8_t *__restrict__ occC, uint64_t *__restrict__ rkeyC,
                                                  uint32_t *__restrict__ parentC)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nP) {
        int d = 0;
        for (int q = 1; q + 1 < S.L; ++q) d = i >= (int64_t)S.pb[q] ? q : d;
        occP[i] = S.occ[d][i - S.pb[d]];
    }
    if (i < nC) {
        int d = 1;
        for (int q = 2; q < S.L; ++q) d = i >= (int64_t)S.cbase[q] ? q : d;
        const int64_t j = i - S.cbase[d];
        occC[i] = S.occ[d][j];
        rkeyC[i] = S.rkey[d][j];
        parentC[i] = S.pb[d - 1] + S.parent[d][j];
    }
}

}  // namespace

int encode_network(gpcc_ctx *ctx, const gpcc_model *m, hipStream_t st, hipStream_t sd, const EncodeNet &a)
{
    const Tree &T = *a.T;
    const int L = T.L;
    auto mark = [&](const char *what) {
        if (!a.ht->on) return;
        char label[48];
        snprintf(label, sizeof label, "%s %s", a.trace, what);
        a.ht->mark(label);
    };
    SetLevels S = {};
    S.L = L;
    int64_t nP = 0, nC = 0;
    for (int d = 0; d < L; ++d) {
        const Level *lv = &T.lv[d];
        S.n[d] = (uint32_t)lv->n; S.pb[d] = (uint32_t)nP; S.cbase[d] = (uint32_t)nC;
        S.occ[d] = lv->occ; S.rkey[d] = lv->rkey; S.parent[d] = lv->parent;
        if (d + 1 < L) nP += lv->n;
        if (d) nC += lv->n;
    }
    TAKE(occP, uint8_t, nP); TAKE(occC, uint8_t, nC); TAKE(rkeyC, uint64_t, nC);
    TAKE(parentC, uint32_t, nC); TAKE(posC, uint32_t, nC); TAKE(slotsC, uint32_t, nC);
    {
        StageTimer tm(ctx, st, ST_ELEM, (double)nP * 2 + (double)nC * (2 + 16 + 8));
        k_set_rows<<<(unsigned)cdiv(std::max(nP, nC), 256), 256, 0, st>>>(S, nP, nC, occP, occC, rkeyC, parentC);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipEventRecord(ctx->ev_main, st));   // the tree is complete on st
    mark("meta queued");
    ConvTiles tilesP, tilesC;
    {
        TilePool pool;
        StageTimer tm(ctx, st, ST_TILES, 0.0);
        GP_TRY(tile_sets(ctx, st, T, a.root, a.cell_root, m->k, a.pairs_dev, &pool, &tilesP, &tilesC));
        tm.add_bytes(pool.alg_bytes);
    }
    mark("tiles built");
    TAKE(pF, float, nP * m->C); TAKE(pA, float, nP * m->C); TAKE(pB, float, nP * m->C);
    { StageTimer tm(ctx, st, ST_ELEM, (double)nP * 129); GP_TRY(embed_occ(st, m->prior_emb, occP, nP, pF, m->C)); }
    GP_TRY(run_trunk(ctx, 0, st, m, 0, Trunk{pF, pA, pB}, tilesP, nP));           // -> pA
    // the second stream (EncodeNet::ranks / set_pos)
    {
        HIP_TRY(hipStreamWaitEvent(sd, ctx->ev_main, 0));
        ctx->arena.flip = true;
        int rc = GPCC_OK;
        {
            StageTimer tm(ctx, sd, ST_OCTREE, 0.0);
            rc = a.ranks(sd);
        }
        ctx->arena.flip = false;
        GP_TRY(rc);
        {
            StageTimer tm(ctx, sd, ST_ELEM, (double)nC * (4 + 8));
            GP_TRY(a.set_pos(sd, posC, slotsC));
        }
        HIP_TRY(hipEventRecord(ctx->ev_side, sd));
    }
    TAKE(cX, float, nC * m->C); TAKE(cA, float, nC * m->C); TAKE(cB, float, nC * m->C);
    { StageTimer tm(ctx, st, ST_ELEM, (double)nC * (128 + 12 + 128)); GP_TRY(child_features(st, pA, parentC, rkeyC, m->temb, nC, cX, m->C)); }
    GP_TRY(run_trunk(ctx, 1, st, m, 5, Trunk{cX, cA, cB}, tilesC, nC));           // -> cA  (X of pcc_utils.py:109)
    // stages: cX, cB are free now; inputs u[s], mid v[s], outputs y[s]
    TAKE(u1, float, nC * m->C); TAKE(u2, float, nC * m->C); TAKE(u3, float, nC * m->C);
    TAKE(v1, float, nC * m->C); TAKE(v2, float, nC * m->C);
    float *u[4] = {cA, u1, u2, u3};
    float *v[4] = {cX, cB, v1, v2};
    {
        const float *const embs[3] = {m->semb[0], m->semb[1], m->semb[2]};
        float *const outs[3] = {u1, u2, u3};
        StageTimer tm(ctx, st, ST_ELEM, (double)nC * (128 + 1 + 3 * 128));
        GP_TRY(stage_inputs_gt(st, cA, embs, occC, nC, outs, m->C));
    }
    ConvBatch cb = {}; cb.C = m->C;
    for (int s = 0; s < 4; ++s) cb.job[s] = ConvJob{u[s], m->conv[10 + 2 * s], nullptr, v[s]};
    GP_TRY(sparse_conv(ctx, 1, st, cb, 4, tilesC, nC, 1));
    TAKE(y0, float, nC * m->C);
    float *y[4] = {y0, u1, u2, u3};
    for (int s = 0; s < 4; ++s) cb.job[s] = ConvJob{v[s], m->conv[10 + 2 * s + 1], nullptr, y[s]};
    GP_TRY(sparse_conv(ctx, 1, st, cb, 4, tilesC, nC, 0));
    GP_TRY(dbg_mark(ctx, st, 1, pA, (size_t)nP * 128)); GP_TRY(dbg_mark(ctx, st, 2, cA, (size_t)nC * 128));
    for (int s = 0; s < 4; ++s) GP_TRY(dbg_mark(ctx, st, 3 + s, y[s], (size_t)nC * 128));
    HIP_TRY(hipStreamWaitEvent(st, ctx->ev_side, 0));   // ranks -> posC / slotsC
    GP_TRY(dbg_mark(ctx, st, 7, posC, (size_t)nC * 4)); GP_TRY(dbg_mark(ctx, st, 8, slotsC, (size_t)nC * 4));
    ctx->arena.release_top_low();                       // what is enqueued on st from here on runs behind the rank pass: its temporaries are free
    StageTimer tm_heads(ctx, st, ST_HEADS, (double)nC * 4 * (128 + 1 + 8 + 4));
    for (int s = 0; s < 4; ++s) {
        HeadArgs ha = {}; ha.C = m->C;
        ha.x = y[s]; ha.n = nC; ha.stage_m = STAGE_M[s];
        ha.w1 = m->hw1[s]; ha.b1 = m->hb1[s]; ha.w2 = m->hw2[s]; ha.b2 = m->hb2[s]; ha.frag = m->hfrag[s];
        ha.occ = occC; ha.stage = s; ha.lohi = a.lohi; ha.mode = 0; ha.pos = posC; ha.slots = slotsC;
        ha.bits = a.bits;
        GP_TRY(head_cdf(st, ha));
    }
    return GPCC_OK;
}

int lanes_append(LaneList *ll, int si, int64_t first_slot, int64_t nc, const RcPlan &pl)
{
    ll->table_bound += 6 * (size_t)pl.nchunks + 8;   // escape code: 48 bits a chunk; first count + k
    // k_rc_compact tells a chunk's backwards lane by the parity of RcChunk::first; k_rc_decode_lds stores 16 symbols at a time
    if (pl.dual && ((first_slot & 1) || pl.llog < 4)) return fail(GPCC_ERR_HIP, "internal: stream %d starts on an odd slot or has lanes below 16 symbols", si);
    for (uint32_t c = 0; c < pl.nlanes; ++c) {
        const int64_t cn = pl.lane_syms(nc, c);
        ll->chunks.push_back(RcChunk{(uint32_t)(first_slot + c), pl.nlanes, (uint32_t)cn, 0, 0, 0});
        ll->max_syms = std::max<uint32_t>(ll->max_syms, (uint32_t)cn);
    }
    return GPCC_OK;
}

StreamSize stream_size(const uint32_t *hcnt, int c0, int c1, int si, bool chunked)
{
    StreamSize z;
    for (int c = c0; c < c1; ++c) z.pay += hcnt[c];
    if (!chunked) return z;
    const uint32_t nch = (uint32_t)((c1 - c0 + 1) / 2);
    for (uint32_t c = 0; c < nch; ++c) z.max_chunk = std::max(z.max_chunk, chunk_bytes(hcnt, c0, c1, c));
    z.fits = rc_window_fits(STAGE_M[si & 3] + 1, z.max_chunk);
    z.tab = rc_table_size([&](uint32_t c) { return chunk_bytes(hcnt, c0, c1, c); }, nch);
    return z;
}

size_t stream_head_put(uint8_t *o, const uint32_t *hcnt, int c0, int c1, const StreamSize &z, bool chunked)
{
    put32(o, (uint32_t)(z.tab + z.pay));
    return 4 + (chunked ? rc_table_put(o + 4, [&](uint32_t c) { return chunk_bytes(hcnt, c0, c1, c); }, (uint32_t)((c1 - c0 + 1) / 2)) : 0);
}

size_t chunked_header_put(uint8_t *o, int version, int chunk_log2, uint16_t posq, int L, const int64_t *level_nodes, int64_t npts)
{
    o[0] = 0xFF; o[1] = 0xFF; o[2] = (uint8_t)version; o[3] = (uint8_t)chunk_log2; o[4] = (uint8_t)posq; o[5] = (uint8_t)(posq >> 8); o[6] = (uint8_t)L; o[7] = 0;
    size_t p = 8;
    for (int d = 0; d < L; ++d) { put32(o + p, (uint32_t)level_nodes[d]); p += 4; }
    put32(o + p, (uint32_t)npts); p += 4;
    return p;
}

size_t base_block_put(uint8_t *o, int64_t bn, const int32_t *xyz, const int64_t origin[3], const uint8_t *occ, int nstreams)
{
    size_t p = 0;
    put32(o + p, (uint32_t)bn); p += 4;
    for (int64_t i = 0; i < bn; ++i)
        for (int a = 0; a < 3; ++a) { put32(o + p, (uint32_t)((int64_t)xyz[3 * i + a] - origin[a])); p += 4; }
    memcpy(o + p, occ, (size_t)bn); p += (size_t)bn;
    o[p] = (uint8_t)nstreams; o[p + 1] = (uint8_t)(nstreams >> 8); p += 2;
    return p;
}

void sum_set_pairs(const unsigned long long *per_level, int L, unsigned long long set_pairs[2])
{
    set_pairs[0] = set_pairs[1] = 0;
    for (int d = 0; d < L; ++d) { if (d + 1 < L) set_pairs[0] += per_level[d]; if (d) set_pairs[1] += per_level[d]; }
}

// ---------------------------------------------------------------------------------------------------------------- decoder
int base_nodes_append(const uint8_t *bxyz, const uint8_t *bocc, int64_t bn, const int64_t t[3], int64_t lim, const char *who, std::vector<BaseNode> *out)
{
    const size_t b0 = out->size();
    for (int64_t i = 0; i < bn; ++i) {
        uint32_t b[3];
        for (int a = 0; a < 3; ++a) {
            const int64_t c = (int32_t)get32(bxyz + 12 * i + 4 * a) + t[a];
            if (c < 0 || c >= lim) return fail(GPCC_ERR_FORMAT, "%sbase coordinate out of range", who);
            b[a] = (uint32_t)c;
        }
        if (!bocc[i]) return fail(GPCC_ERR_FORMAT, "%sempty base occupancy", who);
        out->push_back(BaseNode{morton3(b[0], b[1], b[2]), rkey3(b[0], b[1], b[2]), bocc[i]});
    }
    std::sort(out->begin() + (ptrdiff_t)b0, out->end(), [](const BaseNode &a, const BaseNode &b) { return a.mk < b.mk; });
    for (size_t i = b0 + 1; i < out->size(); ++i) if ((*out)[i].mk == (*out)[i - 1].mk) return fail(GPCC_ERR_FORMAT, "%sduplicate base node", who);
    return GPCC_OK;
}

int alloc_level(gpcc_ctx *ctx, Level *lv, int64_t n, int lvl)
{
    lv->n = n; lv->lvl = lvl;
    TAKE(rkey, uint64_t, n); TAKE(occ, uint8_t, n); TAKE(cstart, uint32_t, n + 1); TAKE(parent, uint32_t, n); TAKE(m2r, uint32_t, n); TAKE(r2m, uint32_t, n);
    lv->rkey = rkey; lv->occ = occ; lv->cstart = cstart; lv->parent = parent; lv->m2r = m2r; lv->r2m = r2m;
    lv->span0 = reinterpret_cast<char *>(rkey); lv->span_bytes = (size_t)(reinterpret_cast<char *>(r2m + n) - reinterpret_cast<char *>(rkey));
    return GPCC_OK;
}

int dec_parent_trunk(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, const uint8_t *occ, int64_t np, const ConvTiles &tilesP, const PairPlan &planP, int64_t planP_np,
                     int fmode, float **pA_out, bool *any_fused)
{
    TAKE_TOP(pF, float, np * m->C); TAKE_TOP(pA, float, np * m->C); TAKE_TOP(pB, float, np * m->C);
    float *Pp = nullptr;
    if (planP.valid()) { TAKE_TOP(pp, float, planP.pcap * 32); Pp = pp; }
    if (planP.valid() && fmode == 1) {
        // (profiling: a persistent launch counts as the convolutions it contains -- 5 here, 13 for a level's chain -- over its whole
        // time, heads / coder phases and barriers included: the conv roofline figure stays conservative)
        ConvRec rec = {0, 0, g, 1, 0, 0, (long long)np, 0, 5, 1};
        if (ctx->prof.on) GP_TRY(prof_event(ctx, st, &rec.e0));
        GP_TRY(fused_parent_trunk(ctx, st, m, planP, planP_np, occ, pF, pA, pB, Pp));
        if (ctx->prof.on) { GP_TRY(prof_event(ctx, st, &rec.e1)); ctx->prof.recs.push_back(rec); }
        *any_fused = true;
    } else {
        { StageTimer tm(ctx, st, ST_ELEM, (double)np * 129); GP_TRY(embed_occ(st, m->prior_emb, occ, np, pF, m->C)); }
        GP_TRY(dbg_mark(ctx, st, g * 100 + 1, pF, (size_t)np * 128));
        GP_TRY(run_trunk(ctx, g, st, m, 0, Trunk{pF, pA, pB}, tilesP, np, planP.valid() ? &planP : nullptr, Pp));
    }
    GP_TRY(dbg_mark(ctx, st, g * 100 + 2, pA, (size_t)np * 128));
    *pA_out = pA;
    return GPCC_OK;
}

int dec_child_lists(gpcc_ctx *ctx, hipStream_t sd, const gpcc_model *m, const Level *cur, const int32_t *cellP, const Level *chi, int32_t *cellC, bool child_plan,
                    unsigned long long *pairs_dev, PairPlan *planC, ConvTiles *tilesC)
{
    StageTimer tm(ctx, sd, ST_TILES, 0.0);
    if (child_plan) return pairplan_build(ctx, sd, cur, cellP, chi, cellC, m->k, planC, pairs_dev);
    const TileLevel tl = {chi, cur, cellP, cellC};
    const int R = conv_pick_rows(chi->n, m->k);
    const int64_t zero_base[1] = {0};
    TilePool pool;
    GP_TRY(tiles_build(ctx, sd, &tl, 1, m->k, R, conv_pick_height(chi->n, R), &pool, pairs_dev));
    GP_TRY(tiles_view(ctx, sd, pool, 0, 1, zero_base, tilesC));
    tm.add_bytes(pool.alg_bytes);
    return GPCC_OK;
}

int child_bufs_take(gpcc_ctx *ctx, const gpcc_model *m, int64_t nc, int64_t pcap, uint32_t nlanes, int64_t lane_syms, int64_t sym_bytes, ChildBufs *b)
{
    TAKE_TOP(cX, float, nc * m->C); TAKE_TOP(cA, float, nc * m->C); TAKE_TOP(cB, float, nc * m->C); TAKE_TOP(cU, float, nc * m->C);
    b->cX = cX; b->cA = cA; b->cB = cB; b->cU = cU; b->P = nullptr;
    if (pcap) { TAKE_TOP(pc, float, pcap * 32); b->P = pc; }
    TAKE_TOP(cdf, uint16_t, rc_rows_capacity(nlanes, lane_syms) * 16);  // interleaved rows + the decoder's look-ahead
    b->cdf = cdf; b->cdf_bytes = (size_t)rc_rows_capacity(nlanes, lane_syms) * 16 * 2;
    for (int s = 0; s < 4; ++s) { TAKE_TOP(sy, uint8_t, sym_bytes); b->sym[s] = sy; }
    return GPCC_OK;
}

int dec_child_fused(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, const PairPlan &planC, const float *pA, int64_t np, const Level &chi, const uint8_t *dbytes,
                    const LevelCoder &lc, const ChildBufs &b)
{
    FusedChild fa = {};
    fa.pA = pA; fa.np = np; fa.parent = chi.parent; fa.rkey = chi.rkey; fa.m2r = chi.m2r; fa.bytes = dbytes; fa.chunks = lc.chunks; fa.nlanes = lc.nlanes; fa.llog = lc.llog;
    fa.cpos = lc.cpos; fa.spos = lc.spos;
    for (int s = 0; s < 4; ++s) { fa.win_bytes[s] = lc.win_bytes[s]; fa.sym[s] = b.sym[s]; }
    fa.cX = b.cX; fa.cA = b.cA; fa.cB = b.cB; fa.cU = b.cU; fa.P = b.P; fa.cdf = b.cdf; fa.occ = chi.occ; fa.coder = lc.coder;
    ConvRec rec = {0, 0, g + 1, 1, 0, 0, (long long)chi.n, 0, 13, 1};
    if (ctx->prof.on) GP_TRY(prof_event(ctx, st, &rec.e0));
    GP_TRY(fused_child_level(ctx, st, m, planC, fa));
    if (ctx->prof.on) { GP_TRY(prof_event(ctx, st, &rec.e1)); ctx->prof.recs.push_back(rec); }
    return GPCC_OK;
}

int dec_child_trunk(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, const float *pA, const Level &chi, const ConvTiles &tilesC, const PairPlan *planC, const ChildBufs &b)
{
    const int64_t nc = chi.n;
    { StageTimer tm(ctx, st, ST_ELEM, (double)nc * (128 + 12 + 128)); GP_TRY(child_features(st, pA, chi.parent, chi.rkey, m->temb, nc, b.cX, m->C)); }
    GP_TRY(dbg_mark(ctx, st, g * 100 + 8, b.cX, (size_t)nc * 128));
    GP_TRY(run_trunk(ctx, g + 1, st, m, 5, Trunk{b.cX, b.cA, b.cB}, tilesC, nc, planC, b.P));  // -> cA
    GP_TRY(dbg_mark(ctx, st, g * 100 + 9, b.cA, (size_t)nc * 128));
    return GPCC_OK;
}

int dec_child_stage(gpcc_ctx *ctx, hipStream_t st, const gpcc_model *m, int g, int s, const Level &chi, const ConvTiles &tilesC, const PairPlan *planC, const LevelCoder &lc,
                    const ChildBufs &b)
{
    const int64_t nc = chi.n;
    const float *xin = b.cA;
    if (s) {
        StageTimer tm(ctx, st, ST_ELEM, (double)nc * (128 + 4 + s + 128));
        GP_TRY(stage_input_dec(st, b.cA, m->semb[s - 1], b.sym, lc.spos ? lc.spos : chi.m2r, s, nc, b.cU, m->C));
        xin = b.cU;
    }
    if (planC) {
        GP_TRY(plan_conv(st, *planC, ConvJob{xin, m->conv[10 + 2 * s], nullptr, b.cX}, b.P, 1));
        GP_TRY(plan_conv(st, *planC, ConvJob{b.cX, m->conv[10 + 2 * s + 1], nullptr, b.cB}, b.P, 0));
    } else {
        ConvBatch cb = {}; cb.C = m->C;
        GP_TRY(conv_chain_begin(ctx, st));
        cb.job[0] = ConvJob{xin, m->conv[10 + 2 * s], nullptr, b.cX};
        GP_TRY(sparse_conv(ctx, g + 1, st, cb, 1, tilesC, nc, 1));
        cb.job[0] = ConvJob{b.cX, m->conv[10 + 2 * s + 1], nullptr, b.cB};
        GP_TRY(sparse_conv(ctx, g + 1, st, cb, 1, tilesC, nc, 0));
        GP_TRY(conv_chain_end(ctx, st));
    }
    GP_TRY(dbg_mark(ctx, st, g * 100 + 10 + 5 * s, xin, (size_t)nc * 128)); GP_TRY(dbg_mark(ctx, st, g * 100 + 11 + 5 * s, b.cX, (size_t)nc * 128));
    GP_TRY(dbg_mark(ctx, st, g * 100 + 12 + 5 * s, b.cB, (size_t)nc * 128));
    HeadArgs ha = {}; ha.C = m->C;
    ha.x = b.cB; ha.n = nc; ha.stage_m = STAGE_M[s];
    ha.w1 = m->hw1[s]; ha.b1 = m->hb1[s]; ha.w2 = m->hw2[s]; ha.b2 = m->hb2[s]; ha.frag = m->hfrag[s];
    ha.m2r = chi.m2r; ha.cdf = b.cdf; ha.mode = 1; ha.pos = lc.cpos; ha.chunk_log2 = lc.llog; ha.nch = lc.nlanes;   // (pos, when given, is what the head uses)
    if (ctx->dbg_on) HIP_TRY(hipMemsetAsync(b.cdf, 0, b.cdf_bytes, st));   // developer trace: rows the head does not write read as zeros
    { StageTimer tm(ctx, st, ST_HEADS, (double)nc * (128 + 4 + stage_row_bytes(s))); GP_TRY(head_cdf(st, ha)); }
    GP_TRY(dbg_mark(ctx, st, g * 100 + 13 + 5 * s, b.cdf, b.cdf_bytes));
    return GPCC_OK;
}

}  // namespace gpcc
