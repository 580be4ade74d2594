/*
 * gauspcc.h -- C ABI of libgauspcc.so, the MI355X (gfx950) implementation of the
 * GausPcc hot path.  Plain pointers and sizes only; every device pointer is a HIP
 * device address on the context's device, every `stream` is a hipStream_t passed
 * as void* (NULL = the legacy default stream).  gpcc_encode / gpcc_decode also use a second stream the
 * context owns (event-fenced against `stream`); a context serves one call at a time.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repository root).  All functions return 0 on success or a negative
 * gpcc_status; gpcc_last_error() gives the thread-local message.  The Python shim
 * (gauspcc_amd/) raises on non-zero, mirroring the reference's Python exceptions.
 */
#ifndef GAUSPCC_H
#define GAUSPCC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPCC_API __attribute__((visibility("default")))

typedef enum {
    GPCC_OK = 0,
    GPCC_ERR_HIP = -1,        /* a HIP runtime call failed */
    GPCC_ERR_ARG = -2,        /* bad argument */
    GPCC_ERR_RANGE = -3,      /* the cloud leaves (-2^20, 2^20) AND its extent is 2^20 or more (any int32 position is fine) */
    GPCC_ERR_DUPLICATE = -4,  /* duplicate point (the reference silently corrupts occupancy here) */
    GPCC_ERR_FORMAT = -5,     /* malformed / truncated bitstream */
    GPCC_ERR_NOMEM = -6
} gpcc_status;

typedef enum { GPCC_F32 = 0, GPCC_F64 = 1, GPCC_I32 = 2, GPCC_I64 = 3 } gpcc_dtype;

typedef struct gpcc_ctx gpcc_ctx;     /* per-device context: workspace arena, staging buffers */
typedef struct gpcc_model gpcc_model; /* GausPcgc weights resident in HBM, MFMA-friendly layout */

GPCC_API const char *gpcc_last_error(void);
GPCC_API int gpcc_version(void);

GPCC_API int gpcc_ctx_create(int device, gpcc_ctx **out);
GPCC_API void gpcc_ctx_destroy(gpcc_ctx *ctx);
/* Chunked containers (chunk_log2 != 0) are this library's own layout (the versions' history: HISTORY.md section 5): version 4 (default) runs a
 * carry-propagating range coder in the lanes of a stream -- same 16-bit CDF rows and rate as torchac's coder, a third of the
 * decoder's dependent chain --, version 3 torchac's coder (arithmetic_kernel.cu:94-163) itself.  Sets what gpcc_encode and
 * gpcc_rc_encode / gpcc_rc_decode use; gpcc_decode reads versions 0 (the reference layout, pcc_utils.py:198-203) to 4. */
GPCC_API int gpcc_ctx_set_container_version(gpcc_ctx *ctx, int version);
/* bytes the context holds now: device (workspace arena, product buffer of the small levels) and pinned host staging.  The
 * reference's CLIs print torch.cuda.max_memory_allocated() (compress_ue_4stage_conv.py:283); this library allocates its
 * workspace itself, so its CLIs add this figure.  Either pointer may be null. */
GPCC_API int gpcc_ctx_bytes(const gpcc_ctx *ctx, int64_t *device_bytes, int64_t *pinned_bytes);

/* developer counter: kernel launches the calling thread has enqueued through this library since the last reset (reset != 0
 * zeroes it); memcpy / memset nodes are not counted.  bench.py reports kernels per decode with it. */
GPCC_API long long gpcc_debug_launches(int reset);

/* Device-side faults that must not abort the process (today: a device-wide scan whose tiles made no progress for ~10 s) raise a sticky
 * word in the context instead of trapping.  Every entry point that synchronises checks it and returns GPCC_ERR_HIP once (the word and
 * the scan state are reset: the next call starts clean); callers of the stage-level entry points that return before their work has run
 * call this after synchronising the stream.  GPCC_OK when nothing was raised. */
GPCC_API int gpcc_device_error_check(gpcc_ctx *ctx);

/* ---- a2  calculate_morton_order            src/gs_compress/HAC/utils/pcc_utils.py:12-22
 * perm_out[N] (int64, device): argsort of x + y*M + z*M^2 after the per-axis min shift
 * (M = max over all axes + 1), i.e. the (z,y,x) raster order; stable for equal keys. */
GPCC_API int gpcc_raster_order(gpcc_ctx *ctx, const void *xyz_dev, int dtype, int64_t n,
                      int64_t *perm_out_dev, void *stream);

/* ---- a1  voxelise (caller side)     src/ai_pcc/GausPcgc/compress_ue_4stage_conv.py:89-94: `xyz / 0.001 + 131072` (when the
 * data is not pre-quantised) then `torch.round(xyz / posQ).int()`; HAC/scene/gaussian_model.py:1107: `round(anchor / voxel)`.
 * out[i] = int32(rint(((x[i] / d1) + add) / d2)) over the 3n coordinates, evaluated in the array's OWN dtype (GPCC_F32 or
 * GPCC_F64) one correctly rounded operation at a time, as the reference's numpy / torch-CPU expressions are; flags bit 0
 * enables the `/ d1 + add` step, bit 1 the `/ d2` step.  xyz_dev (n,3) and out_dev (n,3) int32 are device pointers. */
#define GPCC_VOX_SCALE 1
#define GPCC_VOX_POSQ 2
GPCC_API int gpcc_voxelise(gpcc_ctx *ctx, const void *xyz_dev, int dtype, int64_t n, double d1, double add, double d2, int flags,
                  int32_t *out_dev, void *stream);

/* ---- Network(channels, kernel_size).load_state_dict     pcc_utils.py:65-67, 266-268
 * tensors: GPCC_T_COUNT host pointers to contiguous float32 arrays, upstream layouts
 * (conv kernels (k^3, Cin, Cout); Linear (out, in)); order = gpcc_tensor_id. */
typedef enum {
    GPCC_T_PRIOR_EMB = 0,  /* prior_embedding.weight (256, C) */
    GPCC_T_CONV0 = 1,      /* 18 conv kernels: prior_resnet.{0,2.conv0,2.conv1,3.conv0,3.conv1},
                              target_resnet.{same five}, spatial_conv_s{0..3}.{0,2} */
    GPCC_T_TEMB = 19,      /* target_embedding.target_res_embedding.weight (8, C) */
    GPCC_T_HW1 = 20,       /* pred_head_s{0..3}.0.weight (C, C) */
    GPCC_T_HB1 = 24,       /* pred_head_s{0..3}.0.bias   (C)    */
    GPCC_T_HW2 = 28,       /* pred_head_s{0..3}.2.weight ({2,2,4,16}, C) */
    GPCC_T_HB2 = 32,       /* pred_head_s{0..3}.2.bias   ({2,2,4,16})    */
    GPCC_T_SEMB = 36,      /* pred_head_s{1,2,3}_emb.weight ({2,4,16}, C) */
    GPCC_T_COUNT = 39
} gpcc_tensor_id;

GPCC_API int gpcc_model_create(gpcc_ctx *ctx, int channels, int kernel_size, const float *const *tensors,
                      gpcc_model **out);
GPCC_API void gpcc_model_destroy(gpcc_model *m);

#define GPCC_STATS_IDEAL_BITS 1
typedef struct {
    int64_t num_points;
    int64_t num_bytes;
    int32_t num_levels;        /* stored levels L (base + coded) */
    int32_t flags;             /* IN: GPCC_STATS_IDEAL_BITS asks gpcc_encode for ideal_bits (costs ~4 % of an encode); OUT: 0 */
    int64_t level_nodes[24];   /* nodes per stored level, base first */
    int64_t coded_nodes;       /* sum of nodes over coded levels */
    int64_t conv_pairs;        /* sum over all 18*levels convs of (output node, present neighbour) pairs */
    double device_ms;          /* wall time between the syncs that bracket the call */
    double ideal_bits;         /* encode only, when requested through flags: sum over coded symbols of clamp(-log2(p_gt + 1e-10), 0, 50), the reference's
                                  bpp estimator before the division by N (network_ue_4stage_conv.py:100-182, a14) */
} gpcc_stats;

/* ---- a12  compress_point_cloud (the timed span :78-189 + container :192-203)
 * xyz_dev: (N,3) int32 device, duplicate-free, any order.  chunk_log2 = 0 writes the
 * reference container layout (one torchac range-coder stream per level and stage: a stream is ONE
 * dependent chain, so for this layout the coder -- not the network -- runs on the host, on the library's own
 * torchac coder, csrc/hostcoder.hpp); 6..14 writes the chunked container whose streams are cut into
 * chunks of at most 2^chunk_log2 symbols that decode in parallel.  A chunk must fit the staged decoder's LDS
 * window (64 KiB; 16 KiB for the 16-ary streams): should one come out larger -- possible only at chunk_log2 >= 13 with
 * a model that spends more than 8 bits per 16-ary symbol -- the cloud is coded again with chunk_log2 - 1 (the header
 * records the value used; readers never see the request).  posq_f16 = bits of np.float16(posQ).
 * On success *bytes_out points at a context-owned host buffer valid until the next call. */
GPCC_API int gpcc_encode(gpcc_ctx *ctx, const gpcc_model *m, const int32_t *xyz_dev, int64_t n,
                int chunk_log2, uint16_t posq_f16, const uint8_t **bytes_out, int64_t *nbytes_out,
                gpcc_stats *stats, void *stream);

/* ---- a13  decompress_point_cloud (the timed span :279-385)
 * bytes: the whole .bin file (host).  On success *xyz_dev_out points at a context-owned
 * (N,3) int32 DEVICE buffer (integer leaf coordinates, before the posQ multiply) in the
 * reference's output order (FCG of the raster-sorted last level, pcc_utils.py:375),
 * valid until the next call on this context. */
GPCC_API int gpcc_decode(gpcc_ctx *ctx, const gpcc_model *m, const uint8_t *bytes, int64_t nbytes,
                const int32_t **xyz_dev_out, int64_t *n_out, uint16_t *posq_f16_out,
                gpcc_stats *stats, void *stream);

/* The same into a caller-owned DEVICE buffer of capacity_points x 3 int32 (the chunked containers carry the point count
 * in their header -- u32 at byte 8 + 4 L, L = byte 6 -- so a caller can size it before the call); fails with
 * GPCC_ERR_ARG when the cloud does not fit.  Saves the copy out of the context's buffer. */
GPCC_API int gpcc_decode_to(gpcc_ctx *ctx, const gpcc_model *m, const uint8_t *bytes, int64_t nbytes,
                int32_t *xyz_dev, int64_t capacity_points, int64_t *n_out, uint16_t *posq_f16_out,
                gpcc_stats *stats, void *stream);

/* ---- batched a12 / a13: K scenes through ONE chain of launches
 * Reference: the codec's coordinate tensor has a batch column -- coords = [b, x, y, z], src/gs_compress/HAC/utils/pcc_utils.py:73
 * (b pinned to 0), sort_CF orders by batch last (src/ai_pcc/GausPcgc/kit/op.py:17-30) -- and the stand-alone CLI loops over files
 * (src/ai_pcc/GausPcgc/compress_ue_4stage_conv.py:72-75).  Every scene gets its own container, byte-identical to what gpcc_encode
 * writes for it alone; the scenes share every convolution / head / coder / scan launch of an octree depth (csrc/forest.hpp).
 * xyz_dev / n / posq_f16: HOST arrays of nscenes device pointers, point counts and posQ bits.  On success *bytes_out points at a
 * context-owned host buffer holding the containers one after the other, scene i at [offsets_out[i], offsets_out[i + 1])
 * (offsets_out: nscenes + 1 entries, caller-owned).  stats (nullable): nscenes records; conv_pairs and device_ms of the whole
 * batch are in stats[0].  *batched_out (nullable): 1 when the scenes shared one tree, 0 when they were coded one by one (the
 * reference container layout chunk_log2 = 0, a scene whose extent exceeds 2^18 voxels, more than 256 scenes, or more scenes than the
 * 21-bit coordinate frame stacks: same bytes either way). */
GPCC_API int gpcc_encode_batch(gpcc_ctx *ctx, const gpcc_model *m, const int32_t *const *xyz_dev, const int64_t *n, int nscenes,
                int chunk_log2, const uint16_t *posq_f16, const uint8_t **bytes_out, int64_t *offsets_out,
                gpcc_stats *stats, int *batched_out, void *stream);
/* bytes / nbytes: HOST arrays of nscenes container pointers (host memory) and sizes; xyz_dev / capacity_points: nscenes caller-owned
 * DEVICE buffers ((capacity, 3) int32 each; a chunked container's header carries its point count, see gpcc_decode_to).  Every
 * scene's points come out as gpcc_decode gives them for that container alone.  Containers of the reference layout or of mixed
 * versions are decoded one by one (*batched_out = 0). */
GPCC_API int gpcc_decode_batch(gpcc_ctx *ctx, const gpcc_model *m, const uint8_t *const *bytes, const int64_t *nbytes, int nscenes,
                int32_t *const *xyz_dev, const int64_t *capacity_points, int64_t *n_out, uint16_t *posq_f16_out,
                gpcc_stats *stats, int *batched_out, void *stream);

/* Live timing of the dominant kernel (the sparse convolution): while enabled, every launch is
 * bracketed by HIP events on the stream it runs on.  conv_pair_jobs = sum over launches of
 * (output node, present neighbour) pairs x jobs in the launch; algorithmic flops = 2*C*C*conv_pair_jobs. */
typedef struct {
    double conv_ms;
    int64_t conv_launches;
    int64_t conv_pair_jobs;
    /* the decoder's persistent small-level launches (csrc/fused.hpp), kept apart from the k_sparse_conv family above: their time
     * covers whole chains of layers (heads, range-decoder phases and grid barriers included); fused_launches counts the
     * convolutions they contain (13 per level chain, 5 per prior trunk), fused_pair_jobs their (pair, convolution) products */
    double fused_ms;
    int64_t fused_launches;
    int64_t fused_pair_jobs;
} gpcc_profile;
GPCC_API int gpcc_profile_enable(gpcc_ctx *ctx, int on);   /* 0 off, 1 the convolution, 2 also the stages below (these reset the accumulators); 3 = stop recording, keep what was collected */
GPCC_API int gpcc_profile_get(gpcc_ctx *ctx, gpcc_profile *out);

/* The HBM-bound stages of gpcc_encode / gpcc_decode (SURVEY.md 8d "which roofline"), bracketed by HIP events on the stream
 * their kernels run on while gpcc_profile_enable(ctx, 2) is in force: ms = bracketed time, bytes = the ALGORITHMIC traffic of
 * the bracketed work (an ideal layer-by-layer implementation's reads + writes; formulas in HISTORY.md section 4). */
typedef struct {
    char name[48];
    double ms;
    double bytes;
    int64_t brackets;
    double critical_ms;   /* of ms: the part during which no convolution bracket was open on any stream of the call -- the octree / tile-list
                           * work of a decode runs beside the parent trunk's convolutions, the encoder's rank pass beside its first trunk */
} gpcc_stage;
GPCC_API int gpcc_profile_stages(gpcc_ctx *ctx, gpcc_stage *out, int cap, int *n_out);

/* Developer trace (no reference counterpart): while enabled, gpcc_decode records a checksum of every intermediate buffer
 * of every level (features, level structure, symbols) on the stream that produced it; _get returns the (tag, sum) pairs of
 * the decode that just returned (tag = 100 x level + buffer id, codec.hip) and clears the list.  Two runs of one container
 * must give identical lists: the first difference names the stage that misbehaved (tools/inflight_check.py). */
GPCC_API int gpcc_debug_trace_enable(gpcc_ctx *ctx, int on);
GPCC_API int gpcc_debug_trace_get(gpcc_ctx *ctx, int *tags, unsigned long long *sums, int cap);
/* keep a device copy of every marked buffer whose tag % 100 == tag_mod (-1: none); _get copies the last copy of `tag` out and
 * returns its size in bytes (-1: no such copy) */
GPCC_API int gpcc_debug_capture(gpcc_ctx *ctx, int tag_mod);
GPCC_API long long gpcc_debug_capture_get(gpcc_ctx *ctx, int tag, void *host, long long cap);

/* The library's exclusive prefix sum of uint32 values (every level build, rank derivation, sort pass and tile list runs on it: no
 * reference counterpart, torch.cumsum / unique do this job upstream).  in / out device arrays of n values (in == out allowed), in2 /
 * out2 optional: a second independent scan of the same length in the same launch where the size allows; total_dev (nullable)
 * receives the sum of `in`.  Exported for the unit tests of the scan kernels (tests/test_gpu_primitives.py). */
GPCC_API int gpcc_debug_exclusive_scan(gpcc_ctx *ctx, const uint32_t *in_dev, uint32_t *out_dev, const uint32_t *in2_dev, uint32_t *out2_dev, int64_t n,
                                       uint32_t *total_dev, void *stream);

/* Write n host buffers to n files on `threads` native threads (<= 0: 8).  The attribute loops of HAC / HAC++ produce one `.b` file per
 * 3 000-anchor slice and attribute (HAC/scene/gaussian_model.py:1176-1213: 1 002 files per million anchors; HAC++: 2 338) -- in Python that is
 * ~55 us of interpreter time per file under the GIL; here it is open / write / close.  Returns GPCC_OK or GPCC_ERR_ARG with the first
 * path that failed in gpcc_last_error().  No context, no GPU call. */
GPCC_API int gpcc_write_files(const char *const *paths, const uint8_t *const *data, const int64_t *sizes, int n, int threads);

/* The read side: n whole files into one blob, file i at offsets_out[i] .. offsets_out[i + 1] (offsets_out has n + 1 entries), read by `threads`
 * native threads (<= 0: 8).  The decoders of the attribute loops read 1 002 (HAC) / 2 343 (HAC++) slice files per million anchors: 14 / 27 ms of
 * interpreter time in Python.  *blob_out belongs to the calling thread and is valid until its next call.  GPCC_OK or GPCC_ERR_ARG with the first
 * file that could not be read. */
GPCC_API int gpcc_read_files(const char *const *paths, int n, int threads, const uint8_t **blob_out, int64_t *offsets_out);

/* Copy out of a context-owned device buffer (e.g. gpcc_decode's points) into caller memory,
 * ordered on `stream`; returns after the copy has completed. */
GPCC_API int gpcc_memcpy_d2d(gpcc_ctx *ctx, void *dst_dev, const void *src_dev, int64_t nbytes, void *stream);

/* ---- stage-level entry points (what the reference does through torch / torchsparse /
 * torchac calls); used by the parity tests and by callers that want a single stage. */

/* op.sort_CF order of integer coordinates             src/ai_pcc/GausPcgc/kit/op.py:17-30
 * xyz (n,3) int32 device -> perm (n) uint32 device such that xyz[perm] is (z,y,x) sorted. */
GPCC_API int gpcc_sort_zyx(gpcc_ctx *ctx, const int32_t *xyz_dev, int64_t n, uint32_t *perm_dev, void *stream);

/* FOG loop                                            kit/nn.py:38-55, pcc_utils.py:83-89
 * Builds the octree of xyz on the device and copies every stored level to the host in
 * raster order: coords_out[d] (n_d,3) int32, occ_out[d] (n_d) uint8; capacity per level
 * cap_nodes.  levels_out/level_nodes_out as in gpcc_stats. */
GPCC_API int gpcc_build_octree(gpcc_ctx *ctx, const int32_t *xyz_dev, int64_t n, int32_t *levels_out,
                      int64_t *level_nodes_out, int32_t **coords_out_host, uint8_t **occ_out_host,
                      int64_t cap_nodes, void *stream);

/* spnn.Conv3d (stride 1) on raster-sorted coordinates: torchsparse 2.1.0 (not in tree), call
 * sites network_ue_4stage_conv.py:17-62.  in/out (n,C) float32 device in LOGICAL channel
 * order; w = upstream (k^3,C,C) host; residual may be NULL.  Also returns the number of
 * (node, neighbour) pairs.  relu: bit 0 = ReLU; bit 1 (test knob) = run the pair-plan form the decoder uses on its small levels
 * (csrc/fused.hpp; at most 16384 points) instead of the block-tile kernels -- same sums in the same order, same bits. */
GPCC_API int gpcc_conv3d(gpcc_ctx *ctx, const int32_t *xyz_sorted_dev, int64_t n, int channels, int kernel_size,
                const float *in_dev, const float *w_host, const float *res_dev, int relu,
                float *out_dev, int64_t *pairs_out, void *stream);

/* pred_head_s* + cdf + _convert_to_int_and_normalize  network_ue_4stage_conv.py:65-94,
 * pcc_utils.py:146-171, kit/op.py:50-79.  x (n,C) device logical order; prob (n,m) float32,
 * cdf (n,m+1) uint16 device outputs (either may be NULL). */
GPCC_API int gpcc_head_cdf(gpcc_ctx *ctx, const float *x_dev, int64_t n, int channels, int m,
                  const float *w1_host, const float *b1_host, const float *w2_host, const float *b2_host,
                  float *prob_dev, uint16_t *cdf_dev, void *stream);

/* torchac.encode_int16_normalized_cdf / decode_int16_normalized_cdf   pcc_utils.py:174-177,322-366
 * cdf (n,Lp) uint16 device, sym (n) uint8 device.  chunk_log2 as in gpcc_encode
 * (0 = one stream, bytes identical to torchac's).  encode: *bytes_out context-owned host buffer.
 * For chunk_log2 != 0 both calls code the lanes with the coder of the CONTEXT's container version (gpcc_ctx_set_container_version:
 * 4 = the carry-propagating coder, the default; 3 = torchac's): a caller holding version-3 stage streams sets version 3 first. */
GPCC_API int gpcc_rc_encode(gpcc_ctx *ctx, const uint16_t *cdf_dev, int lp, const uint8_t *sym_dev, int64_t n,
                   int chunk_log2, const uint8_t **bytes_out, int64_t *nbytes_out, void *stream);
GPCC_API int gpcc_rc_decode(gpcc_ctx *ctx, const uint16_t *cdf_dev, int lp, const uint8_t *bytes, int64_t nbytes,
                   int64_t n, int chunk_log2, uint8_t *sym_dev, void *stream);

/* ================= HAC attribute-side kernels (a15, a17-a19) ================= */

/* arithmetic.calculate_cdf(mean, scale, Q, min_value, max_value) -> lower (n, max-min+2) float32
 * HAC/submodules/arithmetic.zip!arithmetic/arithmetic.cpp:4-15, arithmetic_kernel.cu:7-54.  All device. */
GPCC_API int gsac_calculate_cdf(gpcc_ctx *ctx, const float *mean_dev, const float *scale_dev, const float *q_dev, int64_t n,
                                int min_value, int max_value, float *lower_dev, void *stream);

/* arithmetic.arithmetic_encode(sym int16 (n), cdf float (n,Lp), chunk_size, N, Lp) -> (bytes uint8, cnt int32[chunks])
 * arithmetic.cpp:18-29, arithmetic_kernel.cu:94-232.  sym / cdf device; outputs are context-owned HOST buffers. */
GPCC_API int gsac_encode(gpcc_ctx *ctx, const int16_t *sym_dev, const float *cdf_dev, int chunk_size, int64_t n, int lp,
                         const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream);

/* arithmetic.arithmetic_decode(cdf, bytes, cnt, chunk_size, N, Lp) -> sym int16 (n)
 * arithmetic.cpp:32-43, arithmetic_kernel.cu:265-403.  cdf device, bytes / cnt host, sym_out device. */
GPCC_API int gsac_decode(gpcc_ctx *ctx, const float *cdf_dev, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size,
                         int64_t n, int lp, int16_t *sym_out_dev, void *stream);

/* The same coder over already-integerised rows: torchac.encode_int16_normalized_cdf / decode_int16_normalized_cdf
 * (requirements.txt:6; call sites src/gs_compress/HAC/utils/pcc_utils.py:174-177, TC-GS/utils/encodings.py:38-174).
 * cdf (n, Lp) uint16 device.  chunk_size = n gives torchac's single stream. */
GPCC_API int gsac_encode_u16(gpcc_ctx *ctx, const int16_t *sym_dev, const uint16_t *cdf_dev, int chunk_size, int64_t n, int lp,
                             const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream);
GPCC_API int gsac_decode_u16(gpcc_ctx *ctx, const uint16_t *cdf_dev, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size,
                             int64_t n, int lp, int16_t *sym_out_dev, void *stream);

/* The same coder with ONE row for all n symbols (lp = 2 .. 4 entries, host floats): the Bernoulli coder of HAC's hash tables and masks
 * (HAC/utils/encodings_cuda.py:228-262 builds an (n, 3) table whose rows are all (0, 1 - p, 1) -- 120 MB for the ten million mask bits of a
 * million anchors).  Byte-identical to gsac_encode / gsac_decode on that table. */
GPCC_API int gsac_encode_const(gpcc_ctx *ctx, const int16_t *sym_dev, const float *row_host, int chunk_size, int64_t n, int lp,
                               const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream);
GPCC_API int gsac_decode_const(gpcc_ctx *ctx, const float *row_host, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size,
                               int64_t n, int lp, int16_t *sym_out_dev, void *stream);

/* torchac's coder itself, on HOST arrays and one host thread -- the drop-in for torchac.encode_int16_normalized_cdf /
 * decode_int16_normalized_cdf (torchac 0.9.3; call sites TC-GS/utils/encodings.py:84-176, CAT-3DGS/utils/encodings.py:39-175,
 * HAC/utils/pcc_utils.py:174-177): ONE stream for the whole tensor, byte-identical to torchac's.  A single stream is a single
 * dependent chain, which a host core runs several times faster than one GPU lane; gauspcc_amd.torchac builds the integer rows
 * where the caller's tensors live and codes here.  cdf (n, lp) uint16 rows, sym (n) int16, all host memory; out: cap bytes
 * (4 n + 64 always suffice).  No context, no GPU call. */
GPCC_API int gsac_host_encode_u16(const int16_t *sym, const uint16_t *cdf, int64_t n, int lp, uint8_t *out, int64_t cap, int64_t *nbytes_out);
GPCC_API int gsac_host_decode_u16(const uint16_t *cdf, const uint8_t *bytes, int64_t nbytes, int64_t n, int lp, int16_t *sym_out);
/* The same for torchac.encode_float_cdf / decode_float_cdf on a HOST float table (torchac's own calling convention: CPU tensors;
 * TC-GS/utils/encodings.py:84-129 moves its table to the CPU first): row i is integerised on the fly as torchac's
 * _convert_to_int_and_normalize does -- rint(cdf * (2^16 - (lp - 1))) + j modulo 2^16, fp32 -- so the table is read once,
 * 4 bytes per entry, and no int16 copy of it is ever built.  Bytes == the _u16 form on the pre-integerised rows.  lp <= 65536. */
GPCC_API int gsac_host_encode_f32(const int16_t *sym, const float *cdf, int64_t n, int lp, uint8_t *out, int64_t cap, int64_t *nbytes_out);
GPCC_API int gsac_host_decode_f32(const float *cdf, const uint8_t *bytes, int64_t nbytes, int64_t n, int lp, int16_t *sym_out);

/* encoder_gaussian / decoder_gaussian in one call each, WITHOUT the (n, max-min+2) float CDF table of
 * arithmetic.calculate_cdf (src/gs_compress/HAC/utils/encodings_cuda.py:336-371, 399-433):
 *   encode: x_int = round(x / Q), min/max over the slice, the two CDF entries of every symbol evaluated on the fly,
 *           the chunked coder -> (min, max, bytes, cnt) = what the reference writes into the `.b` file;
 *   decode: the <= 64 entries a decoding wave compares evaluated on the fly; x = (sym + min) * Q.
 * Byte-identical to gsac_calculate_cdf + gsac_encode (same entry formula, same integerisation).
 * x / mean / scale / Q device (n); bytes / cnt host; min / max are the float values the file stores. */
GPCC_API int gsac_encode_gaussian(gpcc_ctx *ctx, const float *x_dev, const float *mean_dev, const float *scale_dev, const float *q_dev, int64_t n,
                                  int chunk_size, float *min_out, float *max_out, const uint8_t **bytes_out, int64_t *nbytes_out,
                                  const int32_t **cnt_out, int64_t *nchunks_out, void *stream);
GPCC_API int gsac_decode_gaussian(gpcc_ctx *ctx, const float *mean_dev, const float *scale_dev, const float *q_dev, int64_t n, float min_value,
                                  float max_value, const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, float *x_out_dev,
                                  void *stream);

/* HAC++'s Gaussian-MIXTURE coder (src/gs_compress/HAC-plus/utils/encodings_cuda.py:177-317; callers
 * HAC-plus/scene/gaussian_model.py:1315, 1499): the CDF row of element i is
 *     lower[i][t] = clamp( sum_c calculate_cdf(mean_c[i], scale_c[i], Q[i])[t] * prob_c[i], 0, 1 ),   c = 0 .. k-1 in list order, fp32
 * with the same integerisation, chunking, symbol range and `.b` layout as the single Gaussian.  As above the table is never
 * materialised: gsac_encode_gaussian_mixed == calculate_cdf x k, multiply, add, clamp, arithmetic_encode of :205-247 in one
 * call, gsac_decode_gaussian_mixed == :285-317.  mean / scale / prob: host arrays of k (1..4) device pointers, (n) each.
 * gsac_calculate_cdf_mixed writes the table itself, (n, max - min + 2) fp32 on the device (tests; two-step callers). */
GPCC_API int gsac_encode_gaussian_mixed(gpcc_ctx *ctx, const float *x_dev, const float *const *mean_dev, const float *const *scale_dev,
                                        const float *const *prob_dev, int k, const float *q_dev, int64_t n, int chunk_size, float *min_out,
                                        float *max_out, const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out,
                                        int64_t *nchunks_out, void *stream);
GPCC_API int gsac_decode_gaussian_mixed(gpcc_ctx *ctx, const float *const *mean_dev, const float *const *scale_dev, const float *const *prob_dev, int k,
                                        const float *q_dev, int64_t n, float min_value, float max_value, const uint8_t *bytes, int64_t nbytes,
                                        const int32_t *cnt, int chunk_size, float *x_out_dev, void *stream);
GPCC_API int gsac_calculate_cdf_mixed(gpcc_ctx *ctx, const float *const *mean_dev, const float *const *scale_dev, const float *const *prob_dev, int k,
                                      const float *q_dev, int64_t n, int min_value, int max_value, float *lower_dev, void *stream);

/* The same for every slice of an attribute in ONE call: conduct_encoding / conduct_decoding code each 3000-anchor
 * slice into its own `.b` file (own min / max, hence own alphabet; HAC/scene/gaussian_model.py:1123-1206, 1262-1311) --
 * 334 slices x 3 attributes per million anchors, each a serial chain of 10000-symbol chunks.  Here all chunks of all
 * slices are coded concurrently.  slice_start (nslices + 1, host): element ranges, slice_start[0] = 0.
 * encode: min_out / max_out (nslices, host); cnt lists the chunks slice by slice (ceil(len / chunk_size) each), bytes
 * are their payloads in that order -- the caller cuts them into the per-slice files.  decode: the reverse. */
GPCC_API int gsac_encode_gaussian_slices(gpcc_ctx *ctx, const float *x_dev, const float *mean_dev, const float *scale_dev, const float *q_dev,
                                         const int64_t *slice_start, int nslices, int chunk_size, float *min_out, float *max_out,
                                         const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream);
GPCC_API int gsac_decode_gaussian_slices(gpcc_ctx *ctx, const float *mean_dev, const float *scale_dev, const float *q_dev, const int64_t *slice_start,
                                         int nslices, const float *min_value, const float *max_value, const uint8_t *bytes, int64_t nbytes,
                                         const int32_t *cnt, int chunk_size, float *x_out_dev, void *stream);
/* The same for HAC++'s K-component mixture (gsac_encode_gaussian_mixed): all 3000-anchor slices of ONE ten-channel group of `feat` in one
 * call -- conduct_encoding / conduct_decoding code feat as five such groups per slice, every group's second component coming from the
 * channel-context MLP on the groups already coded (HAC-plus/scene/gaussian_model.py:1300-1321, 1484-1504). */
GPCC_API int gsac_encode_gaussian_mixed_slices(gpcc_ctx *ctx, const float *x_dev, const float *const *mean_dev, const float *const *scale_dev,
                                               const float *const *prob_dev, int k, const float *q_dev, const int64_t *slice_start, int nslices, int chunk_size,
                                               float *min_out, float *max_out, const uint8_t **bytes_out, int64_t *nbytes_out, const int32_t **cnt_out,
                                               int64_t *nchunks_out, void *stream);
GPCC_API int gsac_decode_gaussian_mixed_slices(gpcc_ctx *ctx, const float *const *mean_dev, const float *const *scale_dev, const float *const *prob_dev, int k,
                                               const float *q_dev, const int64_t *slice_start, int nslices, const float *min_value, const float *max_value,
                                               const uint8_t *bytes, int64_t nbytes, const int32_t *cnt, int chunk_size, float *x_out_dev, void *stream);

/* TC-GS / CAT-3DGS's attribute files: ONE torchac stream per file, no chunk table (TC-GS/utils/encodings.py:84-146; the loop that calls it per
 * 1 000-anchor slice: TC-GS/scene/gaussian_model.py:1197-1271, 1358-1420).  The CDF row of element i is the reference's
 *     lower[i][j] = Normal(mean[i], scale[i]).cdf((min + j - 0.5) * Q[i]),   j = 0 .. max - min + 1,
 * 0.5 (1 + erf((v - mean) (1 / scale) / sqrt(2))) in float32 steps (csrc/attributes.hip: normal_cdf_entry) -- torch.distributions' formula, not the
 * erfc form of arithmetic.calculate_cdf above -- integerised as torchac does: rint(entry * (65536 - (lp - 1))) + j; c_high of the last symbol is 2^16.
 *   gsac_normal_cdf_rows        the integer rows (n, max - min + 2) uint16 on the device (tests; callers that want torchac's two-step form).
 *   gsac_encode_normal_streams  every slice [slice_start[s], slice_start[s + 1]) (nslices + 1 host entries, slice_start[0] = 0) is quantised,
 *       x_int = round(x / Q) (float32 division, ties to even), gets its own min / max, and is coded as ONE carry-less stream: the bytes of
 *       gsac_host_encode_u16 on the slice's rows from gsac_normal_cdf_rows.  min_out / max_out (nslices, host); *cnt_out: nslices byte counts,
 *       *bytes_out: the streams concatenated in slice order (context-owned host buffers, valid until the context's next call).  A slice of
 *       length 0 gives an empty stream and min = max = 0.  No CDF table is built: an encoded symbol needs two entries, evaluated in registers.
 *       GPCC_ERR_RANGE when a slice spans more than int16 symbols; GPCC_ERR_ARG when a mean is not finite, a scale not finite or not positive,
 *       a Q not finite or zero (checked on the device before anything computes with them), or when the call must be split: at most 65 535 slices
 *       whose count times (2 longest + 47) bytes stays below 4 GiB (byte offsets are 32 bits), a slice below 2^30 symbols.  Workspace: the
 *       context's arena grows to about 8 bytes x (non-empty slices x LONGEST slice) + 4 bytes per symbol -- every stream gets the longest one's
 *       slots -- so slices of very unequal lengths cost far more than their symbols; callers with such slices group them by length or split the call.
 *   gsac_decode_normal_streams  the reverse, one wave per stream: x_out[i] = (sym + min) * Q[i].  bytes / cnt host, as the encoder returned them;
 *       bytes past a stream's count read as zero and symbols stay inside the alphabet, so a short or foreign file gives some values, never a fault.
 * mean / scale / Q / x device (n = slice_start[nslices]). */
GPCC_API int gsac_normal_cdf_rows(gpcc_ctx *ctx, const float *mean_dev, const float *scale_dev, const float *q_dev, int64_t n, int min_value,
                                  int max_value, uint16_t *rows_dev, void *stream);
GPCC_API int gsac_encode_normal_streams(gpcc_ctx *ctx, const float *x_dev, const float *mean_dev, const float *scale_dev, const float *q_dev,
                                        const int64_t *slice_start, int nslices, float *min_out, float *max_out, const uint8_t **bytes_out,
                                        int64_t *nbytes_out, const int32_t **cnt_out, void *stream);
GPCC_API int gsac_decode_normal_streams(gpcc_ctx *ctx, const float *mean_dev, const float *scale_dev, const float *q_dev, const int64_t *slice_start,
                                        int nslices, const float *min_value, const float *max_value, const uint8_t *bytes, int64_t nbytes,
                                        const int32_t *cnt, float *x_out_dev, void *stream);

/* CAT-3DGS's channel-wise context chain (CAT-3DGS/scene/gaussian_model.py:1451-1552): the attribute streams of a slice of anchors depend on one
 * another PER ANCHOR -- feat group i is coded under mean_i + dmean, clamp(scale_i + dscale, 1e-9) with (dmean | dscale) =
 * Linear(dep_ch, dh) - ReLU - Linear(dh, 2 ch) of the channels [0, dep_ch) already decoded, and scaling / offsets may depend the same way on all
 * of feat.  gsac_decode_normal_chain decodes every stage of every slice in ONE launch: a workgroup per slice, a wave per stage, the slice's anchors
 * in blocks of block_anchors; in step t the wave of stage k works on block t - lag, so what its MLP reads was decoded in an earlier step (waves meet
 * at one workgroup barrier per step; nblocks + max lag steps).  The files are gsac_encode_normal_streams' (one stream per stage and slice), the rows
 * normal_cdf_entry's, the MLP gshac_mlp2's specified fp32 order (bias, then fmaf over k ascending; ReLU x > 0 ? x : 0), mean = ctx + dmean one
 * rounded add, scale = fmaxf(ctx + dscale, 1e-9f): the values equal those of gshac_mlp2 + gsac_decode_normal_streams run stage after stage.
 * One record per stage (at most 8): */
typedef struct {
    int32_t ch;                    /* symbols per anchor, 1..64 */
    int32_t dep_ch;                /* the MLP reads the decoded feat channels [0, dep_ch), <= 64; 0: no MLP (w1..b2 NULL) */
    int32_t dh;                    /* hidden units, <= 128 */
    int32_t lag;                   /* 0 without an MLP; otherwise larger than the lag of every stage that publishes a channel below dep_ch */
    int32_t mean_col, scale_col;   /* first columns of the stage's base mean / scale in a row of ctx_dev */
    int32_t feat_col;              /* >= 0: a feat stage, its values are channels [feat_col, feat_col + ch) for the later stages' MLPs; -1 otherwise */
    int32_t out_col, out_pitch;    /* the stage writes out_dev[a * out_pitch + out_col + c], a = 0 .. n - 1, c = 0 .. ch - 1 */
    int32_t keep_group;            /* with keep_dev: element c of anchor a is coded when keep_dev[a * (ch / keep_group) + c / keep_group] != 0 (offsets: 3);
                                      the others are written as 0 and take no symbol */
    const float *w1, *b1, *w2, *b2;   /* device: (dh, dep_ch), (dh), (2 ch, dh), (2 ch) row-major as nn.Linear stores them */
    const float *q_dev;            /* (n) the step size of every anchor, computed by the caller with the encoder's expression */
    float *out_dev;
    const uint8_t *keep_dev;       /* or NULL */
    const uint8_t *bytes;          /* host: the stage's streams, slice after slice */
    int64_t nbytes;
    const int32_t *cnt;            /* host (nslices): byte count of every stream */
    const float *min_value, *max_value;   /* host (nslices) */
} gsac_chain_stage;
/* ctx_dev (n, ctx_pitch) device; slice s holds the anchors [s * slice_anchors, min(n, (s + 1) * slice_anchors)), nslices = ceil(n / slice_anchors);
 * block_anchors 0 = the default, 1..64 otherwise.  GPCC_ERR_ARG outside the class (more than 8 stages, dh > 128, ch or dep_ch > 64, lags that
 * let a stage read what is not yet decoded); GPCC_ERR_FORMAT for a min / max no stream can have or counts beyond nbytes.  Bytes past a stream's
 * count read as zero and symbols stay inside the alphabet: a short or foreign file gives some finite values, never a fault. */
GPCC_API int gsac_decode_normal_chain(gpcc_ctx *ctx, const gsac_chain_stage *stages, int nstages, const float *ctx_dev, int ctx_pitch, int64_t n,
                                      int slice_anchors, int nslices, int block_anchors, void *stream);

/* GaussianModel.mlp_grid = nn.Sequential(Linear(din, dh), ReLU, Linear(dh, dout)) (src/gs_compress/HAC/scene/gaussian_model.py:258-262,
 * called through get_grid_mlp at :1152-1153 and :1281-1282): y = W2 relu(W1 x + b1) + b2 for n rows.
 * w1 (dh, din), w2 (dout, dh) row-major as nn.Linear stores them; all pointers device.  Specified fp32 order
 * (bias, then fmaf over k ascending), so the encoder and the decoder see the same context parameters. */
GPCC_API int gshac_mlp2(gpcc_ctx *ctx, const float *x_dev, const float *w1_dev, const float *b1_dev, const float *w2_dev, const float *b2_dev,
                        int64_t n, int din, int dh, int dout, float *y_dev, void *stream);
/* The same with the activation as an argument: act 0 = ReLU, 1 = LeakyReLU(slope) -- HAC++'s channel-context MLPs
 * (Channel_CTX_fea.MLP_d0..4: Linear(150 + 10 c, 40) - LeakyReLU - Linear(40, 30), HAC-plus/scene/gaussian_model.py:117-168, called through
 * get_deform_mlp.forward(feat, mean_scale, to_dec=c) at :1306 and :1490): context MLPs too -- encoder and decoder must obtain the same
 * bits, hence the same specified fp32 order.  TC-GS's mlp_triplane (Linear(603, 100) - ReLU - Linear(100, 175), called through get_tri_mlp at
 * TC-GS/scene/gaussian_model.py:1223 and :1386) and any layer with din <= 608, dh <= 100, dout <= 176 run on the matrix pipe as well, with the
 * weights read from L2 (W1 alone is larger than a CU's LDS): the same chains, the same bits. */
GPCC_API int gshac_mlp2_act(gpcc_ctx *ctx, const float *x_dev, const float *w1_dev, const float *b1_dev, const float *w2_dev, const float *b2_dev,
                            int64_t n, int din, int dh, int dout, int act, float slope, float *y_dev, void *stream);

/* _gridencoder.grid_encode_forward (inputs (N,D) in [0,1], embeddings (sO,F), offsets (L+1), resolutions (L),
 * outputs (L,N,F), ..., Rb, binary_vxl, min_level_id)   gridencoder.zip!gridencoder/src/gridencoder.h:12-22,
 * gridencoder.cu:100-361 (the inference forward: no dy_dx).  All device. */
GPCC_API int gsge_forward(gpcc_ctx *ctx, const float *inputs_dev, const float *embeddings_dev, const int32_t *offsets_dev,
                          const int32_t *resolutions_dev, float *outputs_dev, int64_t n, int num_dim, int n_features, int n_levels,
                          int rb, const uint8_t *binary_vxl_dev, const int32_t *min_level_id_dev, void *stream);

/* Device memory from the caller for the training paths (the grid encoder's backward workspace; the rasteriser's frame state, below):
 * alloc(alloc_user, bytes) returns a 256-byte aligned device pointer, or NULL (the call then fails with GPCC_ERR_NOMEM). */
typedef void *(*gsr_alloc_fn)(void *user, size_t bytes);

/* The training forward: gsge_forward's outputs (bit-identical) and, when dy_dx_dev is not NULL, dy_dx (N, L, D, F) with the
 * reference's formula (gridencoder.cu:363-657: edge differences times res - 2, border corners read as 0, no wn, no binary_vxl). */
GPCC_API int gsge_forward_train(gpcc_ctx *ctx, const float *inputs_dev, const float *embeddings_dev, const int32_t *offsets_dev,
                                const int32_t *resolutions_dev, float *outputs_dev, int64_t n, int num_dim, int n_features, int n_levels,
                                int rb, const uint8_t *binary_vxl_dev, const int32_t *min_level_id_dev, float *dy_dx_dev, void *stream);

/* _gridencoder.grid_encode_backward (gridencoder.cu:663-881): grad (L,N,F).  ADDS the embedding gradient into grad_embeddings
 * (n_rows, F) -- rows without contributions are untouched -- and OVERWRITES grad_inputs (N, D) when it is not NULL (dy_dx recomputed
 * from the inputs).  Bitwise reproducible: no float atomics (key pass, stable radix sort by table row, fixed-order sums).  Workspace
 * (about 28 bytes per (point, level, corner)) through `alloc`; enqueued on `stream` without synchronising. */
GPCC_API int gsge_backward(gpcc_ctx *ctx, const float *grad_dev, const float *inputs_dev, const float *embeddings_dev, const int32_t *offsets_dev,
                           const int32_t *resolutions_dev, int64_t n_rows, float *grad_embeddings_dev, float *grad_inputs_dev, int64_t n,
                           int num_dim, int n_features, int n_levels, int rb, const uint8_t *binary_vxl_dev, const int32_t *min_level_id_dev,
                           gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* ================= generate_neural_gaussians, inference path =================
 * src/gs_compress/HAC/gaussian_renderer/__init__.py:25-172 after attribute quantisation (:103-114, done by the caller):
 * view direction / distance (:116-118), optional feature bank (:121-132), opacity / colour / covariance MLPs on
 * [feat | view | dist] (:134-152), masking by neural opacity > 0 (:136-141, 160-162) and the assembly of position,
 * scale and rotation (:165-171).  n visible anchors, feat_dim in {32, 50}, K = n_offsets.
 * rows: the visible anchors as n ascending row indices into the model's tensors (the reference gathers `tensor[visible_mask]` five
 * times, :54-58 -- 0.8 GB of copies per million anchors; here the kernels read the rows in place), or NULL: the tensors hold exactly
 * the n anchors of the call.
 * mlp: 16 device pointers = {w1, b1, w2, b2} of mlp_feature_bank (all four NULL when use_feat_bank is off), mlp_opacity,
 * mlp_cov, mlp_color (nn.Linear layouts; gaussian_model.py:229-256).  mask (n, K) in {0, 1}; cam_center (3) device.
 * Outputs have room for n*K Gaussians; *count_out of them are written (anchor-major, the reference's order). */
GPCC_API int gsnn_generate(gpcc_ctx *ctx, int64_t n, const int32_t *rows, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
                           const float *scaling, const float *mask, const float *cam_center, const float *const *mlp, float *xyz_out,
                           float *color_out, float *opacity_out, float *scale_out, float *rot_out, int64_t *count_out, void *stream);

/* ================= generate_neural_gaussians, training path =================
 * The same Gaussians as gsnn_generate for the n anchors of the call (no row list: the caller gathers), plus what training needs:
 * nopa_out (n K) the neural opacity and keep_out (n K) bool.  mask (n, K) is used as given (HAC's straight-through value (b - s) + s is
 * only nearly {0, 1}).  mask_after_opacity = 0: HAC -- neural_opacity = tanh(z) * mask, keep = neural_opacity > 0, opacity = the kept
 * neural_opacity.  mask_after_opacity = 1: HAC++ -- neural_opacity = tanh(z), keep = tanh(z) > 0, and the mask multiplies the kept rows'
 * opacity and scaling.  The state the backward needs is the exclusive scan of keep, (n K + 1) uint32 in memory from `alloc` (one call),
 * returned in *pos_out and handed to gsnn_backward unchanged; other library calls may run in between.  Synchronises on the survivor count. */
GPCC_API int gsnn_forward_train(gpcc_ctx *ctx, int64_t n, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
                                const float *scaling, const float *mask, const float *cam_center, const float *const *mlp, int mask_after_opacity,
                                float *xyz_out, float *color_out, float *opacity_out, float *scale_out, float *rot_out, float *nopa_out, uint8_t *keep_out,
                                gsr_alloc_fn alloc, void *alloc_user, uint32_t **pos_out, int64_t *count_out, void *stream);
/* Gradients of a loss given the output gradients g_xyz (m, 3), g_color (m, 3), g_opacity (m), g_scale (m, 3), g_rot (m, 4) of the m kept
 * Gaussians and g_nopa (n K) of neural_opacity.  OVERWRITES d_anchor (n, 3), d_feat (n, F), d_offsets (n, K, 3), d_scaling (n, 6),
 * d_mask (n, K) and the 16 MLP gradients d_mlp (the layout of mlp; the bank's four are not written when mlp[0] is NULL).  The hidden
 * layers are recomputed; the weight gradients are fixed-order sums over fixed anchor ranges (no float atomics): bitwise reproducible.
 * alloc is called once for the workspace (about (4 F + 11 K + 10) floats per anchor, the bank's 2 F + 9 more), which the call no longer
 * needs once its kernels have run.  Enqueued on `stream` without synchronising. */
GPCC_API int gsnn_backward(gpcc_ctx *ctx, int64_t n, int feat_dim, int n_offsets, const float *anchor, const float *feat, const float *offsets,
                           const float *scaling, const float *mask, const float *cam_center, const float *const *mlp, int mask_after_opacity,
                           const uint32_t *pos, const float *g_xyz, const float *g_color, const float *g_opacity, const float *g_scale, const float *g_rot,
                           const float *g_nopa, float *d_anchor, float *d_feat, float *d_offsets, float *d_scaling, float *d_mask, float *const *d_mlp,
                           gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* The adaptive-step quantisation noise of the training branch (HAC-plus/gaussian_renderer/__init__.py:47-51, 64-69, 91-99) on nattr <= 3
 * row-aligned attributes of n rows in ONE launch: x[j], u[j], y[j] (n, widths[j]) float32 device, contiguous (any alignment of 4 bytes:
 * the vector width is chosen per attribute from the width and the addresses); u is the caller's U(-0.5, 0.5) draw; q0[j] the base step
 * (host, rounded to float32).  adj: the context MLP's output read in place -- adj[r adj_stride + adj_cols[j]] is row r's adjustment of
 * attribute j -- or NULL for the constant step q0[j] (adj_stride, adj_cols unused).  Per element, in float32 without contraction:
 *   Q_j[r] = q0_j * (1 + tanhf(adj[r, j]))  (q0_j without adj);  y_j[r, c] = x_j[r, c] + u_j[r, c] * Q_j[r];  q_out[r nattr + j] = Q_j[r]
 * gsnn_noise_backward (adj must not be NULL): g[j] (n, widths[j]) the upstream gradients of the y_j, grad_q (n, nattr) that of q_out (NULL: none);
 *   d_adj[r nattr + j] = ((S + grad_q[r nattr + j]) * q0_j) * fmaf(-t, t, 1),  t = tanhf(adj[r, j])  (= q0_j (1 - t^2) (S + grad_q)),
 *   S = sum_c g_j[r, c] * u_j[r, c] in this fixed order: with L = 4 lanes for widths[j] <= 8 and 16 otherwise, lane l adds the rounded
 *   products of the columns l, l + L, l + 2 L, ... in ascending order to 0.0f, then the L partial sums are added in a butterfly,
 *   s_l += s_(l xor d) for d = 1, 2, ..., L / 2.  No atomics: bitwise reproducible.  The gradient of x_j is g[j] itself: nothing is written for it.
 * n = 0 launches nothing.  n < 2^31, n widths[j] < 2^31.  x, u, y, g, widths, q0, adj_cols are host arrays.  Enqueued on `stream`, no synchronisation. */
GPCC_API int gsnn_noise_forward(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *x, const float *const *u, const int64_t *widths,
                                const double *q0, const float *adj, int64_t adj_stride, const int *adj_cols, float *const *y, float *q_out, void *stream);
GPCC_API int gsnn_noise_backward(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *g, const float *const *u, const int64_t *widths,
                                 const double *q0, const float *adj, int64_t adj_stride, const int *adj_cols, const float *grad_q, float *d_adj,
                                 void *stream);
/* The same with the step rule's base as an argument (host, rounded to float32): Q_j[r] = q0_j * (base + tanhf(adj[r, j])).  CAT-3DGS's rule
 * is base = 1.1 (CAT-3DGS/gaussian_renderer/__init__.py:65-67); the two calls above are these with base = 1 and give the same bits.  The base
 * shifts the step and leaves its slope alone: d_adj does not depend on it. */
GPCC_API int gsnn_noise_forward_b(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *x, const float *const *u, const int64_t *widths,
                                  const double *q0, const float *adj, int64_t adj_stride, const int *adj_cols, double base, float *const *y, float *q_out,
                                  void *stream);
GPCC_API int gsnn_noise_backward_b(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *g, const float *const *u, const int64_t *widths,
                                   const double *q0, const float *adj, int64_t adj_stride, const int *adj_cols, double base, const float *grad_q,
                                   float *d_adj, void *stream);
/* The evaluation side: STE_multistep's forward (utils/encodings.py:55-67) on the same nattr <= 3 row-aligned attributes in ONE launch.
 * x, widths, q0, adj, adj_stride, adj_cols, base, y, q_out as above; means: nattr float32 DEVICE scalars.  Per element, in float32, IEEE
 * division, no contraction, rintf (half to even, as torch.round):
 *   Q = q0_j * (base + tanhf(adj[r, j]));  v = use_clamp ? min(max(x, m_j - 15000 Q), m_j + 15000 Q) : x (a NaN x stays NaN);  y = rintf(v / Q) * Q
 * Q = 0 gives non-finite y, as the torch expression does.  No backward: every caller detaches.
 * gsnn_mean: means[j] = (float)(sum of x[j][0 .. counts[j]) / counts[j]) for nattr <= 3 tensors, the sum in double and in a fixed order
 * (256 workgroups per tensor, thread t of workgroup b adds elements b 256 + t, + 65536, ... ascending; a fixed tree over the 256 threads,
 * then over the 256 workgroups): bitwise reproducible, two launches.  partials: nattr * 256 doubles of device scratch. */
GPCC_API int gsnn_quantise(gpcc_ctx *ctx, int64_t n, int nattr, const float *const *x, const int64_t *widths, const double *q0, const float *adj,
                           int64_t adj_stride, const int *adj_cols, double base, const float *means, int use_clamp, float *const *y, float *q_out,
                           void *stream);
GPCC_API int gsnn_mean(gpcc_ctx *ctx, int nattr, const float *const *x, const int64_t *counts, double *partials, float *means, void *stream);

/* ================= Gaussian splat rasteriser, forward (a20) =================
 * diff_gaussian_rasterization (Scaffold-GS fork; zip missing from the reference tree).  Mirrors the C++ API the
 * reference's viewer calls: CudaRasterizer::Rasterizer::visible_filter / ::forward,
 * TC-GS/SIBR_viewers/src/projects/gaussianviewer/renderer/GaussianView.cpp:535-553, 660-688; Python call
 * sites HAC/gaussian_renderer/__init__.py:199-225, 268-303.  All pointers are device pointers; viewmatrix /
 * projmatrix are the 4x4 row-vector (transposed) matrices of HAC/scene/cameras.py:48-57; colours are
 * precomputed (shs = None in every call site); out_color is (3, H, W).  *num_rendered_out is the reference's count -- the tiles of every
 * splat's 3-sigma bounding square -- although the lists that are sorted and blended hold only the (splat, tile) pairs that can reach alpha >=
 * 1 / 255 somewhere in the tile (csrc/rasterizer.hip: tile_touches; the image is bit-identical either way). */
GPCC_API int gsr_visible_filter(gpcc_ctx *ctx, int P, int W, int H, const float *means3D, const float *scales, float scale_modifier,
                                const float *rotations, const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                                float tan_fovx, float tan_fovy, int prefiltered, int *radii, void *stream);
GPCC_API int gsr_forward(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                         const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                         const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy,
                         int prefiltered, float *out_color, int *radii, int64_t *num_rendered_out, void *stream);

/* ================= Rasteriser backward (training) =================
 * The training forward writes the image, radii and *num_rendered_out of gsr_forward (the image bit for bit) and keeps what the backward
 * needs in device memory the caller hands out: alloc(alloc_user, bytes) returns a device pointer (256-byte aligned) that stays valid until the
 * caller has run gsr_backward, or NULL (the call then fails with GPCC_ERR_NOMEM).  It is called twice per frame at most: once for the state
 * sized by P, the tiles and the pixels (per Gaussian: pixel centre, conic and opacity, depth order, pair offsets; per tile: list range and
 * dispatch order; per pixel: final transmittance and the list position after the last Gaussian blended into it), once, after the pair count L
 * is known, for the sorted pair list (12 L bytes).  Nothing of the frame lives in ctx's workspace, so other calls on ctx may run between the
 * forward and the backward.  state (host, GSR_STATE_WORDS words) receives the pair count, P, W, H and the device addresses of that state; it
 * is opaque to the caller and is handed back to gsr_backward unchanged.  Always the two-level sort; colours precomputed. */
#define GSR_STATE_WORDS 16
GPCC_API int gsr_forward_train(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                               const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                               const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy,
                               int prefiltered, float *out_color, int *radii, gsr_alloc_fn alloc, void *alloc_user, uint64_t *state,
                               int64_t *num_rendered_out, void *stream);
/* Gradients of a loss L given dL_dout = dL/d(out_color) (3, H, W) of the frame gsr_forward_train left in state; the forward's inputs and radii
 * are passed again, unchanged.  alloc is called once, for 36 L bytes of per-pair records that the call no longer needs when it returns (the
 * kernels are enqueued on `stream`; the call does not wait for them).  Outputs (P rows each, every row written): dL_dmeans3D (P, 3); dL_dmeans2D
 * (P, 3) = dL/d(NDC x, NDC y) of the projected centre and 0; dL_dcolors (P, 3); dL_dopacities (P); with scales + rotations dL_dscales (P, 3) and
 * dL_drotations (P, 4) (the quaternion as the forward uses it: unnormalised), with cov3D_precomp dL_dcov3D (P, 6) (an off-diagonal entry counts
 * both of its uses); the unused pair may be NULL.  Conventions of diff_gaussian_rasterization: the gradient passes through alpha's min(0.99, .)
 * as if it were not there, a view-space coordinate clamped at +-1.3 tan(fov) is a constant of the projection's Jacobian, the discrete decisions
 * (frustum, radius and tiles, the 1 / 255 and saturation tests) are not differentiated, Gaussians of radius 0 get 0.  No background gradient.
 * The sums have a fixed order: the result is bitwise reproducible. */
GPCC_API int gsr_backward(gpcc_ctx *ctx, const uint64_t *state, int P, const float *background, int W, int H, const float *means3D,
                          const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                          const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy,
                          const int *radii, const float *dL_dout, gsr_alloc_fn alloc, void *alloc_user, float *dL_dmeans3D, float *dL_dmeans2D,
                          float *dL_dcolors, float *dL_dopacities, float *dL_dscales, float *dL_drotations, float *dL_dcov3D, void *stream);

/* ================= Rasteriser depth and opacity maps =================
 * The three calls above with two more maps of the frame, (H, W) float32 each, either may be NULL: out_invdepth = sum_i w_i / tz_i over the
 * Gaussians a pixel blends (w_i = alpha_i T_i, the colour's own weights and blend rules; tz_i the view-space depth the frame sorts by; no
 * background term, not normalised -- the inverse-depth map of the public rasteriser's depth-regularisation release) and out_alpha = 1 - T_final,
 * the accumulated opacity (out_color = sum_i w_i c_i + (1 - out_alpha) background).  Pixels no Gaussian reaches hold 0 in both.
 * gsr_backward_aux takes dL_dinvdepth / dL_dalpha (NULL: zero; a non-NULL one needs a frame rendered with that map) and adds their part to
 * the same outputs: inverse depth is a fourth colour channel with background 0 whose per-Gaussian value 1 / tz sends its gradient to means3D
 * through the view matrix's third row; records are 40 L bytes then, and the result stays bitwise reproducible.  A training frame rendered
 * with a map keeps its per-Gaussian depths in the first block it asks `alloc` for (4 P bytes more) and notes the maps in state's last two
 * words.  With both NULL each call is its sibling above: the same kernels, the same bits. */
GPCC_API int gsr_forward_aux(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                             const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                             const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy,
                             int prefiltered, float *out_color, int *radii, float *out_invdepth, float *out_alpha, int64_t *num_rendered_out,
                             void *stream);
GPCC_API int gsr_forward_train_aux(gpcc_ctx *ctx, int P, const float *background, int W, int H, const float *means3D, const float *colors_precomp,
                                   const float *opacities, const float *scales, float scale_modifier, const float *rotations,
                                   const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx, float tan_fovy,
                                   int prefiltered, float *out_color, int *radii, float *out_invdepth, float *out_alpha, gsr_alloc_fn alloc,
                                   void *alloc_user, uint64_t *state, int64_t *num_rendered_out, void *stream);
GPCC_API int gsr_backward_aux(gpcc_ctx *ctx, const uint64_t *state, int P, const float *background, int W, int H, const float *means3D,
                              const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier,
                              const float *rotations, const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, float tan_fovx,
                              float tan_fovy, const int *radii, const float *dL_dout, const float *dL_dinvdepth, const float *dL_dalpha,
                              gsr_alloc_fn alloc, void *alloc_user, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors,
                              float *dL_dopacities, float *dL_dscales, float *dL_drotations, float *dL_dcov3D, void *stream);

/* ================= GausPcgc context network, training path (network_ue_4stage_conv.py:100-182 with gradients) =================
 * The frame is the encoder's teacher-forced layout: one octree (the FOG loop), a "prior set" of rows (levels 0..L-2 concatenated, base
 * level first, each level in Morton order) and a "target set" (levels 1..L-1), and ONE tile pool for the convolutions of both.  Rows of
 * features are (rows, 32) float32 in the library's PHYSICAL channel order (logical channel c sits at column 4 (c % 4) + c / 4 for c < 16,
 * 16 + 4 (c % 4) + (c - 16) / 4 above); weights and weight gradients use the upstream (K, Cin, Cout) layout in this library's offset
 * enumeration (gauspcc_amd.model.conv_offset_layout).  32 channels only; k = 3, 5 or 7.
 *
 * gpcc_train_frame: xyz (n, 3) int32 device, duplicate-free, any sign.  Everything a convolution or its backward needs is copied into ONE
 * block of caller memory (alloc is called once), so other calls on ctx may run between the forward and the backward; state (host,
 * GPCC_TRAIN_STATE_WORDS words) is opaque and stays valid while that block lives.  levels_out / level_nodes_out (24) as in gpcc_stats. */
#define GPCC_TRAIN_STATE_WORDS 256
GPCC_API int gpcc_train_frame(gpcc_ctx *ctx, const int32_t *xyz_dev, int64_t n, int kernel_size, gsr_alloc_fn alloc, void *alloc_user, uint64_t *state,
                              int32_t *levels_out, int64_t *level_nodes_out, void *stream);
/* The frame's nodes, all levels concatenated base first (Morton order inside a level, so the children of a node are contiguous and
 * octant-ascending): occ (nodes) uint8, coords (nodes, 3) int32; for the target set's rows parent (rows) int32 = the parent's row in the
 * prior set and octant (rows) uint8 = x%2 + 2 (y%2) + 4 (z%2).  Any pointer may be NULL. */
GPCC_API int gpcc_train_frame_nodes(gpcc_ctx *ctx, const uint64_t *state, uint8_t *occ_dev, int32_t *parent_dev, uint8_t *octant_dev, int32_t *coords_dev,
                                    void *stream);
/* w (K, 32, 32) device -> frag (K x 2048 floats) device, the layouts the convolution reads; mirror != 0 builds W'[o] = W[K-1-o]^T, the
 * weights of the input gradient.  channels != 32: GPCC_ERR_ARG. */
GPCC_API int gpcc_train_weights(gpcc_ctx *ctx, const float *w_dev, int channels, int kernel_size, int mirror, float *frag_dev, void *stream);
/* out = conv(in) (+ res) (ReLU if relu) over the rows of one set (0 = prior, 1 = target): the codec's convolution kernels, bit-identical to
 * gpcc_conv3d on the same coordinates.  With mirrored fragments and the (masked) output gradient as `in` this is the input gradient. */
GPCC_API int gpcc_train_conv(gpcc_ctx *ctx, const uint64_t *state, int set, const float *in_dev, const float *frag_dev, const float *res_dev, int relu,
                             float *out_dev, void *stream);
/* grad_w (K, 32, 32) = sum over the (output row i, neighbour row j) pairs of offset o of x[j]^T dy[i] (x, dy rows of the set, physical order).
 * OVERWRITES grad_w.  Fixed-order sums, no atomics: bitwise reproducible.  alloc is called once for K x groups x 4 KiB of partials
 * (groups <= ceil(8192 / K)), which the call no longer needs once its kernels have run (enqueued on `stream`, not waited for). */
GPCC_API int gpcc_train_wgrad(gpcc_ctx *ctx, const uint64_t *state, int set, const float *x_dev, const float *dy_dev, gsr_alloc_fn alloc, void *alloc_user,
                              float *grad_w_dev, void *stream);

/* ================= Exact k-nearest neighbours (training initialisation) =================
 * simple_knn._C.distCUDA2(points) (simple-knn.zip!simple-knn/spatial.cu:16-23, simple_knn.cu:185-219: k = 3, the mean) and sklearn's
 * NearestNeighbors(K).kneighbors(X) on its fit data (TC-GS/scene/gaussian_model.py:1052-1059: k = K - 1 plus the point itself).
 * xyz (n, 3) float32 device, 0 <= n < 2^31, 1 <= k <= 16.  With d(i, j) = (dx*dx + dy*dy) + dz*dz, dx = x_j - x_i, in float32 without
 * contraction: L_i = the k smallest pairs (d(i, j), j) over j != i in lexicographic order (distance, then index), pairs with d > FLT_MAX
 * (overflow) left out, padded with (FLT_MAX, -1).  Outputs, each may be NULL: idx_out (n, k) int64 and dist2_out (n, k) float32 = L_i,
 * mean_out (n) = the sequential float32 sum of L_i's distances / (float)k (for k = 3 simple_knn's value, its P <= 3 sentinels included).
 * A NaN or infinite coordinate: GPCC_ERR_ARG, nothing written.  The cost is below quadratic on every input (a Morton-sorted 64-ary tree of
 * boxes, csrc/knn.hip), 1M identical points included.  alloc is called once, for at most 26 n + 65536 bytes that the call no longer needs
 * once its kernels have run; ctx's workspace arena holds nothing that grows with n.  Enqueued on `stream`; the only synchronisation is the
 * read-back of the non-finite flag. */
GPCC_API int gpcc_knn(gpcc_ctx *ctx, const float *xyz_dev, int64_t n, int k, int64_t *idx_out, float *dist2_out, float *mean_out,
                     gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* ================= Anchor growing (training densification, HAC/scene/gaussian_model.py:823-911) =================
 * torch_scatter.scatter_max in row form: src (m, c) float32, index (m) int64 in [0, dim_size); out, arg (dim_size, c).  For slot s and
 * column c over G = {j : index[j] = s}: out = the maximum over G (and over out's initial value when include_self), a NaN in G making it
 * NaN; arg = the smallest j in G with src[j, c] == out (with a NaN out: the smallest j holding a NaN), or m if there is none; out's bits
 * are src[arg, c]'s when arg < m.  Without include_self this is torch_scatter's own output: initialised to -FLT_MAX, maximised, and then
 * every value still equal to -FLT_MAX set to 0 (masked_fill(out == lowest, 0)): an empty slot gives (0, m), a group whose maximum is
 * -FLT_MAX gives (0, its smallest such j), a group of -inf only gives (0, m).  torch_scatter's tie rule depends on the order of atomics;
 * this one does not, and no float atomics are used.  An index outside [0, dim_size): GPCC_ERR_ARG, nothing written (the call's only
 * synchronisation reads that flag back).  alloc is called once, for at most 24 m + 8 dim_size c bytes plus the sort's digit table and
 * 256 bytes, that the call no longer needs once its kernels have run.  m < 2^31.  Enqueued on `stream`. */
GPCC_API int gpcc_scatter_max(gpcc_ctx *ctx, const float *src_dev, const int64_t *index_dev, int64_t m, int64_t c, int64_t dim_size,
                              int include_self, float *out_dev, int64_t *arg_dev, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* One grid level of anchor_growing.  Candidates xyz (m, 3) float32 with feature rows rows (m) int64 into feats (nrows, c) float32 (rows
 * NULL: row j is candidate j); existing anchors (n, 3) float32.  Voxel g = (int32)rint(x * inv) per axis (one rounded float32 product,
 * round half to even: torch's `round(x / size).int()` on the GPU, whose division by a CPU scalar multiplies by inv = 1.0f / size).
 * A non-finite coordinate or one outside int32 after rounding (candidates or anchors), or a row outside [0, nrows): GPCC_ERR_ARG with
 * nothing written.  Result: the U unique candidate voxels that hold no anchor voxel, in lexicographic signed (x, y, z) order (that of
 * torch.unique(dim=0)); anchors (U, 3) = (float)g * size; features (U, c) = scatter_max over each voxel's candidates of feats[rows[j]]
 * without include_self (the rule above, -FLT_MAX masked to 0).  *count_out = U.  Two synchronisations: the read-back of the
 * candidates' box and the invalid-input flag, and that of U.  alloc is called (1) once for the workspace, at most 84 m + 56 n bytes plus
 * the sort's digit table and 1 KiB, then, only when U > 0, (2) for the outputs, anchors at offset 0 and features at offset
 * (12 U + 255) & ~255, and (3) for 8 U c bytes of per-column maxima.  (1) and (3) are not needed once the kernels have run.  When the
 * candidates' voxels span less than 2^21 per axis one packed key is sorted; otherwise two sorts (z, then x and y) handle any int32
 * voxel.  m, n < 2^31; enqueued on `stream`. */
GPCC_API int gpcc_grow_voxels(gpcc_ctx *ctx, const float *xyz_dev, int64_t m, const int64_t *rows_dev, const float *feats_dev, int64_t nrows,
                              int64_t c, const float *anchors_dev, int64_t n, float inv, float size, int64_t *count_out, gsr_alloc_fn alloc,
                              void *alloc_user, void *stream);

/* ================= Densification statistics (HAC/scene/gaussian_model.py:758-775 training_statis, :914-968 adjust_anchor) =================
 * One iteration of training_statis, in place, enqueued on `stream` with NO host synchronisation.  n anchors of k offsets; visible (n) bytes
 * or NULL (all; then v must equal n); opacity (v k) float32, the neural opacity of the v visible anchors in order; selection (v k) bytes;
 * update_filter (s) bytes; grad (s rows of grad_stride >= 2 floats, columns 0 and 1 read); the accumulators opacity_accum, anchor_demon (n)
 * and offset_gradient_accum, offset_denom (n k) float32.  With v(a) = the visible anchors before a and s(j) = the set selection entries
 * before j, for every visible a, in float32 without contraction:
 *   opacity_accum[a] += ((0.0f + c_0) + c_1) + ... + c_{k-1},  c_i = o_i < 0 ? 0 : o_i,  o_i = opacity[v(a) k + i]  (a NaN stays one)
 *   anchor_demon[a] += 1
 *   for every i with selection[j] set, j = v(a) k + i, and update_filter[s(j)] set, g = grad row s(j):
 *     offset_gradient_accum[a k + i] += sqrtf(g[0] g[0] + g[1] g[1])  (each product, the sum and the root rounded once),  offset_denom[a k + i] += 1
 * Every destination has one source: no atomics, bitwise reproducible.  The host knows v and s from shapes only.  When count(visible) != v
 * or count(selection) != s the update writes NOTHING to the accumulators and forms no index from a rank (the scans are complete before it
 * starts and it compares their totals first); it sets err[0] |= 1 (visible) | 2 (selection) and err[1..4] = count(visible), v,
 * count(selection), s.  err: 8 uint32 words of device memory owned by the caller, zero before the first call; the caller reads them at its
 * next synchronisation.  alloc is called once, for 8 (max(n, v) + 1) bytes plus 512 that the call no longer needs once its kernels have
 * run.  n, v < 2^28, k <= 256, n k and v k < 2^31. */
GPCC_API int gpcc_densify_stats(gpcc_ctx *ctx, int64_t n, int k, const uint8_t *visible_dev, const float *opacity_dev, int64_t v,
                                const uint8_t *selection_dev, const uint8_t *update_filter_dev, int64_t s, const float *grad_dev, int64_t grad_stride,
                                float *opacity_accum_dev, float *anchor_demon_dev, float *offset_gradient_accum_dev, float *offset_denom_dev,
                                uint32_t *err_dev, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* The head of adjust_anchor over total = n0 k entries: g = offset_gradient_accum / offset_denom in float32 (correctly rounded),
 * grads_norm = g != g ? 0 : fabsf(g) (0/0 and every other NaN give 0), offset_mask = offset_denom > offset_thr (bytes 0 / 1).  One launch,
 * no synchronisation. */
GPCC_API int gpcc_densify_front(gpcc_ctx *ctx, const float *offset_gradient_accum_dev, const float *offset_denom_dev, int64_t total, float offset_thr,
                                float *grads_norm_out_dev, uint8_t *offset_mask_out_dev, void *stream);

/* The tail of adjust_anchor, after the framework's anchor_growing has grown opacity_accum and anchor_demon from n0 to n1 >= n0 rows.
 * anchors_mask[a] = anchor_demon[a] > anchor_thr; prune[a] = opacity_accum[a] < min_opacity * anchor_demon[a] (one rounded float32
 * product) && anchors_mask[a], written to prune_out (n1 bytes).  *count_out = n2 = n1 - count(prune).  For the survivors, in order:
 * offset_gradient_accum and offset_denom rows (k each) with the entries of a set offset_mask (n0 k bytes) zeroed and rows of anchors
 * >= n0 zero; opacity_accum and anchor_demon, zero where anchors_mask is set.  alloc is called (1) once for 4 (n1 + 1) bytes of ranks, not
 * needed once the kernels have run, then, only when n2 > 0, (2)-(5) for offset_gradient_accum (n2 k), offset_denom (n2 k), opacity_accum
 * (n2), anchor_demon (n2) floats.  One scan, one gather pass, one synchronisation (the read-back of n2).  n1 < 2^28, n1 k < 2^31. */
GPCC_API int gpcc_densify_finish(gpcc_ctx *ctx, const float *offset_gradient_accum_dev, const float *offset_denom_dev, const uint8_t *offset_mask_dev,
                                 int64_t n0, int k, const float *opacity_accum_dev, const float *anchor_demon_dev, int64_t n1, float anchor_thr,
                                 float min_opacity, uint8_t *prune_out_dev, int64_t *count_out, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* Row compaction of nmats <= 32 float32 matrices of n rows: src[t] (n, widths[t]) device, keep (n) bytes.  *count_out = n2 = count(keep);
 * alloc is called (1) once for 4 (n + 1) bytes of ranks, then, only when n2 > 0, once per matrix in order for its n2 widths[t] floats:
 * the kept rows in order.  One scan, one launch over all matrices, one synchronisation (the read-back of n2).  n < 2^28,
 * n widths[t] < 2^31.  src and widths are host arrays. */
GPCC_API int gpcc_compact_rows(gpcc_ctx *ctx, const uint8_t *keep_dev, int64_t n, int nmats, const float *const *src, const int64_t *widths,
                               int64_t *count_out, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* The transpose of gpcc_compact_rows (the backward of t[keep]): src[t] (m, widths[t]) device, the rows of the kept set in order; dst[t]
 * (n, widths[t]) device receives row i of src[t] at the position of the i-th set entry of keep (n bytes) and zero rows elsewhere.  The
 * caller knows m = count(keep) from the forward: NO synchronisation.  Should keep count more than m entries, those beyond the m-th get
 * zero rows and nothing outside src is read.  alloc is called once, only when m > 0, for 4 (n + 1) bytes of ranks, not needed once the
 * kernels have run.  One scan (none when m = 0), one launch over all matrices.  nmats <= 32, 0 <= m <= n < 2^28, n widths[t] < 2^31.
 * src, widths and dst are host arrays. */
GPCC_API int gpcc_expand_rows(gpcc_ctx *ctx, const uint8_t *keep_dev, int64_t n, int64_t m, int nmats, const float *const *src, const int64_t *widths,
                              float *const *dst, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* ================= Photometric loss (training step, HAC/utils/loss_utils.py: ssim, l1_loss; train.py's loss) =================
 * img1, img2 (batch, channels, height, width) float32 device, contiguous.  SSIM of every plane with the reference's window: the outer
 * product of taps (window_size float32 HOST values: the caller builds them as the reference does, Gaussian taps of sigma 1.5 normalised
 * by torch's float32 sum -- in flat bright regions sigma^2 = E - mu^2 turns an ulp of that sum into a visible bias), zero padding
 * window_size / 2; window_size odd in [1, 31] (GPCC_ERR_ARG otherwise: an even window gives the reference an (H+1) x (W+1) map).  Per pixel, in float32 with sigma^2 = E - mu^2:
 * S = (2 mu1 mu2 + C1)(2 sigma12 + C2) / ((mu1^2 + mu2^2 + C1)(sigma1^2 + sigma2^2 + C2)), C1 = 0.01^2, C2 = 0.03^2.
 * gsr_ssim_forward: ssim_out[0] = the mean of S (size_average) or ssim_out[b] = the mean over item b (batch values).  With size_average,
 * l1_out (may be NULL) = mean |img1 - img2| and loss_out (may be NULL; needs l1_out) = (float)(1 - lambda_dssim) l1 + (float)lambda_dssim (1 - ssim) in float32.
 * Sums are per-tile doubles added in a fixed order (no atomics): bitwise reproducible.  nmaps = 0: nothing else is written; 3 or 4:
 * maps (nmaps, batch, channels, height, width) receives dS/dmu1, dS/dE[x^2] (= dS/dE[y^2]), dS/dE[xy] and, for nmaps = 4, dS/dmu2, what
 * gsr_ssim_backward reads.  alloc is called once for 16 bytes per 32 x 32 tile of every plane, not needed once the kernels have run.
 * gsr_ssim_backward: the same images, window, taps and maps; the upstream gradients are device values: grad_ssim (1 value, or batch values
 * without size_average) and grad_l1 (1 value, or NULL: no L1 term).  dL/dS(p) = ssim_scale grad_ssim[b] / n, dL/d|x - y|(p) = l1_scale
 * grad_l1[0] / N (n = the pixels the mean of item b runs over, N = all).  Writes grad_img1 (needs nmaps >= 3) and grad_img2 (needs nmaps = 4),
 * each may be NULL; sign(0) = 0.  Both calls are enqueued on `stream` without synchronising. */
GPCC_API int gsr_ssim_forward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t batch, int64_t channels, int64_t height, int64_t width,
                              int window_size, const float *taps, int size_average, float *ssim_out, float *l1_out, float *loss_out, double lambda_dssim,
                              float *maps, int nmaps, gsr_alloc_fn alloc, void *alloc_user, void *stream);
GPCC_API int gsr_ssim_backward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t batch, int64_t channels, int64_t height, int64_t width,
                               int window_size, const float *taps, int size_average, const float *maps, int nmaps, const float *grad_ssim, float ssim_scale,
                               const float *grad_l1, float l1_scale, float *grad_img1, float *grad_img2, void *stream);

/* ================= Wavelet loss (training step, TC-GS/utils/loss_utils.py:66-83: wavelet_loss; its DWTForward / DWTInverse of
 * pytorch_wavelets with wave 'haar', mode 'zero') =================
 * One level of the transform, float32 with every product rounded on its own, s = (float)0.7071067811865476, a plane read as zero outside:
 * on the quad a b / c d = x[2r..2r+1][2k..2k+1] the row pass gives lo0 = a s + b s, hi0 = a s - b s, lo1 = c s + d s, hi1 = c s - d s and
 * the column pass LL[r][k] = lo0 s + lo1 s, band0 = lo0 s - lo1 s (low along width, high along height), band1 = hi0 s + hi1 s, band2 =
 * hi0 s - hi1 s; all bands are ceil(H / 2) x ceil(W / 2).  The next level transforms LL.
 * gsr_wavelet_l1_forward: img1, img2 (planes, height, width) float32 device, contiguous.  Two levels of both images in one pass over
 * 4 x 4 pixel blocks; seven band means of |coefficient of img1 - coefficient of img2| in the order LL2, level-1 bands 0..2, level-2
 * bands 0..2 (level 1: planes h1 w1 values each, h1 = ceil(height / 2); LL2 and level 2: planes h2 w2, h2 = ceil(h1 / 2)); bands_out (7
 * values, may be NULL) receives them, loss_out (1 value) = (float) sum_b weights[b] mean_b over the bands with weights[b] != 0 (weights: 7
 * HOST doubles).  Sums are per-workgroup doubles added in a fixed order (no atomics): bitwise reproducible.  alloc is called once for 56
 * bytes per 256 blocks, not needed once the kernels have run.
 * gsr_wavelet_l1_backward: the same images and weights, grad_loss one device value; recomputes the coefficients (nothing is saved) and
 * writes d loss / d img1 to grad_img1 and its negative, bit for bit, to grad_img2 (either may be NULL); sign(0) = 0.
 * gsr_haar_forward: x (planes, height, width) to ll_out (planes, h, w) and high_out (planes, 3, h, w), h = ceil(height / 2), w alike.
 * gsr_haar_inverse: ll (planes, h, w) and high (planes, 3, h, w; NULL = zeros) to out (planes, out_height, out_width), out_height in
 * {2h - 1, 2h} and out_width alike (the padded row / column is cropped).  Haar is orthonormal: each of the two is the other's adjoint,
 * so each is the other's backward.  All four calls are enqueued on `stream` without synchronising. */
GPCC_API int gsr_wavelet_l1_forward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t planes, int64_t height, int64_t width,
                                    const double *weights, float *loss_out, float *bands_out, gsr_alloc_fn alloc, void *alloc_user, void *stream);
GPCC_API int gsr_wavelet_l1_backward(gpcc_ctx *ctx, const float *img1, const float *img2, int64_t planes, int64_t height, int64_t width,
                                     const double *weights, const float *grad_loss, float *grad_img1, float *grad_img2, void *stream);
GPCC_API int gsr_haar_forward(gpcc_ctx *ctx, const float *x, int64_t planes, int64_t height, int64_t width, float *ll_out, float *high_out, void *stream);
GPCC_API int gsr_haar_inverse(gpcc_ctx *ctx, const float *ll, const float *high, int64_t planes, int64_t h, int64_t w, float *out, int64_t out_height,
                              int64_t out_width, void *stream);

/* ================= Spherical-harmonic colours (the rasteriser's shs= argument: diff_gaussian_rasterization's computeColorFromSH, forward
 * and backward; utils/sh_utils.py: eval_sh) =================
 * sh: P rows of coefficients, float32 device; entry (k, c) of row i is sh[i row_stride + k coef_stride + c chan_stride] (strides in
 * floats): (P, M, 3) contiguous is (3, 1, 3 M), eval_sh's (P, 3, M) is (1, M, 3 M); M may exceed the K = (degree + 1)^2 active ones, degree
 * 0..4.  Exactly one of means3D and dirs (each (P, 3) contiguous) is given:
 *   means3D with campos (3 floats on the DEVICE, read there): v = mean - campos, l2 = (v_x v_x + v_y v_y) + v_z v_z, len = sqrt(l2),
 *     d = v / len, or d = 0 when l2 == 0 (a Gaussian at the camera centre keeps its DC term); colour_c = max(value_c + 0.5, 0) and
 *     clamped (P, 3) uint8 = (value_c + 0.5 < 0): equality is not clamped;
 *   dirs: d as given, not renormalised; colour_c = value_c, clamped is not touched (may be NULL).
 * Arithmetic contract: float32, every step one IEEE operation (no fused multiply-add; sqrt and division correctly rounded), in this order.
 * With x, y, z = d: xx = x x, yy, zz, xy = x y, yz = y z, xz = x z, xmy = xx - yy, p = 3 xx - yy, q = (4 zz - xx) - yy,
 * r = (2 zz - 3 xx) - 3 yy, s = xx - 3 yy, xyz = xy z, u = 7 zz - 1, v = 7 zz - 3; each basis value is one constant (a double rounded to
 * float32, sign included) times one polynomial:
 *   b0 = C0;  b1 = -C1 y, b2 = C1 z, b3 = -C1 x;
 *   b4 = C2a xy, b5 = -C2a yz, b6 = C2c ((2 zz - xx) - yy), b7 = -C2a xz, b8 = C2e xmy;
 *   b9 = -C3a (y p), b10 = C3b xyz, b11 = -C3c (y q), b12 = C3d (z r), b13 = -C3c (x q), b14 = C3f (z xmy), b15 = -C3a (x s);
 *   b16 = C4a (xy xmy), b17 = -C4b (yz p), b18 = C4c (xy u), b19 = -C4d (yz v), b20 = C4e (zz (35 zz - 30) + 3), b21 = -C4d (xz v),
 *   b22 = C4g (xmy u), b23 = -C4b (xz s), b24 = C4i (xx s - yy p)           (degree 4 is the r = 1 form, as eval_sh's)
 *   C0 = 1/2 sqrt(1/pi), C1 = sqrt(3/(4 pi)), C2a = 1/2 sqrt(15/pi), C2c = 1/4 sqrt(5/pi), C2e = 1/4 sqrt(15/pi), C3a = 1/4 sqrt(35/(2 pi)),
 *   C3b = 1/2 sqrt(105/pi), C3c = 1/4 sqrt(21/(2 pi)), C3d = 1/4 sqrt(7/pi), C3f = 1/4 sqrt(105/pi), C4a = 3/4 sqrt(35/pi),
 *   C4b = 3/4 sqrt(35/(2 pi)), C4c = 3/4 sqrt(5/pi), C4d = 3/4 sqrt(5/(2 pi)), C4e = 3/16 sqrt(1/pi), C4g = 3/8 sqrt(5/pi), C4i = 3/16 sqrt(35/pi).
 *   value_c = (..((b0 sh[0][c]) + b1 sh[1][c]) + ...) + b_{K-1} sh[K-1][c].
 * gsr_sh_backward: the same inputs, M, clamped as the forward wrote it and dL_dcolors (P, 3).  g_c = 0 where clamped, dL_dcolors_c
 * otherwise.  dL_dsh (entry (k, c) of row i at i grad_row_stride + k grad_coef_stride + c grad_chan_stride; every one of the P M 3
 * entries is written) = b_k g_c for k < K, and exactly 0 for k >= K and for clamped channels.  dL/dd_a = the sum over k = 1 .. K-1,
 * ascending and starting with its first term, of (d b_k / d d_a) t_k, t_k = (sh[k][0] g_0 + sh[k][1] g_1) + sh[k][2] g_2, leaving out the
 * terms whose derivative is identically zero; the derivatives are again constant times polynomial, spelled out in csrc/sh.hip
 * (sh_dir_grad) and restated in tests/sh_ref.py.  dirs: dL_ddirs (P, 3) = dL/dd.  means3D: dot = (dL/dd_x d_x + dL/dd_y d_y) + dL/dd_z d_z,
 * dL_dmeans3D_a = (dL/dd_a - d_a dot) / len, and exactly 0 when l2 == 0.  Degree 0: both are exactly 0.  No gradient for campos.  dL_dsh, dL_dmeans3D / dL_ddirs may each be NULL (not
 * computed).  NaN in a Gaussian's inputs gives NaN in that Gaussian's outputs only.  Each output element has one owner: no atomics, no
 * reductions, bitwise reproducible; the memory path taken (rows staged through LDS or read directly, by stride and alignment) changes no
 * value.  Both calls are enqueued on `stream` without synchronising; P = 0 is a no-op. */
GPCC_API int gsr_sh_forward(gpcc_ctx *ctx, int P, int degree, const float *sh, int64_t coef_stride, int64_t chan_stride, int64_t row_stride,
                            const float *means3D, const float *campos, const float *dirs, float *colors, uint8_t *clamped, void *stream);
GPCC_API int gsr_sh_backward(gpcc_ctx *ctx, int P, int degree, int M, const float *sh, int64_t coef_stride, int64_t chan_stride, int64_t row_stride,
                             const float *means3D, const float *campos, const float *dirs, const uint8_t *clamped, const float *dL_dcolors,
                             float *dL_dsh, int64_t grad_coef_stride, int64_t grad_chan_stride, int64_t grad_row_stride, float *dL_dmeans3D,
                             float *dL_ddirs, void *stream);

/* ================= Entropy rate models (training step, HAC-plus/utils/entropy_models.py: Entropy_gaussian, Entropy_gaussian_mix_prob_2 / _3,
 * Low_bound; the same Gaussian model as gsac_calculate_cdf) =================
 * x (n, c) float32 device, contiguous; k in {1, 2, 3} mixture components.  mean[i], scale[i] (and prob[i] for k > 1) are device pointers,
 * kinds[3k] their shapes in the order mean_0..k-1, scale_0..k-1, prob_0..k-1 (kinds[2k..] unused for k = 1): 0 = full (n, c) contiguous,
 * 1 = per row (n), 2 = one value.  Q likewise (q_kind 0, 1, 2, q a device pointer) or 3 = the host value q_host (q unused).  x_mean is one
 * float32 device value (read on the device, never copied back).  Per element, in float32 and in the reference's expression order:
 *   Q = max(Q, q_floor) when q_floor > 0 (CAT-3DGS: 1e-9); lo = x_mean - 15000 Q, hi = x_mean + 15000 Q; x' = clamp(x, lo, hi)
 *   s_i = max(scale_i, 1e-9); Phi_i(v) = 0.5 (1 + erf((v - mean_i) (1 / s_i) / sqrt 2)) (torch's Normal.cdf, the 1 + erf form)
 *   L = |Phi_0(x' + Q/2) - Phi_0(x' - Q/2)| (k = 1) or sum_i prob_i |Phi_i(x' + Q/2) - Phi_i(x' - Q/2)| (list order)
 *   L' = max(L, 1e-6); out = L' (return_lkl) or -log2(L')
 * gsac_rate_forward writes out (n, c).  gsac_rate_backward takes the upstream gradient grad_out (n, c) and writes any of grad_x (n, c),
 * grad_mean[i], grad_scale[i], grad_prob[i], grad_q, each shaped as its operand (n, c) / (n) / (1), NULL = not wanted (the arrays
 * themselves may be NULL); a host Q has no gradient.  Analytic gradients with autograd's choices at the kinks: clamp passes where
 * lo <= x <= hi, where scale_i >= 1e-9 and where Q >= q_floor; |.| has gradient 0 at 0; Low_bound passes iff L >= 1e-6; the clamp
 * bounds are detached (x_mean gets no gradient, Q enters through x' +- Q/2 only).  Per-row and one-value gradients are summed in a fixed
 * order (per row: columns in order; one value: rows in order per workgroup in double, then the workgroup partials in a fixed tree), no
 * atomics: bitwise reproducible.  alloc is called once, only when a one-value gradient is wanted, for 8 bytes per workgroup of
 * ceil(n / floor(256 / c)) per such gradient, not needed once the kernels have run.  n = 0 launches nothing (one-value gradients are set
 * to 0).  Both calls are enqueued on `stream` without synchronising.  Non-finite mean or scale is not rejected. */
GPCC_API int gsac_rate_forward(gpcc_ctx *ctx, int k, int64_t n, int64_t c, const float *x, const float *x_mean, const float *const *mean,
                               const float *const *scale, const float *const *prob, const int *kinds, const float *q, int q_kind, double q_host,
                               double q_floor, int return_lkl, float *out, void *stream);
GPCC_API int gsac_rate_backward(gpcc_ctx *ctx, int k, int64_t n, int64_t c, const float *x, const float *x_mean, const float *const *mean,
                                const float *const *scale, const float *const *prob, const int *kinds, const float *q, int q_kind, double q_host,
                                double q_floor, int return_lkl, const float *grad_out, float *grad_x, float *const *grad_mean,
                                float *const *grad_scale, float *const *grad_prob, float *grad_q, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* The rate term of CAT-3DGS's channel-wise context chain in training (CAT-3DGS/gaussian_renderer/__init__.py:92-123): the feat groups, then
 * scaling, then offsets, each stage under mean = ctx + dmean, scale = ctx + dscale with (dmean | dscale) the stage MLP's output.  In training
 * the channels an MLP reads are the noisy feat itself, so with the MLPs' outputs in hand every stage is priced in ONE launch and
 * differentiated in one.  One record per stage (at most 8; together they price every column of the three attributes exactly once and no ctx
 * column is read by two of them): */
typedef struct {
    int32_t attr;                  /* 0 feat, 1 scaling, 2 offsets */
    int32_t col;                   /* the stage prices the attribute's columns [col, col + ch) */
    int32_t ch;                    /* 1..64 */
    int32_t mean_col, scale_col;   /* first columns of the stage's base mean / scale in a row of ctx (CAT-3DGS: scales come first) */
    const float *res;              /* device (m, 2 ch) contiguous, the stage MLP's output read in place: dmean = res[:, :ch], dscale = res[:, ch:]; NULL: none */
} gsac_rate_stage;
/* All tensors float32 device: ctx (m, ctx_width) with ctx_stride floats between rows, read in place; feat (m, F), scaling (m, 6),
 * offsets (m, 3 K) contiguous; q (m, 3) the per-row steps of the three attributes (gsnn_noise_forward's q_out); x_mean[3] the three clamp
 * centres, read on the device; mask (m, K) the offsets mask or NULL.  Per element of stage s, in float32 without contraction:
 *   mean = ctx[r, mean_col + j] + res[r, j], scale = ctx[r, scale_col + j] + res[r, ch + j] (one rounded add each; the operand itself
 *   without res); then gsac_rate_forward's element with k = 1, Q = q[r, attr], x_mean[attr] and q_floor; offsets bits are multiplied by
 *   mask[r, c / 3].  bits (m, F + 6 + 3 K), columns [feat | scaling | offsets].
 * gsac_chain_rate_backward takes grad_bits (m, F + 6 + 3 K) and writes any of (NULL = not wanted): d_feat, d_scaling, d_offsets (shaped as the
 * inputs); d_ctx (m, ctx_width) contiguous, EVERY column written -- a stage's mean and scale columns its gradients, columns no stage reads
 * (the three step adjustments) 0; d_res[s] (m, 2 ch) the same values as the stage's d_ctx columns (d_res or an entry NULL: not wanted);
 * d_q (m, 3); d_mask (m, K) = sum over the three columns of grad_bits * the unmasked bits.  Gates are gsac_rate_backward's, the scale gate on
 * the sum scale + dscale >= 1e-9.  d_q and d_mask are added by one owner with columns ascending, no atomics: bitwise reproducible.
 * F + 6 + 3 K <= 512, ctx_width <= 1088.  m = 0 launches nothing.  stages, d_res are host arrays.  Enqueued on `stream`, no synchronisation. */
GPCC_API int gsac_chain_rate_forward(gpcc_ctx *ctx, int64_t m, int feat_dim, int n_offsets, const float *ctx_dev, int64_t ctx_stride, int ctx_width,
                                     const float *feat, const float *scaling, const float *offsets, const float *q, const float *x_mean, double q_floor,
                                     const float *mask, const gsac_rate_stage *stages, int nstages, float *bits, void *stream);
GPCC_API int gsac_chain_rate_backward(gpcc_ctx *ctx, int64_t m, int feat_dim, int n_offsets, const float *ctx_dev, int64_t ctx_stride, int ctx_width,
                                      const float *feat, const float *scaling, const float *offsets, const float *q, const float *x_mean, double q_floor,
                                      const float *mask, const gsac_rate_stage *stages, int nstages, const float *grad_bits, float *d_feat,
                                      float *d_scaling, float *d_offsets, float *d_ctx, float *const *d_res, float *d_q, float *d_mask, void *stream);

/* ================= Tri-plane context sampler (TC-GS/utils/triplane.py: sample_from_planes :87-164, Triplane.sample :226-238) =================
 * planes (3, C, H, W), max_coords, min_coords (3), all float32 device; radii and box_warp = 1 as Triplane passes them (radii = 0.5 *
 * spatial_lr_scale).  coordinates: (n, k, 3) with repeat = 0, or (n, 3) with repeat = 1: every anchor's one sample is written k times
 * (the reference's anchor.unsqueeze(1).repeat(1, K, 1) call sites), bit-identical to the materialised form.  out (n, k * 3 * C):
 * out[n, (k_i * 3 + p) * C + ch], the reference's (N, K, 3, C) result.  Per plane p, in float32 and the reference's expression order:
 *   mag_sq[p] = min(min(|proj_p(max)|^2, |proj_p(min)|^2), radii^2), proj_0(b) = (b.x, b.y), proj_1(b) = (b.x, b.z), proj_2(b) = (b.z, b.x)
 *   c = 2 coordinate; u_0 = (c.y, c.z), u_1 = (c.x, c.z), u_2 = (c.x, c.y); v = u / sqrt(mag_sq[p]) * 2 - 1; x = 6 v
 *   m = max(|x|^2, FLT_EPSILON); z = x if m <= 1 else ((2 sqrt(m) - 1) / m) x; g = z / 2
 *   bilinear grid_sample of planes[p] at g (padding zeros, align_corners false): pixel = ((g + 1) size - 1) / 2, g[0] along W, g[1] along H
 * A sample whose pixel coordinate is not finite gives zeros and no gradient (torch would index with it); no index is formed from it.
 * Limits: C in [1, 256], H and W in [2, 4096], k >= 1 (k <= 64 with repeat), n * k * 12 < 2^32; a violation returns GPCC_ERR_ARG before
 * any launch.  n = 0 launches nothing (the backward zeroes grad_planes).
 * gsge_plane_backward: grad_out (n, k * 3 * C).  OVERWRITES grad_planes (3, C, H, W) and, when it is not NULL, grad_coordinates (shaped
 * as coordinates; through the bilinear weights, both branches of the contraction and the scaling; the repeat form's is the sum over its
 * k copies).  No gradient for the bounds or radii.  Bitwise reproducible: no float atomics (one (texel, slot) key per (sample, plane,
 * corner), stable radix sort, fixed-order sums; the repeat form adds its k gradient copies in k order first).
 * Workspace through `alloc`: forward 3 C H W floats; backward about 28 bytes per (sample, plane, corner) plus up to 2 x 3 C H W floats.
 * Both calls are enqueued on `stream` without synchronising. */
GPCC_API int gsge_plane_forward(gpcc_ctx *ctx, const float *planes, const float *coordinates, const float *max_coords, const float *min_coords,
                                double radii, int64_t n, int k, int repeat, int channels, int height, int width, float *out, gsr_alloc_fn alloc,
                                void *alloc_user, void *stream);
GPCC_API int gsge_plane_backward(gpcc_ctx *ctx, const float *grad_out, const float *planes, const float *coordinates, const float *max_coords,
                                 const float *min_coords, double radii, int64_t n, int k, int repeat, int channels, int height, int width,
                                 float *grad_planes, float *grad_coordinates, gsr_alloc_fn alloc, void *alloc_user, void *stream);
/* The context rows: the sampler with an output row of k * 3 * C + tail_width floats whose last tail_width columns are a copy of row n of
 * `tail` (n, tail_width) float32 contiguous -- TC-GS's torch.cat([feat_context, anchor], dim=1) (gaussian_renderer/__init__.py:66), the
 * (N, 603) input of mlp_triplane, written once.  tail_width in [0, 16] (0: tail may be NULL; the two calls above are these with 0 and give
 * the same bits); with a tail k <= 64 in both coordinate forms.  The feature columns are the sampler's, bit for bit; the tail is copied.
 * gsge_plane_rows_backward reads grad_out (n, k * 3 * C + tail_width) in place, rows that many floats apart: no contiguous copy of the
 * feature columns is needed.  The tail's gradient is the column view grad_out[:, k * 3 * C:], which the caller takes itself. */
GPCC_API int gsge_plane_rows_forward(gpcc_ctx *ctx, const float *planes, const float *coordinates, const float *max_coords, const float *min_coords,
                                     double radii, int64_t n, int k, int repeat, int channels, int height, int width, const float *tail,
                                     int tail_width, float *out, gsr_alloc_fn alloc, void *alloc_user, void *stream);
GPCC_API int gsge_plane_rows_backward(gpcc_ctx *ctx, const float *grad_out, const float *planes, const float *coordinates, const float *max_coords,
                                      const float *min_coords, double radii, int64_t n, int k, int repeat, int channels, int height, int width,
                                      int tail_width, float *grad_planes, float *grad_coordinates, gsr_alloc_fn alloc, void *alloc_user,
                                      void *stream);

/* ================= Multi-scale tri-plane features (CAT-3DGS/scene/triplane.py: TriPlaneField.forward / get_density :246-342,
 * interpolate_ms_features :89-146, grid_sample_wrapper :40-65) =================
 * pts (n, 3); planes: 3 * n_levels device pointers in (level, plane) order, plane i (C, heights[i], widths[i]) with one C for all
 * (for a resolution (rx, ry, rz) and a multiplier m the reference's planes are (m ry, m rx), (m rz, m rx), (m rz, m ry) as (H, W));
 * n_levels in [1, 8]; level: the `level` argument of interpolate_ms_features (get_density passes 2); quantise: read rintf(16 v) / 16 for
 * a texel v (STEQuantizer(latent * 16) / 16: both scalings are exact and torch.round rounds halves to even, so the fused form has the
 * materialised one's bits).  The transform, all float32 DEVICE pointers (no host copy, no synchronisation): aabb (2, 3) always; with
 * contract also pca_mean (3), rotation (3, 3), variance (3), con_aabb (2, 3).  Per point, float32 in the reference's expression order:
 *   contract:  p = pts - pca_mean; q_j = sum_i p_i rotation[i][j]; q = q / variance; x = ((q + 1) / 2) * 2 - 1; mag = |x|_2
 *              x = (2 - 1 / mag) (x / mag) where mag > 1, else x, formed as the reference's blend x_c m + x (1 - m) with m = 0 / 1
 *              x = x / 4 + 0.5; g = (x - con_aabb[0]) * ((aabb[1] - aabb[0]) / (con_aabb[1] - con_aabb[0])) + aabb[0]
 *   otherwise: g = (pts - aabb[0]) * (2 / (aabb[1] - aabb[0])) - 1
 *   plane p of every level reads the components (0, 1), (0, 2), (1, 2) of g, the first along W, the second along H
 *   bilinear grid_sample, align_corners true, padding border: pixel = (g + 1) / 2 * (size - 1) clamped to [0, size - 1]; corners and
 *   weights as grid_sample forms them; a corner at index `size` has weight 0 and is never read
 *   T_l = the (3 C) concatenation of level l's three reads; F_0 = T_0; F_l = T_l + F_{l-1} if level > l, else F_{l-1}
 *   out[n, l * 3 C + p * C + ch] = F_l[p * C + ch]: out (n, n_levels * 3 * C)
 * contract = 0 / 1 select the two lines above; 2: pts are contract_to_unisphere's output already and only the last line (the reference's
 * con_normalize_aabb, what get_density applies) runs, reading aabb and con_aabb; 3: g = pts, nothing is read (interpolate_ms_features).
 * A point whose g is not finite in every component gives a zero row and no gradient, and no index is formed from it.  (The reference
 * yields NaN there: a point the PCA step maps to the origin has 1 / mag = inf in its blend, which this code reproduces and then drops.)
 * Limits: C in [1, 256], H and W in [2, 4096], n * 3 * n_levels * 4 < 2^32; a violation returns GPCC_ERR_ARG before any launch.
 * n = 0 launches nothing (the backward zeroes the plane gradients).
 * gsge_msplane_backward: grad_out (n, n_levels * 3 * C).  The gradient reaching T_l is the sum, in ascending block order, of the
 * grad_out blocks l' >= l when level l takes part (l = 0 or level > l), and nothing otherwise.  OVERWRITES grad_planes[i], shaped as
 * plane i (the straight-through quantiser passes it unchanged) and, when grad_pts is not NULL, grad_pts (n, 3): through the bilinear
 * weights (quantised texels when quantise), zero along an axis whose pixel coordinate was clamped (as torch's border clipping sets it),
 * and normalize_aabb's scale (contract = 0; none for 3).  With contract the reference detaches the points: a non-NULL grad_pts with
 * contract = 1 or 2 is GPCC_ERR_ARG.
 * `planes` is read only for grad_pts (it may be NULL otherwise).  No gradient for the transform's parameters.
 * Bitwise reproducible: no float atomics (one (texel row, slot) key per (point, level, plane, corner), the rows of all planes in one
 * key space (a plane's base row plus y W + x), stable radix sort by row, fixed-order sums).
 * Workspace through `alloc`: forward C floats per texel of all planes; backward about 28 bytes per (point, level, plane, corner) plus
 * up to twice the forward's.  Both calls are enqueued on `stream` without synchronising. */
GPCC_API int gsge_msplane_forward(gpcc_ctx *ctx, const float *pts, int64_t n, int n_levels, const float *const *planes, int channels,
                                  const int *heights, const int *widths, int level, int quantise, int contract, const float *pca_mean,
                                  const float *rotation, const float *variance, const float *aabb, const float *con_aabb, float *out,
                                  gsr_alloc_fn alloc, void *alloc_user, void *stream);
GPCC_API int gsge_msplane_backward(gpcc_ctx *ctx, const float *grad_out, const float *pts, int64_t n, int n_levels, const float *const *planes,
                                   int channels, const int *heights, const int *widths, int level, int quantise, int contract,
                                   const float *pca_mean, const float *rotation, const float *variance, const float *aabb, const float *con_aabb,
                                   float *const *grad_planes, float *grad_pts, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* Backward of gshac_mlp2_act (the training forward IS gshac_mlp2_act: nothing is saved).  Recomputes h = b1 + x W1^T with the forward's chain, so
 * the activation mask is the forward's bit for bit (act' = 0 / slope at h <= 0, as torch), then g = (dy W2) o act'(h), dx = g W1, dW2 = dy^T act(h),
 * db2 = sum dy, dW1 = g^T x, db1 = sum g.  dy (n, dout); OVERWRITES dw1 (dh, din), db1 (dh), dw2 (dout, dh), db2 (dout) and, when it is not NULL,
 * dx (n, din): a NULL dx skips that product and leaves the bits of the others unchanged.  The rows are cut into slabs of gshac_mlp2_slab_rows rows
 * (a function of n and the sizes alone); every slab writes one partial of the parameter gradients into the workspace (slabs x (parameters + dh
 * + dout) floats, through alloc) and a second launch adds them in slab order; the bias gradients, and the sum over the slabs, are compensated
 * sums in that fixed order: no atomics, bitwise reproducible.  n == 0 zeroes the parameter gradients.  All
 * pointers device; no host synchronisation.  The layer sizes are the forward's (16 (din + dh) floats <= 64 KB). */
GPCC_API int gshac_mlp2_backward(gpcc_ctx *ctx, const float *x_dev, const float *w1_dev, const float *b1_dev, const float *w2_dev, const float *b2_dev,
                                 int64_t n, int din, int dh, int dout, int act, float slope, const float *dy_dev, float *dx_dev, float *dw1_dev,
                                 float *db1_dev, float *dw2_dev, float *db2_dev, gsr_alloc_fn alloc, void *alloc_user, void *stream);
/* rows per slab of gshac_mlp2_backward for n rows of this layer (0 for sizes it does not take) */
GPCC_API int64_t gshac_mlp2_slab_rows(int64_t n, int din, int dh, int dout);

/* ================= Tri-plane ARM rate (CAT-3DGS/scene/arm.py: get_neighbor, ArmMLP, compute_rate; scene/triplane.py: get_density) =================
 * The rate of quantised latents under the auto-regressive model.  y[v]: level v, (channels[v], heights[v], widths[v]) float32 device,
 * contiguous, any values; n_levels in [0, 64], every level of at most 2^30 latents.  The MLP: dims[0 .. n_layers] are its widths, dims[0] = 12
 * (the causal half of a 5 x 5 mask), 1 to 8 hidden widths in [1, 32], dims[n_layers] = 2; params holds w (out, in) then b (out) of every
 * layer in order, one flat float32 device buffer.  Hidden widths 16, 16, 16, 16 take a specialised kernel, anything else a generic one.
 * Per latent (c, h, w), in float32:
 *   ctx_i = y[c, h - 2 + i / 5, w - 2 + i % 5], i = 0..11, 0 outside the plane; never another channel
 *   a layer is x W^T + b (+ x for a hidden layer whose widths agree), a ReLU behind every hidden layer; (mu, ls) = MLP(ctx)
 *   s = exp(-0.5 clamp(ls, -10, 13.8155)); F(t) = 0.5 - 0.5 sign(t - mu) expm1(-|t - mu| / s)
 *   rate = -log2(max(F(x + 0.5) - F(x - 0.5), 2^-16))
 * gsarm_rate_forward writes any of rate, mu, scale (flat over the levels in (level, c, h, w) order; NULL = not wanted) and rate_sum (one
 * value: per-lane sums in double, a fixed tree per workgroup, the workgroups in order).  alloc is needed for rate_sum only (8 bytes per
 * workgroup and level, at most 1024 workgroups).
 * gsarm_rate_backward: grad_rate is shaped as rate, or one device value when grad_is_scalar (the summed form).  OVERWRITES grad_y[v]
 * (shaped as y[v]; NULL entries, or a NULL array, are skipped) and grad_params (shaped as params; NULL = not wanted).  Nothing but the
 * latent is read: the hidden layers are recomputed.  autograd's choices at the kinks: the floor passes iff the probability is >= 2^-16
 * (a latent on it adds exactly 0 to every gradient), the clamp passes iff -10 <= ls <= 13.8155, a ReLU where its output is > 0.
 * The context part of a latent's gradient is a gather from a scratch of 12 floats per latent of the largest level; parameter gradients
 * are sums per persistent workgroup (at most 1024, carried across the levels), added in a fixed order.  No atomics: bitwise
 * reproducible.  Workspace through alloc: 12 x 4 bytes per latent of the largest level (when a grad_y is wanted) plus workgroups x
 * parameters doubles (when grad_params is).  Both calls are enqueued on `stream` without synchronising. */
GPCC_API int gsarm_rate_forward(gpcc_ctx *ctx, int n_levels, const float *const *y, const int *channels, const int *heights, const int *widths,
                                const float *params, int n_layers, const int *dims, float *rate, float *rate_sum, float *mu, float *scale,
                                gsr_alloc_fn alloc, void *alloc_user, void *stream);
GPCC_API int gsarm_rate_backward(gpcc_ctx *ctx, int n_levels, const float *const *y, const int *channels, const int *heights, const int *widths,
                                 const float *params, int n_layers, const int *dims, const float *grad_rate, int grad_is_scalar,
                                 float *const *grad_y, float *grad_params, gsr_alloc_fn alloc, void *alloc_user, void *stream);

/* ================= Tri-plane latent bitstream (CAT-3DGS/scene/gaussian_model.py: encode_triplane / decode_triplane) =================
 * The levels of one plane, coded under the ARM above (same levels / params / dims arguments; the latents must be integers).  The byte
 * format is this library's own, not the reference's `constriction` streams.  Per latent (mu, s) are what
 * gsarm_rate_forward returns, quantised mu_q = rint(16 mu) / 16, s_q = max(rint(16 s) / 16, 1 / 16).  Alphabet of a level:
 * A = ceil(max |y|) + 2 (at most 1024), L = 2 A + 1 symbols, index y + A.  A CDF row has L + 1 uint16 entries: 0, then
 * rint(F(j - A - 0.5) (65536 - L)) + j for 0 < j < L, then 2^16 (stored as 0), F the Laplace CDF above in float32.
 * A channel's plane is cut into K = ceil(W / S) strips of S = strips[v] >= 4 columns (K <= 1024); strip k of channel c is chunk
 * c K + k: its symbols by row, then by column, one torchac-compatible carry-less stream (== gsac_host_encode_u16 on them).
 * gsac_arm_encode: finds A per level (alphabet_out[v]), codes every chunk; *bytes_out = the chunks' bytes in (level, channel, strip)
 *   order, *cnt_out = their byte counts (context-owned host memory, valid until the context's next call).  GPCC_ERR_RANGE when a latent
 *   is not an integer, an alphabet would exceed 1024, or a mu / scale is not finite (nothing usable is returned).
 * gsac_arm_decode: the inverse into y_out[v] (device, shaped as the levels); bytes / cnt are HOST pointers as gsac_arm_encode returned
 *   them.  One workgroup per channel, one lane per strip: at step T lane k decodes the segment of row (T - k) / 2 when T - k is even,
 *   a workgroup barrier per step, K + 2 H - 2 steps.  Bytes past a chunk's count read as zero and symbols stay inside the alphabet: a
 *   wrong payload decodes to some grid.  Both calls synchronise `stream`.
 * gsac_arm_cdf_rows: the integer rows of n (mu_q, s_q) pairs (already quantised, device) -> rows_out (n, 2 A + 2) uint16, device. */
GPCC_API int gsac_arm_encode(gpcc_ctx *ctx, int n_levels, const float *const *y, const int *channels, const int *heights, const int *widths,
                             const int *strips, const float *params, int n_layers, const int *dims, int *alphabet_out, const uint8_t **bytes_out,
                             int64_t *nbytes_out, const int32_t **cnt_out, int64_t *nchunks_out, void *stream);
GPCC_API int gsac_arm_decode(gpcc_ctx *ctx, int n_levels, float *const *y_out, const int *channels, const int *heights, const int *widths,
                             const int *strips, const int *alphabets, const float *params, int n_layers, const int *dims, const uint8_t *bytes,
                             int64_t nbytes, const int32_t *cnt, int64_t nchunks, void *stream);
GPCC_API int gsac_arm_cdf_rows(gpcc_ctx *ctx, const float *mu, const float *scale, int64_t n, int A, uint16_t *rows_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSPCC_H */
