/*
 * zvec_hip.h — C ABI of the MI355X (gfx950) flat / IVF-Flat distance-scan core for zvec.
 *
 * This is the drop-in boundary: plain C, opaque handles, plain pointers and sizes, `int` status
 * (0 = success, negative = the reference's IndexError value, src/include/zvec/core/framework/
 * index_error.h:39-62 / src/core/framework/index_error.cc:20-71).  The reference has no FFI for this
 * path (it is in-process C++); every entry point below states the reference C++ operator it stands
 * behind, so that the C++ subclasses a maintainer registers with INDEX_FACTORY_REGISTER_STREAMER /
 * _SEARCHER are one-line forwards.
 *
 * Scores are the reference's metric-kernel ("boundary B") scores, smaller = better:
 *   L2 -> squared Euclidean, IP -> MINUS inner product, COSINE -> 1 - ip on normalised rows.
 * `core_interface::Index::_dense_search` (src/core/interface/index.cc:624-649) applies
 * metric->normalize() above this boundary (IP: negate) and keeps doing so unchanged.
 *
 * Pointers named d_* are DEVICE pointers on the handle's GPU; all others are host pointers.
 * *_dev entry points are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 * context's own stream); the host-pointer forms copy in/out and return after completion.
 */
#ifndef ZVEC_HIP_H_
#define ZVEC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZVEC_HIP_ABI_VERSION 1

/* IndexMeta::DataType subset (src/include/zvec/core/framework/index_meta.h:27-50) */
enum {
  ZVEC_HIP_DT_FP32 = 0,
  ZVEC_HIP_DT_FP16 = 1,
  ZVEC_HIP_DT_BINARY32 = 2, /* IndexMeta::DT_BINARY32 = 7 (index_meta.h:39): a row is dim / 32 uint32_t words */
  ZVEC_HIP_DT_BINARY64 = 3  /* IndexMeta::DT_BINARY64 = 8 (index_meta.h:40): a row is dim / 64 uint64_t words */
};

/* IndexMetric names served: "SquaredEuclidean" (src/core/metric/euclidean_metric.cc:743),
 * "InnerProduct" (inner_product_metric.cc:256), "Cosine" (cosine_metric.cc:141). */
enum {
  ZVEC_HIP_METRIC_L2 = 0,
  ZVEC_HIP_METRIC_IP = 1,
  ZVEC_HIP_METRIC_COSINE = 2,
  ZVEC_HIP_METRIC_HAMMING = 3 /* "Hamming" (src/core/metric/hamming_metric.cc:236) */
};

/* Binary rows (flat indexes, and inverted lists through the zvec_hip_bivf_* family below).  HammingMetric accepts DT_BINARY32 / DT_BINARY64 and nothing else (hamming_metric.cc:146-147)
 * and scores a pair with HammingDistanceMatrix<uint32_t / uint64_t> (src/ailego/math/hamming_distance_matrix.h:41, :339):
 *   - `dim` counts BITS; a row is dim / 32 uint32_t (BINARY32) or dim / 64 uint64_t (BINARY64) words in the host's byte order,
 *     dim / 8 bytes either way; dim must be a non-zero multiple of 32 resp. 64 (the reference asserts !(dim & 31) / !(dim & 63))
 *     and at most 2^20: zvec_hip_flat_create returns ZVEC_HIP_ERR_INVALID_ARGUMENT otherwise;
 *   - score = (float) popcount(row ^ query), smaller is better; exact for every dim within the cap;
 *   - ZVEC_HIP_METRIC_HAMMING goes with a binary dtype only and a binary dtype with ZVEC_HIP_METRIC_HAMMING only: every other
 *     pairing is ZVEC_HIP_ERR_MISMATCH;
 *   - served on a binary handle: flat_create / destroy / reserve, append, append_dev, put, holes, count, get_vector(s), search,
 *     search_dev, search_by_ids, batch_distance, build_filter (exclude_bitset and threshold mean what they mean elsewhere: a
 *     document is dropped iff score > threshold), and — DT_BINARY32 only, fed with fp32 rows / queries that are turned into sign
 *     bits on the device ("fp32 -> sign bits" below) — append_fp32, append_fp32_dev, search_fp32, search_fp32_dev;  ZVEC_HIP_ERR_UNSUPPORTED: search_grouped*, the shadow entries, load_features,
 *     load_blocks, zvec_hip_shards_create and zvec_hip_ivf_create with a binary dtype (inverted lists over binary rows are a handle
 *     family of their own: zvec_hip_bivf_create);
 *   - lists are ascending by score; which of several equal scores are returned at the k-th place, and their order, is unspecified
 *     (the reference's heap resolves ties arbitrarily). */

/* IndexError values used (index_error.cc:20-71) */
enum {
  ZVEC_HIP_OK = 0,
  ZVEC_HIP_ERR_RUNTIME = -1,           /* IndexError_Runtime (a HIP call failed) */
  ZVEC_HIP_ERR_UNSUPPORTED = -12,      /* IndexError_Unsupported */
  ZVEC_HIP_ERR_OUT_OF_RANGE = -17,     /* IndexError_OutOfRange */
  ZVEC_HIP_ERR_NO_MEMORY = -19,        /* IndexError_NoMemory (device or host allocation failed) */
  ZVEC_HIP_ERR_NO_READY = -21,         /* IndexError_NoReady */
  ZVEC_HIP_ERR_NO_EXIST = -22,         /* IndexError_NoExist (position / key not found) */
  ZVEC_HIP_ERR_MISMATCH = -24,         /* IndexError_Mismatch (dim / dtype / metric mismatch) */
  ZVEC_HIP_ERR_INVALID_ARGUMENT = -31, /* IndexError_InvalidArgument */
  ZVEC_HIP_ERR_NO_INDEX_LOADED = -204, /* IndexError_NoIndexLoaded */
  ZVEC_HIP_ERR_NO_TRAINED = -205       /* IndexError_NoTrained */
};

typedef struct zvec_hip_flat_s *zvec_hip_flat_t;
typedef struct zvec_hip_ivf_s *zvec_hip_ivf_t;
typedef struct zvec_hip_ctx_s *zvec_hip_ctx_t;
typedef struct zvec_hip_shards_s *zvec_hip_shards_t;
typedef struct zvec_hip_gate_s *zvec_hip_gate_t;
typedef struct zvec_hip_sparse_s *zvec_hip_sparse_t;
typedef struct zvec_hip_bivf_s *zvec_hip_bivf_t;

/* library / device ------------------------------------------------------------------------- */
int zvec_hip_abi_version(void);
int zvec_hip_device_count(int *count);
const char *zvec_hip_error_string(int code); /* IndexError::What analogue */

/* Process-wide options of the host-pointer entry points (also read from the environment at first use: ZVEC_HIP_WAIT,
 * ZVEC_HIP_ZEROCOPY).  zvec calls boundary B with ONE query per call from many threads, each with its own context
 * (src/core/interface/index.cc:24-45,605-619; tools/core/bench.cc:145-245), so how a call waits and how 3 KB travel matter:
 *   "wait"      0 = spin in hipStreamSynchronize; 1 (default) = poll a completion word in pinned memory — spinning while the
 *               answer is ~0.1 ms away, SLEEPING when the previous wait on the context was long (64 spinning callers exhaust a
 *               16-CPU quota and are frozen by the scheduler for most of every period: 19.5 k searches/s at 16 threads fell to
 *               5.2 k at 64; sleeping: 18.4 k); 2 = block on a hipEventBlockingSync event
 *   "zerocopy"  transfers up to 256 KiB may skip the copy engine through host-mapped pinned slots of the context: bit 1 (value 2,
 *               the default) = the last kernels write keys | scores | counts straight into host memory; bit 0 = the first kernel
 *               reads the queries in place (measured slower than the staged copy: off by default); 0 = staged copies both ways
 *   "assign256" 1 (default) = fp16 labelling / k-means assignment on the 256 x 256 multi-phase tile; 0 = the 128 x 128 tile
 *   "scan256"   1 (default) = flat scans of fp16 rows by at least 256 queries with k <= 11 and no filter take the 256 x 256
 *               multi-phase tile when the base is streamed (past the Infinity Cache); 2 = on small bases too (tests); 0 = the
 *               128 x 128 tile always.  Same results either way (ZVEC_HIP_ASSIGN256 / ZVEC_HIP_SCAN256 in the environment).
 *   "sparse_group_rows"  0 .. 64: zvec_hip_sparse_search_grouped dumps the scores of a sub-batch of at most this many queries
 *               with a whole wave per stored row, of a wider one with a lane per query; 0 = never the former.  Same lists
 *               either way on exact data.
 *   "sparse_inverted_build"  1 (default) = the inverted lists of a sparse index are built on the device; 0 = on the host, the
 *               reference of the device build.  Read when a build starts.  The same bytes, and so the same search results,
 *               either way.
 *   "bivf_part_bytes"  1024 .. 2^30 (default 2^30): a zvec_hip_bivf_search keeps the partial lists of one slice of its batch within
 *               this many bytes and answers a batch that needs more in slices of queries.  Same results either way.
 *   "hnsw_build_round_div"  0 .. 2^20 (default 16), "hnsw_build_round_max"  1 .. 2^20 (default 4096): the rounds of zvec_hip_hnsw_build
 *   "hnsw_ws_bytes"  1024 .. 2^30 (default 2^30): a zvec_hip_hnsw_search keeps the visited bits and candidate regions of one slice of
 *               its batch within this many bytes and answers a batch that needs more in slices of queries.  Same results either way.
 * Unsupported (-12) for an unknown name, invalid argument (-1) for a value outside the option's range. */
int zvec_hip_set_option(const char *name, int value);
int zvec_hip_get_option(const char *name, int *value);

/* Page-locked host memory for callers that assemble query batches themselves (the micro-batcher of include/zvec_hip_operator.hpp
 * gathers the single queries of zvec's caller threads into such a block): a host-pointer search whose `queries` lie in it uploads
 * them in one DMA instead of the runtime's staged copy of pageable memory.  NoMemory (-19) when the allocation fails. */
int zvec_hip_host_alloc(uint64_t bytes, void **out);
int zvec_hip_host_free(void *p);

/* search context: IndexRunner::create_context() (index_runner.h:400-470).  One per caller thread;
 * owns a HIP stream and the scan workspace.  Passing NULL to a search uses the handle's built-in
 * context under a mutex. */
int zvec_hip_ctx_create(int device, zvec_hip_ctx_t *out);
int zvec_hip_ctx_destroy(zvec_hip_ctx_t ctx);
int zvec_hip_ctx_synchronize(zvec_hip_ctx_t ctx);
/* bind the context to a caller-owned hipStream_t (e.g. torch's current stream); NULL restores its own */
int zvec_hip_ctx_set_stream(zvec_hip_ctx_t ctx, void *stream);

/* Pipelining consecutive batches.  The reference overlaps queries by giving every caller thread its own context
 * (index.cc:24-45); on the GPU one search is a short sequence of small kernels around ONE bandwidth- or MFMA-bound scan.
 * Contexts that share a gate run that dominant scan kernel one after the other, in call order, while everything else of
 * their searches (query preparation, coarse pass, plan, merges, L2 refinement, the caller's candidate exchange) overlaps
 * the other context's scan: with two contexts on two streams the device runs scans back to back.  A gate is one HIP
 * event, re-recorded behind every gated scan and waited for in front of the next; contexts and gate on one device.
 * Destroy the gate after detaching (set_gate(ctx, NULL)) or destroying its contexts. */
int zvec_hip_gate_create(int device, zvec_hip_gate_t *out);
int zvec_hip_gate_destroy(zvec_hip_gate_t gate);
int zvec_hip_ctx_set_gate(zvec_hip_ctx_t ctx, zvec_hip_gate_t gate);

/* ---- flat (brute force) -------------------------------------------------------------------
 * stands behind FlatStreamer<32> / FlatSearcher<32>
 *   (src/core/algorithm/flat/flat_streamer.cc:304-389, flat_searcher.cc:162-211).
 * `dim` is the element dimension of IndexMeta (for COSINE: d+1 floats, or d+2 halves for DT_FP16 — the
 * trailing fp32 norm written by CosineConverter, cosine_converter.cc:112-134,205-212; it is not scanned). */
int zvec_hip_flat_create(uint32_t dim, int dtype, int metric, int device, zvec_hip_flat_t *out);
int zvec_hip_flat_destroy(zvec_hip_flat_t h);
int zvec_hip_flat_reserve(zvec_hip_flat_t h, uint64_t capacity);
/* IndexStreamer::add_impl / add_with_id_impl (index_runner.h:476-487), FlatBuilder::build
 * (flat_builder.cc:188-276): append n rows (dim elements each) in storage order.
 * keys == NULL -> key = storage position. */
int zvec_hip_flat_append(zvec_hip_flat_t h, const void *vecs, uint64_t n, const uint64_t *keys);
int zvec_hip_flat_append_dev(zvec_hip_flat_t h, const void *d_vecs, uint64_t n,
                             const uint64_t *d_keys, void *stream);
/* IndexStreamer::add_with_id_impl(id, vec, qmeta, ctx) in bulk (index_runner.h:483-487) — what core_interface::Index::_dense_add
 * calls for every document (src/core/interface/index.cc:505-537).  FlatStreamerEntity::add_vector_with_id semantics
 * (flat_streamer_entity.cc:900-990), row by row: the row of ids[i] lives at storage position ids[i] under key ids[i];
 * id == count appends, id > count first pads positions [count, id) with holes (kInvalidKey rows no search returns),
 * id < count overwrites in place.  keys: NULL (key = id, the reference's rule) or the key to store with each row, for
 * a caller that keeps its own id -> position map.  zvec_hip_flat_holes: hole positions currently in the store. */
int zvec_hip_flat_put(zvec_hip_flat_t h, const uint32_t *ids, uint64_t n, const void *vecs, const uint64_t *keys);
int zvec_hip_flat_holes(zvec_hip_flat_t h, uint64_t *count);
int zvec_hip_flat_count(zvec_hip_flat_t h, uint64_t *count);
/* IndexRunner::get_vector_by_id (index_runner.h:450-453): copy row `pos` (dim elements) to out. */
int zvec_hip_flat_get_vector(zvec_hip_flat_t h, uint64_t pos, void *out);
/* the same for a list of positions in one launch + one copy (IndexContext::set_fetch_vector, index_context.h:139:
 * the vectors of a result list, index.cc:635-647); out = n rows of the element type, row-major */
int zvec_hip_flat_get_vectors(zvec_hip_flat_t h, const uint64_t *positions, uint64_t n, void *out);
/* search_impl / search_bf_impl(query, qmeta, count, ctx) (index_runner.h:490-531).
 * exclude_bitset: nullable, 1 bit per storage position (bit i of word i/64), set = filter(key)
 * returned true = excluded (IndexFilter, index_filter.h:48-50).
 * threshold: IndexContext::threshold() RNN radius, FLT_MAX = none (index_document.h:250-261).
 * outputs: [count][topk] keys / scores ascending by score, out_counts[q] valid entries. */
int zvec_hip_flat_search(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *queries,
                         uint32_t count, uint32_t topk, float threshold,
                         const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                         uint32_t *out_counts);
int zvec_hip_flat_search_dev(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *d_queries,
                             uint32_t count, uint32_t topk, float threshold,
                             const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                             float *d_out_scores, uint32_t *d_out_counts, void *stream);

/* FlatStreamer::search_bf_by_p_keys_impl (flat_streamer.cc:346-389; index_runner.h:579-585): query q is
 * compared only with the rows ids[offsets[q] .. offsets[q+1]) (storage positions; the host maps primary
 * keys to positions and drops unknown keys, as get_vector_by_key != 0 -> continue does).  Same outputs and
 * filter / threshold meaning as zvec_hip_flat_search. */
int zvec_hip_flat_search_by_ids(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *queries,
                                uint32_t count, const uint32_t *ids, const uint32_t *offsets,
                                uint32_t topk, float threshold, const uint64_t *exclude_bitset,
                                uint64_t *out_keys, float *out_scores, uint32_t *out_counts);

/* Group-by search: search_impl / search_bf_impl of a context with set_group_params(group_num, group_topk) and
 * set_group_by(fn) (index_context.h:129,215; FlatSearcherContext::group_by_search_impl, flat_searcher_context.h:1005-1043;
 * FlatStreamer::group_by_search_impl, flat_streamer.cc:391-437; result assembly topk_to_group_result,
 * flat_streamer_context.h:135-180).  Every group keeps its `group_topk` closest documents; the `group_num` groups whose
 * best document is closest are returned, best group first.  group_of_position[pos] (host, one entry per stored row, values
 * < ngroups; larger values = "no group", skipped) is the caller's group_by(key) mapped to dense numbers — the plugin sweeps
 * the std::function once per key, like the filter.  Outputs: out_groups[count][group_num] group numbers (out_ngroups[q]
 * valid), out_keys / out_scores [count][group_num][group_topk] ascending, out_counts[count][group_num] documents at or
 * below `threshold` (a group whose best document is beyond the radius is listed with 0 documents, as the reference does).
 * Filter bits as in zvec_hip_flat_search. */
int zvec_hip_flat_search_grouped(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count,
                                 const uint32_t *group_of_position, uint32_t ngroups, uint32_t group_num, uint32_t group_topk,
                                 float threshold, const uint64_t *exclude_bitset, uint32_t *out_groups, uint32_t *out_ngroups,
                                 uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
/* FlatStreamer::group_by_search_p_keys_impl (flat_streamer.cc:439-483): the grouped form of zvec_hip_flat_search_by_ids */
int zvec_hip_flat_search_grouped_by_ids(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count,
                                        const uint32_t *ids, const uint32_t *offsets, const uint32_t *group_of_position,
                                        uint32_t ngroups, uint32_t group_num, uint32_t group_topk, float threshold,
                                        const uint64_t *exclude_bitset, uint32_t *out_groups, uint32_t *out_ngroups,
                                        uint64_t *out_keys, float *out_scores, uint32_t *out_counts);

/* IndexMetric::batch_distance (src/include/zvec/core/framework/index_metric.h:85-87; ailego BaseDistance::ComputeBatch,
 * src/ailego/math_batch/distance_batch.h:29-49): ONE query against n scattered stored rows (storage positions), scores
 * only, in the listed order — the one-to-many form the graph indexes drive; for L2 / IP the reference's batch form is a
 * loop of the 1x1 kernel.  Positions beyond the row count score +inf. */
int zvec_hip_flat_batch_distance(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *query, const uint32_t *positions,
                                 uint32_t n, float *out_scores);

/* ---- IVF-Flat -----------------------------------------------------------------------------
 * stands behind IVFStreamer / IVFSearcher (src/core/algorithm/ivf/ivf_streamer.cc:183-250,
 * ivf_searcher.cc:183-250) with IVFCentroidIndex (ivf_centroid_index.cc:273-297) and
 * IVFEntity::search (ivf_entity.cc:587-716).
 * Searches on separate contexts may run while another thread loads or rebuilds the index: they see the old index or the
 * new one, or ZVEC_HIP_ERR_NO_INDEX_LOADED between begin_lists and end_lists. */
int zvec_hip_ivf_create(uint32_t dim, int dtype, int metric, int device, zvec_hip_ivf_t *out);
int zvec_hip_ivf_destroy(zvec_hip_ivf_t h);
/* load a trained index (what IVFSearcher::load reads from the ivf.* segments,
 * ivf_index_format.h:26-60,152-164): centroids [nlist][dim]; rows in inverted-list order, list l
 * owning rows [list_offsets[l], list_offsets[l+1]); keys per row (NULL -> row number). */
int zvec_hip_ivf_load(zvec_hip_ivf_t h, const void *centroids, uint32_t nlist,
                      const uint64_t *list_offsets, const void *vecs, const uint64_t *keys);
/* IVFBuilder::train + build on the GPU (ivf_builder.cc:212-403): k-means over a sample, nearest-
 * centroid labelling, list packing.  d_vecs: [n][dim] row-major DEVICE rows; keys: host, nullable.
 * The trained structure can be read back with zvec_hip_ivf_export so that a CPU reference can
 * search the very same index. */
int zvec_hip_ivf_build_dev(zvec_hip_ivf_t h, const void *d_vecs, uint64_t n, const uint64_t *keys,
                           uint32_t nlist, uint32_t kmeans_iters, uint32_t sample_per_list,
                           uint64_t seed, void *stream);
int zvec_hip_ivf_build(zvec_hip_ivf_t h, const void *vecs, uint64_t n, const uint64_t *keys,
                       uint32_t nlist, uint32_t kmeans_iters, uint32_t sample_per_list,
                       uint64_t seed);
int zvec_hip_ivf_info(zvec_hip_ivf_t h, uint64_t *count, uint32_t *nlist);
/* read back: centroids [nlist][dim], list_offsets [nlist+1], row_ids [count] = original row number
 * (build) / load-order row (load) of each list-order position; any pointer may be NULL. */
int zvec_hip_ivf_export(zvec_hip_ivf_t h, void *centroids, uint64_t *list_offsets,
                        uint64_t *row_ids);
int zvec_hip_ivf_get_vector(zvec_hip_ivf_t h, uint64_t list_pos, void *out);
int zvec_hip_ivf_get_vectors(zvec_hip_ivf_t h, const uint64_t *list_positions, uint64_t n, void *out);
/* IVFSearcher::search_impl(query, qmeta, count, ctx):
 *   nprobe         = max(round(nlist*scan_ratio),1)          ivf_searcher_context.h:70-74
 *   max_scan_count = max(bf_threshold, ceil(N*scan_ratio))    ivf_searcher_context.h:75-78
 * lists are probed in coarse-score order while the running scanned count < max_scan_count
 * (ivf_searcher.cc:217-237).  exclude_bitset is over list-order positions. */
int zvec_hip_ivf_search(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count,
                        uint32_t topk, float threshold, uint32_t nprobe, uint32_t max_scan_count,
                        const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                        uint32_t *out_counts);
int zvec_hip_ivf_search_dev(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *d_queries,
                            uint32_t count, uint32_t topk, float threshold, uint32_t nprobe,
                            uint32_t max_scan_count, const uint64_t *d_exclude_bitset,
                            uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts,
                            void *stream);
/* The coarse pass apart from the rest, for a sharded index.  Every shard must plan from the SAME probe sets, and the
 * pass (2 x Q x nlist x d flop against the replicated centroids, IVFCentroidIndex::search, ivf_centroid_index.cc:273-297) is the one
 * part of a shard's step that does not shrink with the number of shards.  Dealt over the shards instead: shard r runs
 * zvec_hip_ivf_coarse_dev on its slice of the batch, the probe lists — d_probe_idx [count][min(nprobe, nlist)] centroid ids in
 * coarse-score order, d_probe_cnt [count] valid entries — are exchanged (Q x nprobe x 4 bytes), and every shard runs
 * zvec_hip_ivf_search_probes_dev, which is zvec_hip_ivf_search_dev without its coarse pass (ivf_searcher.cc:217-247 from the
 * given lists; the max_scan_count rule still uses the global list sizes).  Same results as zvec_hip_ivf_search_dev. */
int zvec_hip_ivf_coarse_dev(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t nprobe,
                            uint32_t *d_probe_idx, uint32_t *d_probe_cnt, void *stream);
int zvec_hip_ivf_search_probes_dev(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk,
                                   float threshold, uint32_t nprobe, uint32_t max_scan_count, const uint32_t *d_probe_idx,
                                   const uint32_t *d_probe_cnt, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                                   float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* Half-width pre-selection for an fp32 L2 / inner-product index ("shadow lists"): same results, about half the bytes per search.
 * IVFSearcher::search_impl scores every row of the probed lists in fp32 (ivf_searcher.cc:217-247, ivf_entity.cc:664-717); on the
 * GPU that scan is bound by the bytes of the lists.  zvec_hip_ivf_set_shadow(h, 1, preselect) stores every row a second time rounded
 * to fp16 (HalfFloatConverter's rounding) at the same positions; searches of more than a handful of queries (no radius, k <= 32) then
 * scan the fp16 rows for `preselect` rows per query (0: chosen by the index, from max(32, 3k): zvec_hip_ivf_shadow_width; <= 64), re-score those on the fp32 rows with the kernel that
 * refines the fp32 route's final lists, keep the k best and CERTIFY them: a row that was left out cannot beat the k-th kept one once
 * the measured rounding of the two conversions (max over the stored rows of |b - b16|, per query |q - q16|; triangle inequality for
 * L2, Cauchy-Schwarz for IP) and the accumulation error are allowed for.  Queries that fail the certificate get a second pass over the
 * fp16 rows at twice the width, and what fails that too is re-run on the fp32
 * lists: by zvec_hip_ivf_search itself (host pointers), or — device pointers, where the search call only enqueues — by
 * zvec_hip_ivf_shadow_certify, which the caller runs on the same context with the same arguments before it reads the results
 * (*rerun = queries that ended on the fp32 lists; a call with no shadow search pending returns 0 at once).  What is pending is the
 * LAST search of the context: a certify call whose count, topk or index differs from that search's is refused (InvalidArgument), and
 * a call on the context that does not go through a twin (a search without one, zvec_hip_flat_search_by_ids, the grouped flat searches,
 * zvec_hip_flat_batch_distance) leaves nothing pending.  Unsupported: fp16 / cosine indexes, rows
 * beyond the half range.  enable = 0 frees the copy.  zvec_hip_ivf_shadow_info: state, bytes held, max |b - b16|, max |b16|.
 * Like zvec_hip_ivf_load, zvec_hip_ivf_set_shadow is an index-level operation: not while searches of the index are in flight.
 * Data the twin cannot serve (rows within the fp16 rounding of each other, a few rows of huge norm under inner product) would pay the
 * fp16 scan AND the fp32 re-run on every search: after four certify steps in a row that re-ran more than half of their queries the
 * next 64 searches of the index read the fp32 rows directly, then the twin is tried again (same results either way). */
/* The same for a flat store (FlatSearcher::search_impl / search_bf_impl, flat_searcher.cc:162-211: every row scored in fp32): an fp16
 * twin of the rows present at the call; searches (no radius, k <= 32, any batch size) pre-select on it, re-score in fp32, certify.  A
 * single query's scan is bound by the bytes of the rows (halved), a wide batch's by the fp32 matrix rate (fp16 instead).  ANY later
 * mutation of the store (append / put / load / reserve) drops the twin; set it again when the rows have settled.  Host-pointer
 * searches certify inside the call, zvec_hip_flat_search_dev is followed by zvec_hip_flat_shadow_certify. */
int zvec_hip_flat_set_shadow(zvec_hip_flat_t h, int enable, uint32_t preselect);
int zvec_hip_flat_shadow_info(zvec_hip_flat_t h, int *enabled, uint64_t *bytes, float *max_row_error, float *max_row_norm);
int zvec_hip_flat_shadow_width(zvec_hip_flat_t h, uint32_t topk, uint32_t *rows);
int zvec_hip_flat_shadow_certify(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk,
                                 const uint64_t *d_exclude_bitset, uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts,
                                 void *stream, uint32_t *rerun);
int zvec_hip_ivf_set_shadow(zvec_hip_ivf_t h, int enable, uint32_t preselect);
int zvec_hip_ivf_shadow_info(zvec_hip_ivf_t h, int *enabled, uint64_t *bytes, float *max_row_error, float *max_row_norm);
/* preselect = 0 leaves the width to the index: it starts at max(32, 3k); six certify steps in a row without a re-run narrow it by 8
 * (a narrower list is cheaper to keep), a step that re-ran more than 1/32 of its queries widens it by 8 and makes the width it failed
 * at the floor from then on; range max(16, 1.5k rounded up to 8) .. 64.  *rows = the width the next search with this k will use
 * (0: no twin). */
int zvec_hip_ivf_shadow_width(zvec_hip_ivf_t h, uint32_t topk, uint32_t *rows);
int zvec_hip_ivf_shadow_certify(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk,
                                uint32_t nprobe, uint32_t max_scan_count, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                                float *d_out_scores, uint32_t *d_out_counts, void *stream, uint32_t *rerun);
/* IVFSearcher::search_bf_impl: every list in list-id order (ivf_entity.cc:719-745). */
int zvec_hip_ivf_search_bf(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *queries,
                           uint32_t count, uint32_t topk, float threshold,
                           const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                           uint32_t *out_counts);
/* shard: keep only the lists this shard owns (centroids stay replicated), the multi-GPU partition of
 * SURVEY §8(e) ("whole inverted lists assigned to GPUs, balanced by bytes").  The list -> shard map is the greedy
 * largest-first assignment of zvec_hip_ivf_shard_map over the GLOBAL list sizes, so every rank derives the same map
 * without communicating.  Call before load / build / begin_lists. */
int zvec_hip_ivf_keep_shard(zvec_hip_ivf_t h, uint32_t shard, uint32_t nshards);
/* the map itself (pure host arithmetic, no GPU needed): lists ordered by (128-row tiles desc, id asc), each given to the
 * shard holding the fewest tiles so far (lowest shard on ties).  owner_out[nlist]; shard_rows_out[nshards] nullable. */
int zvec_hip_ivf_shard_map(const uint32_t *list_sizes, uint32_t nlist, uint32_t nshards, uint32_t *owner_out,
                           uint64_t *shard_rows_out);
/* owner of every list of a loaded / filling index (owner_out[nlist]) */
int zvec_hip_ivf_list_owners(zvec_hip_ivf_t h, uint32_t *owner_out);

/* ---- streamed IVF build ---------------------------------------------------------------------
 * IVFBuilder's three phases as separate calls, so that a (sharded) index far larger than one chunk of raw rows can be
 * built without ever holding the corpus: train (ivf_builder.cc:212-267) on a sample; label chunks of rows with their
 * nearest centroid (ivf_builder.h:253-274, ivf_builder.cc:607-650); announce the global list sizes, then hand the chunks
 * over again with their labels — rows of lists this shard owns are appended to those lists in arrival order (the
 * dump step, ivf_builder.cc:652-729 / ivf_dumper.h:33-160).  zvec_hip_ivf_build[_dev] is exactly
 * train(strided sample) + label(all) + begin + add(all) + end. */
int zvec_hip_ivf_train_dev(zvec_hip_ivf_t h, const void *d_sample, uint64_t n_sample, uint32_t nlist,
                           uint32_t kmeans_iters, uint64_t seed, void *stream);
/* centroids trained elsewhere (e.g. broadcast from rank 0): [nlist][dim] host rows of the index element type */
int zvec_hip_ivf_set_centroids(zvec_hip_ivf_t h, const void *centroids, uint32_t nlist);
int zvec_hip_ivf_get_centroids(zvec_hip_ivf_t h, void *centroids, uint32_t *nlist);   /* either pointer nullable */
/* d_labels[i] = id of the centroid nearest to d_rows[i] under the index metric (DEVICE array, n entries);
 * returns after the labels are complete.  NoTrained (-205) before train / set_centroids / load. */
int zvec_hip_ivf_label_dev(zvec_hip_ivf_t h, const void *d_rows, uint64_t n, uint32_t *d_labels, void *stream);
/* list_sizes[nlist]: GLOBAL row count of every list (all shards).  Allocates the lists this shard owns. */
int zvec_hip_ivf_begin_lists(zvec_hip_ivf_t h, const uint32_t *list_sizes);
/* labels / keys: HOST arrays for the n rows of this call (keys NULL -> key = first_row + i); first_row = global row
 * number of d_rows[0] (what zvec_hip_ivf_export reports as row_ids).  InvalidArgument if a list overflows its
 * announced size. */
int zvec_hip_ivf_add_dev(zvec_hip_ivf_t h, const void *d_rows, uint64_t n, const uint32_t *labels,
                         const uint64_t *keys, uint64_t first_row, void *stream);
/* NoReady (-21) while any owned list is short of its announced size; the index is searchable afterwards */
int zvec_hip_ivf_end_lists(zvec_hip_ivf_t h);
/* per-query statistics of the last search on ctx (IndexContext::Stats, index_context.h:67-111):
 * scanned[q] = total_scan_count, probes[q] = lists actually probed.  Host arrays, nullable. */
int zvec_hip_ivf_last_stats(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, uint32_t count,
                            uint32_t *scanned, uint32_t *probes);

/* ---- Hamming IVF: binary rows through inverted lists ------------------------------------------
 * The reference's IVF is metric-generic: IVFStreamer::search_impl (src/core/algorithm/ivf/ivf_streamer.cc:183-250) never looks
 * at the data type, IVFCentroidIndex (ivf_centroid_index.cc:273-297) is a flat index over the centroids under the rows' own
 * metric, and the trainer has a binary branch, BinaryKmeansAlgorithm<uint32_t / uint64_t> (src/core/algorithm/cluster/
 * opt_kmeans_cluster.cc:760-851, 1319-1326) over BinaryVectorMean (cluster/vector_mean.h:538-650).  zvec_hip_ivf_* keeps refusing
 * binary rows; this family stands beside it.  Score = (float) popcount(row ^ query).
 *   Probe set: the min(nprobe, nlist) centroids smallest by the pair (distance, centroid index), in that ascending order — the
 *   centroid index's heap admits with a strict `<` (heap.h:103-114), so the centroid seen first wins a tie.
 *   max_scan_count: lists are probed in that order while the running scanned count < max_scan_count; every probed list adds its
 *   whole length (ivf_streamer.cc:223-237), as in zvec_hip_ivf_search.
 *   Result: the topk best rows of the probed lists that are not excluded and score <= threshold, ascending; which of several equal
 *   scores sit at the k-th place, and their order, is unspecified.  topk > 128: ZVEC_HIP_ERR_UNSUPPORTED.
 * Searches take the handle's reader side, load and build the writer side; a context's mutex is taken first. */
/* dtype / dim rules of zvec_hip_flat_create for binary rows: Mismatch (-24) for an fp dtype, InvalidArgument (-31) for a dim that
 * is not a multiple of 32 (BINARY32) / 64 (BINARY64) or above 2^20 (hamming_metric.cc:146-147) */
int zvec_hip_bivf_create(uint32_t dim_bits, int dtype, int device, zvec_hip_bivf_t *out);
int zvec_hip_bivf_destroy(zvec_hip_bivf_t h);
/* as zvec_hip_ivf_load (what IVFSearcher::load reads, ivf_index_format.h:26-60,152-164): centroids [nlist] rows; `rows` in
 * inverted-list order, list l owning positions [list_offsets[l], list_offsets[l+1]); keys per row (NULL -> list-order position) */
int zvec_hip_bivf_load(zvec_hip_bivf_t h, const void *centroids, uint32_t nlist, const uint64_t *list_offsets, const void *rows,
                       const uint64_t *keys);
/* IVFBuilder::train + build (ivf_builder.cc:212-403) with the binary trainer: the initial centroids are nlist distinct rows (a
 * partial Fisher-Yates shuffle of the row numbers driven by splitmix64 seeded with `seed`, draws reduced by `% (n - i)`); each of
 * the kmeans_iters iterations labels every row with its nearest centroid by (distance, index) and replaces every centroid that has
 * members by their bitwise majority — bit i set iff ones_i > (members >> 1), BinaryVectorMean::mean (vector_mean.h:599-613) —;
 * then the rows are labelled once more and packed, inside a list in ascending original row number.  kmeans_iters == 0 leaves the
 * initial rows as centroids.  The same arguments always give the same index.  rows: host, [n] rows; keys: host, NULL -> the
 * original row number.  InvalidArgument unless 0 < nlist <= n. */
int zvec_hip_bivf_build(zvec_hip_bivf_t h, const void *rows, uint64_t n, const uint64_t *keys, uint32_t nlist, uint32_t kmeans_iters,
                        uint64_t seed);
/* the same from DEVICE rows; keys stay a host array.  Returns after the index is complete. */
int zvec_hip_bivf_build_dev(zvec_hip_bivf_t h, const void *d_rows, uint64_t n, const uint64_t *keys, uint32_t nlist,
                            uint32_t kmeans_iters, uint64_t seed, void *stream);
int zvec_hip_bivf_info(zvec_hip_bivf_t h, uint64_t *count, uint32_t *nlist);
/* read back as zvec_hip_ivf_export: centroids [nlist] rows, list_offsets [nlist+1], row_ids [count] = original row number (build) /
 * load-order row (load) of each list-order position; any pointer may be NULL.  NoIndexLoaded (-204) before load / build. */
int zvec_hip_bivf_export(zvec_hip_bivf_t h, void *centroids, uint64_t *list_offsets, uint64_t *row_ids);
/* IVFEntity::get_vector by list-order position (ivf_entity.cc:587-716 addresses rows the same way); NoExist beyond the count */
int zvec_hip_bivf_get_vectors(zvec_hip_bivf_t h, const uint64_t *list_positions, uint64_t n, void *out);
/* IVFStreamer::search_impl (ivf_streamer.cc:183-250) under the rules above.  exclude_bitset is over list-order positions, one bit
 * per position, as in zvec_hip_ivf_search.  NoIndexLoaded (-204) before load / build; InvalidArgument for topk == 0 or nprobe == 0. */
int zvec_hip_bivf_search(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count, uint32_t topk, float threshold,
                         uint32_t nprobe, uint32_t max_scan_count, const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                         uint32_t *out_counts);
int zvec_hip_bivf_search_dev(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk,
                             float threshold, uint32_t nprobe, uint32_t max_scan_count, const uint64_t *d_exclude_bitset,
                             uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* what the last search of this index on ctx probed (IndexContext::Stats, index_context.h:67-111, and the coarse result behind it):
 * probe_idx [count][min(nprobe, nlist)] the probe order, probe_cnt [count] the lists probed under the max-scan rule, scanned
 * [count] their rows.  Host arrays, nullable; waits for the context's stream.  NoReady (-21) without such a search. */
int zvec_hip_bivf_last_probes(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t *probe_idx, uint32_t *probe_cnt,
                              uint32_t *scanned);

/* ---- Hamming IVF fed with fp32: rows kept in list order, candidates re-ranked on them ------------------------
 * The reference's pipeline for a binary index over fp32 documents is BinaryConverter on the rows (src/core/quantizer/
 * binary_converter.cc:25-128) -> IVFBuilder (ivf_builder.cc:212-403) -> BinaryReformer on every query (binary_reformer.cc:46-68) ->
 * IVFStreamer::search_impl (ivf_streamer.cc:183-250); a deployment then re-scores the survivors on the original values.  A
 * ZVEC_HIP_DT_BINARY32 handle of 32 * ceil(dim / 32) bits may own the documents' fp32 rows, row-major [count][dim] in LIST ORDER (row
 * p is the document at list-order position p), and a re-score metric, ZVEC_HIP_METRIC_L2 or ZVEC_HIP_METRIC_IP.  The rows cost
 * dim * 4 bytes per document, 32 times the dim / 8 bytes of its bits.  destroy, and the next load or build of any kind, free them;
 * a handle that never sees these calls is unchanged.  Every entry: Mismatch (-24) for a DT_BINARY64 handle (the converter never
 * emits one, binary_converter.cc:100-102) or another width, Unsupported (-12) for a metric other than L2 / IP, InvalidArgument (-31)
 * for dim == 0 or dim > 2^20. */
/* zvec_hip_binary_encode_dev of the rows (encode_dims = dim: bit i = rows[i] >= bin_threshold), zvec_hip_bivf_build of those bits
 * — the same arguments give the same index as the plain build of the same bits —, and the fp32 rows gathered into list order on
 * the device with the build's packing permutation.  rows: host, [n][dim]; keys: host, NULL -> the original row number.  A refused
 * call leaves the handle as it was; everything the fp32 side needs is allocated before the index is touched, and a failure after
 * that point leaves the handle without an index, as one of zvec_hip_bivf_build does. */
int zvec_hip_bivf_build_fp32(zvec_hip_bivf_t h, const float *rows, uint64_t n, uint32_t dim, int metric, const uint64_t *keys,
                             uint32_t nlist, uint32_t kmeans_iters, uint64_t seed, float bin_threshold);
/* the same from DEVICE rows; keys stay a host array.  Returns after the index is complete. */
int zvec_hip_bivf_build_fp32_dev(zvec_hip_bivf_t h, const float *d_rows, uint64_t n, uint32_t dim, int metric, const uint64_t *keys,
                                 uint32_t nlist, uint32_t kmeans_iters, uint64_t seed, float bin_threshold, void *stream);
/* for a handle filled by zvec_hip_bivf_load or the plain build (what IVFSearcher::load leaves, ivf_index_format.h:26-60): rows is
 * [count][dim], ALREADY in list order (zvec_hip_bivf_export's row_ids maps a build's positions to the original rows), and is copied
 * in; calling it again replaces the rows, and a failed call keeps the old ones.  The bits of the index are NOT re-derived from the
 * rows and NOT checked against them: the caller vouches that row p belongs to the bits at position p.  NoIndexLoaded (-204) before
 * load / build.  The _dev form copies from device memory on `stream` (NULL: the handle's) and returns after the copy. */
int zvec_hip_bivf_attach_rows(zvec_hip_bivf_t h, const float *rows, uint32_t dim, int metric);
int zvec_hip_bivf_attach_rows_dev(zvec_hip_bivf_t h, const float *d_rows, uint32_t dim, int metric, void *stream);
/* the fp32 rows of the listed list-order positions, out: host [n][dim] (IVFEntity::get_vector addresses rows the same way,
 * ivf_entity.cc:587-716); NoExist (-22) beyond the count, NoReady (-21) when the handle holds no rows */
int zvec_hip_bivf_get_rows(zvec_hip_bivf_t h, const uint64_t *list_positions, uint64_t n, float *out);
/* dim (0: no rows), the re-score metric and the bytes of the array; any pointer may be NULL */
int zvec_hip_bivf_rows_info(zvec_hip_bivf_t h, uint32_t *dim, int *metric, uint64_t *bytes);
/* BinaryReformer::transform of every query (binary_reformer.cc:46-68: all `dim` values against bin_threshold, as
 * zvec_hip_flat_search_fp32), then two stages that both stay on the device.
 *   Stage 1: zvec_hip_bivf_search's chain (ivf_streamer.cc:183-250) with kc = min(topk * refine, 128) and no radius; nprobe,
 *   max_scan_count and exclude_bitset (over list-order positions) mean what they mean there.  Its result — list-order positions and
 *   Hamming scores, ascending — stays in the context; which of several equal Hamming scores sit at the kc-th place is unspecified.
 *   Stage 2: every candidate is re-scored on its fp32 row: L2 = the fp32 sum of (q_i - b_i)^2, the difference rounded once, each
 *   step an fma; IP = minus the fp32 sum of q_i * b_i; the order of the sum is the library's, values must be finite.  The topk best
 *   by the pair (fp32 score, rank in stage 1's list) are written ascending — a tie in the fp32 score has one answer given the
 *   candidates — and a document with score > threshold is dropped: the radius applies to the fp32 score only.  out_counts[q] can be
 *   below topk (short probed lists, the radius); ONLY the first out_counts[q] entries of a query's output rows are written.
 * Checked before any output is touched: InvalidArgument (-31) for topk, refine or nprobe == 0; Unsupported (-12) for topk > 128;
 * NoIndexLoaded (-204); NoReady (-21) when the handle holds no rows; Mismatch (-24) when dim differs from the rows'; Unsupported
 * for dim > 16128 — a work-group keeps its query in LDS, and 63 KiB of query plus the 528 bytes of scores behind it is what a
 * launch may take without a raised limit.  Batches are sliced under "bivf_part_bytes" as zvec_hip_bivf_search slices them; a slice
 * runs both stages.  keys come from the handle's key column. */
int zvec_hip_bivf_search_fp32(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const float *queries, uint32_t count, uint32_t dim, uint32_t topk,
                              uint32_t refine, float threshold, float bin_threshold, uint32_t nprobe, uint32_t max_scan_count,
                              const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
int zvec_hip_bivf_search_fp32_dev(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const float *d_queries, uint32_t count, uint32_t dim,
                                  uint32_t topk, uint32_t refine, float threshold, float bin_threshold, uint32_t nprobe,
                                  uint32_t max_scan_count, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                                  float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* stage 1 of the last zvec_hip_bivf_search_fp32[_dev] of this index on ctx, which ran with this kc = min(topk * refine, 128):
 * positions [count][kc] list-order positions ascending by Hamming score, hamming_scores [count][kc], counts [count] the candidates
 * of each query (entries beyond them are unspecified).  Host arrays, nullable; waits for the context's stream.  NoReady (-21)
 * without such a search. */
int zvec_hip_bivf_last_candidates(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t kc, uint32_t *positions,
                                  float *hamming_scores, uint32_t *counts);

/* ---- partial top-k merge ------------------------------------------------------------------
 * CombinedVectorColumnIndexer::Search concat + sort + truncate
 * (src/db/index/column/vector_column/combined_vector_column_indexer.cc:91-232); also the merge
 * after the RCCL all-gather of per-GPU candidate lists.
 * inputs [nparts][count][topk] keys/scores + [nparts][count] counts; ties keep part order. */
int zvec_hip_merge_topk(zvec_hip_ctx_t ctx, const uint64_t *keys, const float *scores,
                        const uint32_t *counts, uint32_t nparts, uint32_t count, uint32_t topk,
                        uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
int zvec_hip_merge_topk_dev(zvec_hip_ctx_t ctx, const uint64_t *d_keys, const float *d_scores,
                            const uint32_t *d_counts, uint32_t nparts, uint32_t count,
                            uint32_t topk, uint64_t *d_out_keys, float *d_out_scores,
                            uint32_t *d_out_counts, void *stream);

/* Packed form for the shard exchange: one buffer per part laid out
 *   [count*topk keys u64][count*topk scores f32][count counts u32]  padded to a multiple of 16 bytes
 * (zvec_hip_packed_bytes), parts `part_stride` bytes apart — exactly what one all-gather of the per-rank
 * buffers produces, so the candidate lists go search -> RCCL -> merge without any repacking kernel.
 * zvec_hip_packed_layout returns the three offsets inside one part. */
uint64_t zvec_hip_packed_bytes(uint32_t count, uint32_t topk);
int zvec_hip_merge_topk_packed_dev(zvec_hip_ctx_t ctx, const void *d_packed, uint64_t part_stride,
                                   uint32_t nparts, uint32_t count, uint32_t topk, uint64_t *d_out_keys,
                                   float *d_out_scores, uint32_t *d_out_counts, void *stream);

/* ---- one index over several GPUs, inside one process ---------------------------------------
 * zvec is a single-process embedded library: the plugin cannot count on a launcher to use the 8 GPUs of a node.  One
 * zvec_hip_shards_t owns G device shards of ONE index and does what CombinedVectorColumnIndexer::Search does over
 * blocks (combined_vector_column_indexer.cc:91-232): fan the batch out, rebase, concatenate in part order, keep the
 * top-k.  Partition: FLAT = contiguous row ranges (every append is cut into G pieces; key = the caller's
 * key or the global storage position), IVF = whole inverted lists dealt by zvec_hip_ivf_shard_map, centroids
 * replicated, probe sets global.  A search runs one worker thread per shard (own device, context and stream); each
 * writes its candidate lists in the packed layout and peer-copies them (xGMI) to devices[0], which merges them with
 * the kernel of zvec_hip_merge_topk_packed_dev.  `devices` may repeat a device (several shards on one GPU).
 * The one-process-per-GPU form of the same partition (RCCL all-gather of the same packed lists) is zvec_amd/dist.py. */
enum { ZVEC_HIP_SHARDS_FLAT = 0, ZVEC_HIP_SHARDS_IVF = 1 };
int zvec_hip_shards_create(uint32_t dim, int dtype, int metric, int kind, const int *devices, uint32_t ndev,
                           zvec_hip_shards_t *out);
int zvec_hip_shards_destroy(zvec_hip_shards_t h);
/* rows held in total / per shard (per_shard[ndev] nullable) */
int zvec_hip_shards_count(zvec_hip_shards_t h, uint64_t *total, uint64_t *per_shard);
/* FLAT: IndexStreamer::add_impl in bulk (index_runner.h:476-487); keys NULL -> key = global storage position */
int zvec_hip_shards_flat_append(zvec_hip_shards_t h, const void *vecs, uint64_t n, const uint64_t *keys);
/* IVF: IVFBuilder::train + build over the shards (ivf_builder.cc:212-403): k-means on devices[0], labels computed in
 * G pieces, every shard fills the lists it owns.  Same sample / seed rule as zvec_hip_ivf_build, hence the same
 * centroids and lists as an unsharded build. */
int zvec_hip_shards_ivf_build(zvec_hip_shards_t h, const void *vecs, uint64_t n, const uint64_t *keys, uint32_t nlist,
                              uint32_t kmeans_iters, uint32_t sample_per_list, uint64_t seed);
/* IVF: IVFSearcher::load of host arrays (see zvec_hip_ivf_load); every shard keeps its lists */
int zvec_hip_shards_ivf_load(zvec_hip_shards_t h, const void *centroids, uint32_t nlist, const uint64_t *list_offsets,
                             const void *vecs, const uint64_t *keys);
/* the segment-payload loaders over the shards (same arguments as zvec_hip_ivf_load_segments /
 * zvec_hip_flat_load_features): what the plugin's load() / open() call when it is configured with several devices */
int zvec_hip_shards_ivf_load_segments(zvec_hip_shards_t h, const void *inverted_header, uint64_t header_bytes,
                                      const void *inverted_meta, uint64_t meta_bytes, const void *inverted_body,
                                      uint64_t body_bytes, const void *keys, uint64_t keys_bytes, const void *centroids);
int zvec_hip_shards_flat_load_features(zvec_hip_shards_t h, const void *features, uint64_t bytes, uint64_t count,
                                       int column_major, uint32_t batch_size, const uint64_t *keys);
/* FLAT: search_bf_by_p_keys_impl and the fetch_vector gather over the shards; ids / positions are GLOBAL storage
 * positions (append order), unknown ids are skipped / NO_EXIST like the single-device entries */
int zvec_hip_shards_flat_search_by_ids(zvec_hip_shards_t h, const void *queries, uint32_t count, const uint64_t *ids,
                                       const uint32_t *offsets, uint32_t topk, float threshold, const uint64_t *exclude_bitset,
                                       uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
int zvec_hip_shards_flat_get_vectors(zvec_hip_shards_t h, const uint64_t *positions, uint64_t n, void *out);
/* IVF: deal the coarse pass over the shards (off by default): shard g scores its 1/G of the batch against its replica of the
 * centroids and peer-copies that slice of the probe lists into every shard's table (xGMI, Q x (nprobe + 1) x 4 bytes in all),
 * every shard then plans from the table (zvec_hip_ivf_coarse_dev / zvec_hip_ivf_search_probes_dev).  Same results. */
int zvec_hip_shards_deal_coarse(zvec_hip_shards_t h, int enable);
/* search_impl(query, qmeta, count, ctx) over the shards; host pointers; FLAT ignores nprobe / max_scan_count.
 * exclude_bitset: 1 bit per GLOBAL storage position (FLAT: append order; IVF: list-order positions of the whole
 * index), sliced per shard on the host.  Results: the global top-k, as from one unsharded index. */
int zvec_hip_shards_search(zvec_hip_shards_t h, const void *queries, uint32_t count, uint32_t topk, float threshold,
                           uint32_t nprobe, uint32_t max_scan_count, const uint64_t *exclude_bitset,
                           uint64_t *out_keys, float *out_scores, uint32_t *out_counts);

/* ---- measurement hook ---------------------------------------------------------------------
 * Records HIP events around the dominant scan kernel of each search on ctx (on the stream the
 * kernel is launched on) and returns the accumulated launch count / milliseconds since the last
 * reset.  Used by bench.py for the roofline line. */
int zvec_hip_ctx_profile(zvec_hip_ctx_t ctx, int enable);
int zvec_hip_ctx_profile_read(zvec_hip_ctx_t ctx, uint64_t *launches, double *scan_ms,
                              double *algorithmic_bytes, double *algorithmic_flops, int reset);
/* Which route the last flat search on ctx took (zvec_hip_flat_search / _search_dev over fp rows): the profile above names a
 * launch by its duration only, this names it by what the host dispatched.  Cleared when such a search starts; a search that
 * went in slices ORs them.  Host bookkeeping, no device call.  Defined only straight after such a search: every other
 * search kind on the context (IVF, whose coarse pass is a flat scan; k-means labelling; group-by, by-ids, Hamming and
 * sparse searches) leaves the word undefined — they may OR bits into it and never clear it.
 *   bits 0..8    shape of the main scan: 0 dense-score path, 1 / 2 / 3 the 4-wave tile with 1 / 2 / 4 query groups, 4 the 16-row
 *                shape, 5 the 8-wave 128 x 128 tile, 6 the 256 x 256 fp16 tile, 7 the gathering 8-wave tile (sparse keep-set),
 *                8 the kept rows were copied to a compacted store first (the scan of the copy sets its own shape bit as well)
 *   bit 9        the main scan ran its exclusion variant
 *   bits 10..11  seeding of the shared admission bounds: 0 none, 1 the k-th of 256 minima of a dense prefix dump, 2 the k-th score
 *                of a prefix scan with lists
 *   bits 16..25  seeding 2 only: bits 0..9 of the prefix scan itself */
int zvec_hip_ctx_last_route(zvec_hip_ctx_t ctx, uint32_t *route);

/* The plan of the last IVF search on ctx (zvec_hip_ivf_search / _search_bf / _search_dev / _search_probes_dev): which route the host
 * dispatched and, for the tile route, the arrays the plan kernels left for the list scan — the only view of them that does not go
 * through the final top-k.  A test and debugging hook: the searches themselves only remember a few host words (no launch, copy or
 * wait is added to them); this call waits for the context's stream and copies the plan buffer out once.  A search that was handed a
 * caller's stream must have been waited for by the caller.
 *   info      always filled: route, and for the tile route every scalar below
 *   arrays    each may be NULL; filled for the tile route only: q_nprobe, q_scanned, q_nslots [nq], slot_begin [nq + 1],
 *             list_count, list_tpc [nlist], list_qoff, item_off [nlist + 1] (item_off in the deal order: lists largest first),
 *             csr_q, csr_slot [csr_len <= nq x nprobe] (list-major; the order inside a list is not defined)
 * Returns 0 for the tile route, ZVEC_HIP_ERR_NO_READY ("nothing to report", info->route says why) when the last search took the
 * direct or the large-k route, was cut short by an error, or was not an IVF search (a flat, group-by or by-ids search on the
 * context in between; other search kinds leave the plan of the last IVF search readable). */
#define ZVEC_HIP_IVF_ROUTE_NONE 0u
#define ZVEC_HIP_IVF_ROUTE_DIRECT_BLOCK_TOPK 1u /* a few queries, wave per row: the scoring blocks keep their own top-k lists */
#define ZVEC_HIP_IVF_ROUTE_DIRECT_SELECT 2u     /* a few queries, wave per row: score matrix, selected in one run or two steps */
#define ZVEC_HIP_IVF_ROUTE_TILE 3u              /* list-major work items on the matrix tile */
#define ZVEC_HIP_IVF_ROUTE_LARGE_K 4u           /* k beyond the scan's resident lists: expanded positions, scored pair by pair */
typedef struct zvec_hip_ivf_plan_info {
  uint32_t route;          /* ZVEC_HIP_IVF_ROUTE_* */
  uint32_t scan_threads;   /* threads of the plan's single-group scan kernel: 1024 on the context's own stream, 256 beside another lane */
  uint32_t nq, nlist;
  uint32_t nprobe;         /* probe ranks per query (nlist under brute force) */
  uint32_t brute_force;
  uint32_t tpc;            /* base tiles per chunk of this search (a list's own: list_tpc) */
  uint32_t rows_per_group; /* query rows of one work item */
  uint32_t total_items;
  uint32_t csr_len;        /* = list_qoff[nlist] */
  uint64_t slots_bound;    /* result slots the host sized the partial lists for; >= slot_begin[nq] */
} zvec_hip_ivf_plan_info;
int zvec_hip_ctx_last_ivf_plan(zvec_hip_ctx_t ctx, zvec_hip_ivf_plan_info *info, uint32_t *q_nprobe, uint32_t *q_scanned,
                               uint32_t *q_nslots, uint32_t *slot_begin, uint32_t *list_count, uint32_t *list_qoff,
                               uint32_t *item_off, uint32_t *list_tpc, uint32_t *csr_q, uint32_t *csr_slot);

/* Per-box calibration for the measurement line (bench.py `roofline.box_clock_mhz` / `box_stream_gbs`): what this box's HBM delivers
 * to a pure streaming reader (16-byte non-temporal loads over `bytes` of device memory: d_buf, or a scratch allocation when NULL),
 * best of `reps` launches, and the shader clock held under that load (s_memtime against the constant 100 MHz s_memrealtime).  So a
 * reader can tell a slow box from slow code: the list scan of SURVEY §8(d) streams the index the same way. */
int zvec_hip_calibrate(int device, const void *d_buf, uint64_t bytes, uint32_t reps, double *clock_mhz, double *stream_gbs);

/* FlatSearcher::load of the features segment of a dumped flat index (FlatBuilder<32>::write_row_index /
 * write_column_index, src/core/algorithm/flat/flat_builder.cc:186-276): `count` rows of the handle's element type —
 * row-major, or (column_major != 0) full `batch_size`-row blocks transposed in units of the element type followed by
 * a row-major remainder.  keys: the "flat.keys" payload (uint64[count]) or NULL (key = position).  Appends. */
int zvec_hip_flat_load_features(zvec_hip_flat_t h, const void *features, uint64_t bytes, uint64_t count, int column_major,
                                uint32_t batch_size, const uint64_t *keys);

/* The centroid index in a space of its own.  IVFBuilder trains INNER-PRODUCT indexes through a MipsConverter
 * (src/core/algorithm/ivf/ivf_builder.cc:552-555): the nested "ivf.centroid" index of such a file holds converted centroids — more
 * dimensions, squared-Euclidean metric, a MipsReformer named in its meta — and IVFCentroidIndex::search reforms every query before
 * the coarse scan (ivf_centroid_index.cc:273-297), while the inverted lists keep the original rows and metric.
 * zvec_hip_ivf_load_segments may then be given centroids = NULL; zvec_hip_ivf_set_coarse_space installs the converted centroid
 * rows (nlist x coarse_dim elements of the index's element type, centroid-id order; coarse_metric L2 or IP) and searches go
 * through zvec_hip_ivf_search_coarse, which takes the reformed queries ([count][coarse_dim]) beside the original ones
 * (zvec_hip_ivf_search_bf needs neither).  IVFSearcher::search_impl otherwise, ivf_searcher.cc:183-250. */
int zvec_hip_ivf_set_coarse_space(zvec_hip_ivf_t h, uint32_t coarse_dim, int coarse_metric, const void *centroids, uint32_t nlist);
int zvec_hip_ivf_search_coarse(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const void *queries, const void *coarse_queries, uint32_t count,
                               uint32_t topk, float threshold, uint32_t nprobe, uint32_t max_scan_count,
                               const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores, uint32_t *out_counts);

/* HipFlatStreamer::open over a storage the reference's FlatStreamer has written (FlatStreamerEntity, flat_streamer_entity.cc:43-47,
 * flat_streamer_entity.h:287-311, BlockHeader / DeletionMap flat_index_format.h:91-126): `blocks` = a run of `nblocks` blocks of
 * `block_size` bytes as they lie in a "flat.features<i>" segment — [block_vector_count x element][block_vector_count x u64 key]
 * ... [DeletionMap][BlockHeader] — and keep[b] = the live rows of block b (bit r: r < vector_count, not deleted, key valid).
 * One strided copy + one launch per run instead of a provider walk row by row.  Appends, in block / row order.
 * `bytes` = the extent of `blocks` the caller vouches for: InvalidArgument when nblocks x block_size does not fit in it or a block
 * is too small for its rows, keys and 16 tail bytes. */
int zvec_hip_flat_load_blocks(zvec_hip_flat_t h, const void *blocks, uint64_t bytes, uint64_t nblocks, uint32_t block_size,
                              uint32_t block_vector_count, const uint32_t *keep);

/* IVFSearcher::load from the raw payloads of the segments a dumped reference index holds (SURVEY next-2):
 *   inverted_header  "ivf.inverted_header": InvertedIndexHeader (ivf_index_format.h:26-37) + the serialised IndexMeta
 *                    (IndexMetaFormatHeader, src/core/framework/index_meta.cc:23-34: major order, data type, dimension)
 *   inverted_meta    "ivf.inverted_meta":   InvertedListMeta[inverted_list_count] (ivf_index_format.h:41-47)
 *   inverted_body    "ivf.inverted_body":   32-vector blocks per list as IVFDumper writes them (ivf_dumper.cc:19-81,
 *                    388-406): full blocks of a column-major index transposed, everything else row-major
 *   keys             "hc.keys":             uint64[total_vector_count] in dump (= list) order
 *   centroids        [inverted_list_count][dim] rows of the index element type (the features of the nested centroid
 *                    index "ivf.centroid", which the caller's storage layer opens)
 * The plugin obtains these blobs from zvec's own IndexStorage (segment->read), exactly as IVFSearcher::load does; the
 * body is uploaded as it is and re-laid out on the GPU.  Mismatch (-24) when data type / dimension differ from the
 * handle's, InvalidArgument for inconsistent sizes or offsets.  Parity: checked against index files dumped by
 * the reference's own IVFDumper / FlatBuilder / MemoryDumper compiled in place (tests/golden/ref_index_files.npz). */
int zvec_hip_ivf_load_segments(zvec_hip_ivf_t h, const void *inverted_header, uint64_t header_bytes,
                               const void *inverted_meta, uint64_t meta_bytes, const void *inverted_body,
                               uint64_t body_bytes, const void *keys, uint64_t keys_bytes, const void *centroids);

/* The container framing of a dumped index FILE (IndexFormat, src/include/zvec/core/framework/index_format.h:26-95;
 * IndexUnpacker::unpack, index_unpacker.h:103-330): [MetaHeader][segments' data][segment metas + ids][MetaFooter],
 * possibly chained.  Lists the segments of a whole file image — id, byte offset in the image, size — so that a caller
 * holding only the file can hand "flat.features" / "flat.keys" / "ivf.*" / "hc.keys" to the loaders above (the plugin
 * gets them from zvec's IndexStorage instead).  Header / footer / meta CRCs (crc32c) are always checked, the content CRC
 * when checksum != 0.  Host-only code.  out may be NULL with cap 0 to count; OutOfRange (-17) when cap is too small
 * (count is still set), Mismatch (-24) for a bad size field or checksum, InvalidArgument for inconsistent offsets. */
typedef struct {
  char id[64];
  uint64_t offset, size, padding;
  uint32_t crc, reserved_;
} zvec_hip_segment_t;
int zvec_hip_container_segments(const void *image, uint64_t bytes, int checksum, zvec_hip_segment_t *out, uint32_t cap,
                                uint32_t *count);

/* Query reformers on the device, for callers that keep raw fp32 query batches in HBM:
 *   cosine != 0: CosineReformer::transform (src/core/quantizer/cosine_reformer.cc:66-112) — q/||q|| followed by ||q||
 *                (out rows: dim+1 floats, or dim+2 halves with the norm's bytes in the last two slots);
 *   out_dtype == ZVEC_HIP_DT_FP16: HalfFloatReformer (round to nearest even).
 * d_in: [count][dim] fp32, d_out: device buffer of count rows of the output width.  Bit-identical to the reference's
 * AVX-512 host code (norm summation order, correctly rounded sqrt / divide). */
int zvec_hip_reform_queries_dev(zvec_hip_ctx_t ctx, const float *d_in, uint32_t count, uint32_t dim, int cosine,
                                int out_dtype, void *d_out, void *stream);

/* ---- fp32 -> sign bits (binary quantisation) ------------------------------------------------------------------
 * BinaryConverter on the rows of an index (src/core/quantizer/binary_converter.cc:25-128, :138-167) and BinaryReformer on every
 * query (src/core/quantizer/binary_reformer.cc:46-68), on the device.  Both run ailego::BinaryQuantizer::encode
 * (src/ailego/algorithm/binary_quantizer.cc:40-57): bit j of word w is in[32 w + j] >= threshold, LSB first; the threshold is the
 * quantizer's (binary_quantizer.h:48-55, 0 unless set; BinaryQuantizer::train does nothing, binary_quantizer.cc:35-37).
 *   d_in / in: [count][dim] fp32, rows at their natural 4-byte alignment; d_out / out: [count][ceil(dim / 32)] uint32_t, row-major —
 *   a DT_BINARY32 row of 32 * ceil(dim / 32) bits (BinaryConverterHolder::dimension, binary_converter.cc:93-102).
 *   Bit i of a row is in[i] >= threshold for i < encode_dims and 0 for every other bit of the row's words: encode(in, encode_dims,
 *   out) written into a zeroed row.  The comparison is the C one: -0.0f >= 0.0f holds, nan gives 0, +inf 1, -inf 0, a denormal
 *   compares by its value.  1 <= encode_dims <= dim <= 2^20.
 *   encode_dims exists because the reference's two sides disagree: BinaryConverterHolder::Iterator::encode_record calls
 *   encode(vec, dim_ / 2, ...) with dim_ the PADDED bit count 32 * ceil(dim / 32) (binary_converter.cc:34-39, :69-73), so the rows
 *   it converts carry bits for the first 32 * ceil(dim / 32) / 2 input values only, while its reformer encodes all `dim` values of a
 *   query (binary_reformer.cc:62).  encode_dims = dim is what the names promise; encode_dims = 32 * ceil(dim / 32) / 2 reproduces
 *   the reference's converted rows.  (BinaryReformer's batch form, binary_reformer.cc:71-92, encodes the count * dim values as ONE
 *   run, which equals the per-query form only when dim is a multiple of 32; the per-query form is the one served here.)
 * zvec_hip_binary_encode_dev only enqueues work on `stream` (NULL: the context's).  zvec_hip_binary_encode is the same through host
 * pointers, staged through the device in bounded slices.  count == 0 returns 0 and writes nothing; a NULL context or pointer,
 * dim == 0, dim > 2^20 or encode_dims outside [1, dim] is ZVEC_HIP_ERR_INVALID_ARGUMENT and touches no output. */
int zvec_hip_binary_encode_dev(zvec_hip_ctx_t ctx, const float *d_in, uint64_t count, uint32_t dim, uint32_t encode_dims,
                               float threshold, uint32_t *d_out, void *stream);
int zvec_hip_binary_encode(zvec_hip_ctx_t ctx, const float *in, uint64_t count, uint32_t dim, uint32_t encode_dims,
                           float threshold, uint32_t *out);
/* IndexConverter::transform + IndexBuilder::build of a "BinaryConverter" index (binary_converter.cc:185-196; flat_builder.cc:188-276),
 * IndexStreamer::add_impl behind the converter: n fp32 rows of `dim` values are encoded on the device (encode_dims, threshold as
 * above) and stored exactly as zvec_hip_flat_append[_dev] stores the same words — positions, keys (NULL: key = position), all of
 * the rows or none.  The handle must be ZVEC_HIP_DT_BINARY32 with 32 * ceil(dim / 32) bits; every other handle (DT_BINARY64, which
 * the converter never emits, binary_converter.cc:100-102; the fp types; another width) is ZVEC_HIP_ERR_MISMATCH.  n == 0 returns 0. */
int zvec_hip_flat_append_fp32(zvec_hip_flat_t h, const float *vecs, uint64_t n, uint32_t dim, uint32_t encode_dims,
                              float threshold, const uint64_t *keys);
int zvec_hip_flat_append_fp32_dev(zvec_hip_flat_t h, const float *d_vecs, uint64_t n, uint32_t dim, uint32_t encode_dims,
                                  float threshold, const uint64_t *d_keys, void *stream);
/* BinaryReformer::transform of every query (binary_reformer.cc:46-68: all `dim` values encoded, against bin_threshold) followed by
 * zvec_hip_flat_search[_dev] (search_impl, index_runner.h:490-531): outputs, ties, threshold, exclude_bitset and the topk cap are
 * those calls'.  queries: [count][dim] fp32.  The handle pairs with `dim` as for zvec_hip_flat_append_fp32.  The encoded queries
 * live in the context's workspace: the device-pointer form allocates nothing once the workspace has grown to the batch. */
int zvec_hip_flat_search_fp32(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const float *queries, uint32_t dim, float bin_threshold,
                              uint32_t count, uint32_t topk, float threshold, const uint64_t *exclude_bitset,
                              uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
int zvec_hip_flat_search_fp32_dev(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const float *d_queries, uint32_t dim,
                                  float bin_threshold, uint32_t count, uint32_t topk, float threshold,
                                  const uint64_t *d_exclude_bitset, uint64_t *d_out_keys, float *d_out_scores,
                                  uint32_t *d_out_counts, void *stream);

/* ---- predicate materialisation --------------------------------------------------------
 * Replaces the per-candidate IndexFilter callback (index_filter.h:48-50) whose producers are
 * DocFilter::is_filtered (src/db/sqlengine/planner/doc_filter.cc:74-87), DeleteStore::Filter
 * (src/db/index/common/delete_store.h:61-72) and InvertedSearchResult::Filter
 * (src/db/index/column/inverted_column/inverted_search_result.h:34-50):
 *     excluded(id) = deleted.contains(id) || !invert_result.contains((uint32_t)id) || !forward_bool[id]
 * evaluated once per storage position of the index (id = the key stored at that position) into the
 * 1-bit-per-position exclude bitset the search entry points take.  Each term is optional.
 *   delete_kind  ZVEC_HIP_ROARING_NONE / _32 (roaring_bitmap_portable_serialize, CRoaring 2.0.4) / _64MAP
 *                (roaring::Roaring64Map::write) / _FILE (a delete-store file image: the 64-byte BitmapMetaHeader
 *                of concurrent_roaring_bitmap.h:186-192 — magic, is_32bit, crc32c — followed by the payload)
 *   invert       32-bit portable roaring (the inverted-index result set: ids that MATCH), or NULL
 *   forward_bits Arrow boolean buffer, LSB first, forward_len bits (ids beyond it are not excluded, doc_filter.cc:104)
 * A 32-bit delete bitmap is probed with (uint32_t)id, like ConcurrentRoaringBitmap64::contains (:196-203).
 * Pointers in the descriptor are HOST memory; out_words is (count+63)/64 uint64 on the device (out_on_device != 0)
 * or on the host.  Returns InvalidArgument for a malformed stream, Mismatch (-24) for a bad magic / checksum. */
enum { ZVEC_HIP_ROARING_NONE = 0, ZVEC_HIP_ROARING_32 = 1, ZVEC_HIP_ROARING_64MAP = 2, ZVEC_HIP_ROARING_FILE = 3 };
typedef struct {
  const void *delete_bitmap;
  uint64_t delete_bytes;
  int32_t delete_kind;
  int32_t reserved_;
  const void *invert_bitmap;
  uint64_t invert_bytes;
  const uint8_t *forward_bits;
  uint64_t forward_len;
} zvec_hip_doc_filter_t;
int zvec_hip_flat_build_filter(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const zvec_hip_doc_filter_t *filter,
                               uint64_t *out_words, int out_on_device, void *stream);
/* positions are list-order positions, as for zvec_hip_ivf_search's exclude_bitset */
int zvec_hip_ivf_build_filter(zvec_hip_ivf_t h, zvec_hip_ctx_t ctx, const zvec_hip_doc_filter_t *filter,
                              uint64_t *out_words, int out_on_device, void *stream);
/* ailego::Crc32c::Hash (src/ailego/hash/crc32c.cc:626-634): raw CRC-32C update, no pre/post inversion */
uint32_t zvec_hip_crc32c(const void *data, uint64_t len, uint32_t crc);

/* ---- flat index of sparse rows ---------------------------------------------------------------
 * stands behind FlatSparseStreamer / FlatSparseSearcher (src/core/algorithm/flat_sparse/flat_sparse_streamer.cc:186-300,
 * flat_sparse_search.h:58-148) for fp32 and fp16 values under one of two metrics, fixed when the handle is created
 * (zvec_hip_sparse_create_metric):
 *   ZVEC_HIP_METRIC_IP  "InnerProductSparse" (inner_product_metric.cc:329, 484-495: MinusInnerProductSparseMatrix<float>::Compute
 *                       for DT_FP32, <ailego::Float16> for DT_FP16); what zvec_hip_sparse_create and _create_typed give
 *   ZVEC_HIP_METRIC_L2  "SquaredEuclideanSparse" (SquaredEuclideanSparseMetric, src/core/metric/euclidean_metric.cc:1027-1095;
 *                       SquaredEuclideanSparseDistanceMatrix<float>::Compute, src/ailego/math/euclidean_distance_matrix.h:
 *                       2480-2638).  The reference's metric accepts DT_FP16 but hands out the <float> routine for it
 *                       (euclidean_metric.cc:1070-1072), so there is no fp16 summation of its own to match: the definition
 *                       under "Score" below is the contract for both value types.
 * Value type, row format, index order, the 4096-pair cap, validation of host queries, exclude_bitset, threshold, the topk caps,
 * the rules for listed rows and the group-by ranking rules are the same under both metrics; scores are smaller-is-better and
 * lists ascend under both.  Rules, as the reference has them:
 *   - Value type.  A handle serves ONE value type, chosen at zvec_hip_sparse_create_typed: ZVEC_HIP_DT_FP32 (float) or
 *     ZVEC_HIP_DT_FP16 (IEEE binary16, 2 bytes).  Every `values` pointer below (rows, queries, get_vector, host or device) is a
 *     `const void *` / `void *` read as elements of the handle's type, the way zvec_hip_flat_* treats `vecs`.  fp16 values are
 *     stored as halves (never widened in memory); each is widened to fp32 where it is read, which is exact (subnormals included),
 *     and the products are formed and summed in fp32, as the reference does on an AVX host (InnerProductSparseInSegmentAVX,
 *     src/ailego/math/inner_product_matrix_fp16.cc:1066-1226: the matched halves go through _mm256_cvtph_ps into an fp32
 *     accumulator, :1208-1223).  No half-precision arithmetic.  Scores are fp32 for either type.  Values must be finite: inf and
 *     NaN give unspecified scores.
 *   - Row format.  A row, and a query, is `count` pairs (uint32_t index, value), count <= 4096
 *     (PARAM_FLAT_SPARSE_MAX_DIM_SIZE, flat_sparse_utility.h:22).  The reference discards a longer row
 *     (flat_sparse_streamer.cc:197-201); here zvec_hip_sparse_append returns ZVEC_HIP_ERR_INVALID_ARGUMENT for it and stores
 *     NOTHING of the call; a longer query is refused the same way.  count == 0 is a legal row and a legal query.
 *     A batch is CSR-like: counts[n], then the runs back to back in indices[] / values[].
 *   - Index order.  The indices of a run must be STRICTLY ascending.  The reference neither sorts nor checks:
 *     transform_sparse_format (src/ailego/math/inner_product_matrix.h:2891-2968; SparseUtility::TransSparseFormat,
 *     src/core/utility/sparse_utility.h:272-350) cuts a run into 16-bit segments as it comes (a segment id that goes backwards
 *     falls into the "// std::abort()" branch, :2926-2928, and is counted into the wrong segment) and the scoring routines
 *     (Compute, :2838-2859, and ComputeInnerProductSparseInSegment, :2866-2888) are merge joins that advance both sides on a
 *     match: an unsorted or repeated index gives the reference an unspecified score.  Such a run is refused here:
 *     ZVEC_HIP_ERR_INVALID_ARGUMENT from append and from the host-pointer search.  zvec_hip_sparse_search_dev cannot see its
 *     queries' indices: runs that break the rule give unspecified scores there (never an out-of-range access).
 *   - Score, ZVEC_HIP_METRIC_IP.  MINUS the inner product over the indices present in both row and query (Compute ends with
 *     *out = -sum, :2861), smaller is better, lists ascending: the convention of ZVEC_HIP_METRIC_IP on a dense flat handle.  A
 *     pair without a shared index (an empty row or query included, :2795-2799) scores exactly 0 and is an ordinary candidate,
 *     as in the reference's heap.  Products are summed in fp32, in an order of the library's choosing.
 *   - Score, ZVEC_HIP_METRIC_L2.  The squared distance over the UNION of the two index sets: an index present in both adds
 *     (b - q)^2, one of the row alone b^2, one of the query alone q^2.  Scores are >= 0, never -0 and never negative.  The
 *     score of row b against query q is s = A + R, all in fp32, halves widened exactly first:
 *       A  summed over the stored elements of the row, in an order of the library's choosing, each step an fma, every term
 *          non-negative: an element whose index is in the query's run adds (b - q)^2, the difference rounded once; any other
 *          element adds b^2.
 *       R  the query mass that matched nothing.  If every query element was matched (hits == qlen, counted while A is formed;
 *          the empty query included) R is exactly +0.  Otherwise R = max(0, Qn - Mq), Qn the fp32 sum of q^2 over the whole
 *          run (formed once per query per launch or work item, never per row), Mq the fp32 sum of q^2 over the matched ones.
 *     So a row searched with itself, and any identical pair, scores exactly +0.0; a pair of empty runs scores exactly +0.0; an
 *     empty row scores Qn and an empty query the row's sum of squares; a pair with no shared index scores |b|^2 + |q|^2 and
 *     is an ordinary candidate, no zero tie.  (The expansion |b|^2 + |q|^2 - 2 b.q is NOT used: it cancels exactly where a
 *     nearest-neighbour search looks and cannot return 0 for a row searched with itself.)  For fp32 values this is the
 *     reference's quantity in another order of summation (theirs is sequential inside 16-bit index segments); it agrees with
 *     the exact value within (rlen + 4) * 2^-23 * A + [hits < qlen] * (qlen + 4) * 2^-23 * (Qn + Mq), not bit for bit.
 *   - threshold and exclude_bitset mean what they mean for zvec_hip_flat_search (a document is dropped iff score > threshold;
 *     bit i of word i / 64 = storage position i, the row's number in append order).
 *   - Ties.  Which of several equal scores are returned at the k-th place, and their order, is unspecified (the reference's
 *     heap resolves ties arbitrarily).  Under ZVEC_HIP_METRIC_IP zero scores tie massively; under ZVEC_HIP_METRIC_L2 a zero
 *     score means identical runs and ties are as rare as equal distances.
 *   - topk * 12 + 16 <= 60 KiB as elsewhere, else ZVEC_HIP_ERR_UNSUPPORTED.
 *   - Listed rows (zvec_hip_sparse_search_by_ids, zvec_hip_sparse_batch_distance).  `ids` / `positions` are STORAGE POSITIONS:
 *     the caller maps primary keys to positions and drops unknown keys, as get_id(p_key) == kInvalidNodeId does in the reference
 *     (flat_sparse_entity.h:67-70).  A position >= the row count is never dereferenced; search_by_ids never returns it and
 *     batch_distance scores it +inf.  A position listed twice for a query is scored twice and may be returned twice (the
 *     reference's heap takes both emplace calls).  exclude_bitset, threshold, ties and the topk cap mean what they mean for
 *     zvec_hip_sparse_search; equal scores come in the order of the list.  out_counts[q] can be below topk simply because the
 *     list was short; an empty list gives 0.  Host queries are validated as in zvec_hip_sparse_search.  offsets that descend,
 *     offsets[0] != 0, a NULL where none is allowed and topk == 0 return ZVEC_HIP_ERR_INVALID_ARGUMENT and touch no output.
 *   - Group-by (zvec_hip_sparse_search_grouped, zvec_hip_sparse_search_grouped_by_ids): FlatSparseEntity::search_group and
 *     search_group_p_keys (flat_sparse_entity.h:79-128), ranked and assembled as ConvertGroupMapToResult does
 *     (flat_sparse_search.h:23-53; the dispatch, :77-117).  Queries are taken exactly as by zvec_hip_sparse_search /
 *     zvec_hip_sparse_search_by_ids (CSR, values of the handle's type, runs strictly ascending and validated on the host, at
 *     most 4096 pairs a run; count > 2^19, or for listed rows count * longest list > 2^32 - 1, returns ZVEC_HIP_ERR_OUT_OF_RANGE;
 *     ids / offsets as for search_by_ids).  group_of_position[n], ngroups, group_num,
 *     group_topk and the five outputs mean what they mean for zvec_hip_flat_search_grouped, same layout; a position with
 *     group_of >= ngroups does not compete.  A group keeps its group_topk best candidates under (score, scan ordinal), the
 *     ordinal being the storage position for the full scan and the place in the list for listed rows; groups are ranked by
 *     their best score, equal best scores by group number, and the first group_num are kept; documents with score > threshold
 *     are cut AFTER that ranking, so a group may be listed with no document.  A position listed twice competes twice; a
 *     position >= the row count or excluded never competes.  Under ZVEC_HIP_METRIC_IP a pair with no shared index scores
 *     exactly 0 and is an ordinary candidate: the zero ties are resolved by the ordinal rule, which is stricter than the
 *     "unspecified" of Ties above; under ZVEC_HIP_METRIC_L2 equal scores are resolved by the same rule.
 *     ngroups, group_num or group_topk of 0: ZVEC_HIP_ERR_INVALID_ARGUMENT; group_num * 12 + 16 or group_topk * 16 + 16 above
 *     60 KiB: ZVEC_HIP_ERR_UNSUPPORTED; a refused call touches no output.  An empty index gives out_ngroups[q] = 0.
 *   - Inverted lists (zvec_hip_sparse_set_inverted, zvec_hip_sparse_inverted_info), ZVEC_HIP_METRIC_IP only, fp32 or fp16 values,
 *     off by default.  The reference has no such layout: it scans.  enable != 0 asks for a second, term-major layout of the same
 *     rows: the distinct stored indices in ascending order, and per index the list of (storage position, value as stored) of the
 *     rows that hold it, ascending by position.  While it is on, zvec_hip_sparse_search and zvec_hip_sparse_search_dev walk only
 *     the lists of the query's own indices instead of every stored element, for every topk they accept; their contract is the one
 *     above, unchanged: score = -(sum over shared indices), formed with fp32 fma in an order of the library's choosing (here:
 *     the query's run order), a pair without a shared index scores the same zero as without the lists and is an ordinary candidate,
 *     exclude_bitset, threshold, ascending lists, unspecified ties, the 4096-pair cap, validation of host queries and the topk
 *     refusal as above.  The same call twice returns the same bits.  The lists are built on the host from the stored rows by the
 *     first search that needs them; zvec_hip_sparse_append only marks them out of date, and the next such search rebuilds them
 *     once (`builds` counts the builds; the info call never builds).  More than 2^32 - 1 stored pairs, or more than 2^32 - 4096
 *     rows, make such a search return ZVEC_HIP_ERR_OUT_OF_RANGE.  enable == 0 frees the lists.  Listed rows, group-by and
 *     zvec_hip_sparse_get_vector read the rows themselves whether the lists are on or off.  On a ZVEC_HIP_METRIC_L2 handle
 *     zvec_hip_sparse_set_inverted returns ZVEC_HIP_ERR_UNSUPPORTED and changes nothing: the distance over the union of the index
 *     sets would need the expansion that "Score, ZVEC_HIP_METRIC_L2" rules out.  A NULL handle: ZVEC_HIP_ERR_INVALID_ARGUMENT.
 *   - Add-with-id (zvec_hip_sparse_put, zvec_hip_sparse_holes, zvec_hip_sparse_put_info): FlatSparseStreamerEntity::
 *     add_vector_with_id (flat_sparse_streamer_entity.cc:708-783), what Index::_sparse_add calls per document, in bulk.  n rows in
 *     CSR form as for zvec_hip_sparse_append, applied row by row in call order: the row of ids[i] lives at storage position ids[i];
 *     id == count appends; id > count first pads [count, id) with HOLES, empty rows stored under the invalid key (all ones) that
 *     no search returns; id < count replaces the row in place of the old one, and a hole that is written stops being one; an id
 *     named twice in a call keeps the later row.  keys == NULL stores key = id (the reference's rule), else keys[i] with row i.
 *     Validation is that of append (at most 4096 pairs a run, strictly ascending, NULL arrays only where there are no pairs:
 *     ZVEC_HIP_ERR_INVALID_ARGUMENT; so is a NULL ids with n > 0); an id of 2^32 - 1, or more than 2^32 - 2 rows afterwards,
 *     returns ZVEC_HIP_ERR_OUT_OF_RANGE.  All or nothing: a refused call, and one whose allocation fails
 *     (ZVEC_HIP_ERR_NO_MEMORY), leaves rows, keys, holes and counts as they were.  n == 0 returns 0.  Both value types, both
 *     metrics.  zvec_hip_sparse_count reports the pairs stored afterwards: those of a replaced row are gone.  The inverted lists
 *     are marked out of date as by append.  Three routes, chosen per call (zvec_hip_sparse_put_info tells which): 0 tail, every
 *     id at or behind the old count, the append path plus empty rows; 1 in place, every replaced row keeps its length and only
 *     its pairs and key are rewritten; 2 splice, a replaced row changes its length, so the pairs behind it move: the four arrays
 *     are written anew in one pass over the store and swapped in, and until then the store exists twice in device memory.  A put
 *     must not overlap a zvec_hip_sparse_search_dev of the same handle that is still running on the caller's stream.
 *     Holes: every search entry ORs the hole bits into its exclude set (the caller's pointer goes through untouched while the
 *     handle has no hole); zvec_hip_sparse_batch_distance scores a hole +inf; zvec_hip_sparse_get_vector of a hole returns
 *     count 0 and status 0, the empty row the reference stores; exclude bitsets and group_of_position are indexed by storage
 *     position, holes included.  zvec_hip_sparse_append on a handle that has holes extends the hole bits with the rows.
 *   - Rows and queries from device memory (zvec_hip_sparse_append_dev, zvec_hip_sparse_append_dense_dev,
 *     zvec_hip_sparse_from_dense_dev, zvec_hip_sparse_search_dense_dev, zvec_hip_sparse_ingest_info, zvec_hip_sparse_put_dev).
 *     The reference has no such entry: its rows arrive in host memory.  Every array named d_* is device memory of the handle's (the context's)
 *     device.  A DENSE matrix is n rows of `dim` elements of the handle's value type, row r at d_rows + r * ld elements
 *     (ld >= dim); column j becomes index j.  An element is KEPT iff it is not zero: +0 and -0 are dropped, every other bit
 *     pattern is kept as it is, subnormals included (inf and NaN too, with unspecified scores, see Value type); the kept
 *     elements of a row stand in column order, so every run ascends strictly, and the same matrix gives the same bytes on every
 *     call.  Neither d_rows nor ld * sizeof(value) needs to be a multiple of 16 (d_rows must be a multiple of the value's own
 *     size).  Rows are cut into column slices of slice_cols columns (a constant of the library, zvec_hip_sparse_ingest_info), so
 *     a call of one wide row spreads over the device as a call of many rows does.  Validation is the rule of append, done on
 *     the device: at most 4096 pairs a row (a dense row with more non-zeros is REFUSED with the whole call, where the reference
 *     discards the row), runs strictly ascending, and for CSR the counts summing to `elements`:
 *     ZVEC_HIP_ERR_INVALID_ARGUMENT.  So are a NULL handle, a NULL required array with n > 0 and ld < dim; more than 2^32 - 2
 *     rows afterwards returns ZVEC_HIP_ERR_OUT_OF_RANGE.  All or nothing: a refused call leaves rows, keys, holes, counts and
 *     the inverted lists' state as they were.  n == 0 returns 0.  d_keys == NULL stores key = storage position.  Hole bits are
 *     extended and the inverted lists marked out of date as by zvec_hip_sparse_append.  Waits: the two appends enqueue their
 *     checks on `stream` (NULL: the handle's own) and WAIT for it once, to read the status word and the total before anything
 *     of the store changes; they then write the rows on the same stream and return with the rows stored, having drained it as
 *     zvec_hip_sparse_append does.  zvec_hip_sparse_search_dense_dev waits once for its queries' lengths, which
 *     zvec_hip_sparse_search_dev needs on the host to cut query blocks, and then IS that call: scores, ties, threshold, exclude
 *     bitset, topk caps, the row scan or the inverted lists, both metrics, word for word; a query with more than 4096 non-zeros
 *     returns ZVEC_HIP_ERR_INVALID_ARGUMENT and touches no output.  zvec_hip_sparse_from_dense_dev waits once for the total.
 *     A device append must not overlap a zvec_hip_sparse_search_dev of the same handle still running on another stream.
 *     zvec_hip_sparse_put_dev is zvec_hip_sparse_put with d_ids[n], d_counts[n], d_indices[elements], d_values[elements] and
 *     d_keys[n] (or NULL: key = id) in device memory, and its contract is that entry's word for word: call order, the later row
 *     of an id named twice, appends, holes, replacements, all or nothing, both value types and metrics, the three routes chosen
 *     by the same rule and reported by zvec_hip_sparse_put_info, the inverted lists marked out of date; the store afterwards is
 *     byte for byte the store after zvec_hip_sparse_put of the same arrays.  Validation is the rule of append, done on the
 *     device as for zvec_hip_sparse_append_dev (ZVEC_HIP_ERR_INVALID_ARGUMENT, also for a NULL d_ids with n > 0); an id of
 *     2^32 - 1, or more than 2^32 - 2 rows afterwards, returns ZVEC_HIP_ERR_OUT_OF_RANGE; a refused call leaves the last
 *     put_info as it was too.  The pairs and the keys never cross to the host: the host reads back 12 bytes a row (id, count,
 *     the length of the row stored at the id) and the status word, keeps the hole bits, chooses the route and sizes the
 *     allocations; the stage that the in-place and splice kernels read, the keys and the splice's piece table are built on the
 *     device.  Waits: the checks are enqueued on `stream` (NULL: the handle's own) and the call WAITS for it once, for those
 *     words, before anything of the store changes; the rows are then written on the same stream and the call returns with them
 *     stored, having drained it.  A zvec_hip_sparse_put_dev must not overlap a zvec_hip_sparse_search_dev of the same handle
 *     still running on another stream.
 * Not served (each is the reference's to keep doing on the CPU): removing a document, the
 * MipsSquaredEuclideanSparse metric, loaders of the reference's dumped sparse segments, shards, the plugin and the C++ mirror
 * (zvec_hip_operator.hpp); by the inverted lists: ZVEC_HIP_METRIC_L2, listed rows and group-by; from device memory:
 * a matrix of another type than the handle's, and any rule for keeping an element other than "not zero". */
int zvec_hip_sparse_create(int device, zvec_hip_sparse_t *out); /* fp32 values, InnerProductSparse */
/* dtype: ZVEC_HIP_DT_FP32 or ZVEC_HIP_DT_FP16; anything else returns ZVEC_HIP_ERR_UNSUPPORTED and leaves *out untouched.
 * InnerProductSparse. */
int zvec_hip_sparse_create_typed(int dtype, int device, zvec_hip_sparse_t *out);
/* dtype as above; metric: ZVEC_HIP_METRIC_IP (InnerProductSparse) or ZVEC_HIP_METRIC_L2 (SquaredEuclideanSparse).  Any other
 * metric, or an unsupported dtype, returns ZVEC_HIP_ERR_UNSUPPORTED and leaves *out untouched.  The two creators above are
 * calls of this one with ZVEC_HIP_METRIC_IP. */
int zvec_hip_sparse_create_metric(int dtype, int metric, int device, zvec_hip_sparse_t *out);
/* the value type the handle was created with */
int zvec_hip_sparse_dtype(zvec_hip_sparse_t h, int *dtype);
/* the metric the handle was created with */
int zvec_hip_sparse_metric(zvec_hip_sparse_t h, int *metric);
int zvec_hip_sparse_destroy(zvec_hip_sparse_t h);
/* room for `rows` rows and `elements` (index, value) pairs in all; the store also grows on demand, geometrically */
int zvec_hip_sparse_reserve(zvec_hip_sparse_t h, uint64_t rows, uint64_t elements);
/* FlatSparseStreamer::add_impl / add_with_id_impl (flat_sparse_streamer.cc:186-300) in bulk: n rows in storage order, row i
 * being counts[i] pairs; keys == NULL -> key = storage position.  All or nothing (see Row format, Index order). */
int zvec_hip_sparse_append(zvec_hip_sparse_t h, const uint32_t *counts, const uint32_t *indices, const void *values,
                           uint64_t n, const uint64_t *keys);
/* zvec_hip_sparse_append with every array in device memory: d_counts[n], the runs back to back in d_indices[elements] /
 * d_values[elements], d_keys[n] or NULL.  Validated on the device; see Rows and queries from device memory above. */
int zvec_hip_sparse_append_dev(zvec_hip_sparse_t h, const uint32_t *d_counts, const uint32_t *d_indices, const void *d_values,
                               uint64_t n, uint64_t elements, const uint64_t *d_keys, void *stream);
/* n dense device rows of `dim` elements of the handle's value type, `ld` elements apart: the non-zeros of row r become the row at
 * the next storage position, column j as index j.  dim == 0 gives empty rows.  See Rows and queries from device memory above. */
int zvec_hip_sparse_append_dense_dev(zvec_hip_sparse_t h, const void *d_rows, uint64_t n, uint32_t dim, uint64_t ld,
                                     const uint64_t *d_keys, void *stream);
/* The converter alone, as zvec_hip_binary_encode_dev is for the sign bits: n dense device rows of dtype ZVEC_HIP_DT_FP32 or
 * ZVEC_HIP_DT_FP16 (anything else: ZVEC_HIP_ERR_UNSUPPORTED) -> d_counts[n] and the runs back to back in d_indices / d_values
 * (room for elems_cap pairs).  *elements, the pairs of the matrix, is always written (0 by a refused call).  d_indices or d_values
 * NULL: a size query, only the counts are written.  ZVEC_HIP_ERR_OUT_OF_RANGE when elems_cap is too small: nothing but the counts
 * is written.  A row may be longer than 4096 here: the converter does not know an index's cap.  Waits once on `stream` (NULL: the
 * context's) for the total; the pairs are enqueued behind it.  A NULL ctx, elements, d_in or d_counts with n > 0, and ld < dim:
 * ZVEC_HIP_ERR_INVALID_ARGUMENT. */
int zvec_hip_sparse_from_dense_dev(zvec_hip_ctx_t ctx, int dtype, const void *d_in, uint64_t n, uint32_t dim, uint64_t ld,
                                   uint32_t *d_counts, uint32_t *d_indices, void *d_values, uint64_t elems_cap, uint64_t *elements,
                                   void *stream);
/* The last successful zvec_hip_sparse_append_dev / _append_dense_dev of the handle.  route: -1 none yet, 0 CSR, 1 dense; elements:
 * the pairs that call stored; slice_cols: columns of one work item of the dense converter (a constant of the library, reported
 * before any call); ms: wall-clock time of the call.  Every output nullable. */
int zvec_hip_sparse_ingest_info(zvec_hip_sparse_t h, int *route, uint64_t *elements, uint32_t *slice_cols, double *ms);
/* FlatSparseStreamer::add_with_id_impl in bulk: row i, counts[i] pairs, goes to storage position ids[i]; see Add-with-id above. */
int zvec_hip_sparse_put(zvec_hip_sparse_t h, const uint32_t *ids, const uint32_t *counts, const uint32_t *indices,
                        const void *values, uint64_t n, const uint64_t *keys);
/* zvec_hip_sparse_put with every array in device memory: d_ids[n], d_counts[n], the runs back to back in d_indices[elements] /
 * d_values[elements], d_keys[n] or NULL.  Validated on the device, one wait, the pairs stay on the device; see Rows and queries
 * from device memory above.  zvec_hip_sparse_put_info reports it as it reports a host put. */
int zvec_hip_sparse_put_dev(zvec_hip_sparse_t h, const uint32_t *d_ids, const uint32_t *d_counts, const uint32_t *d_indices,
                            const void *d_values, uint64_t n, uint64_t elements, const uint64_t *d_keys, void *stream);
/* positions that are holes now */
int zvec_hip_sparse_holes(zvec_hip_sparse_t h, uint64_t *count);
/* The last successful zvec_hip_sparse_put / _put_dev of the handle.  route: -1 none yet, 0 tail, 1 in place, 2 splice; moved_elems:
 * (index, value) pairs the device wrote for it (routes 0 and 1: the call's own; route 2: every pair of the store); chunk_elems:
 * destination pairs one work-group of the splice copies (a constant of the library, reported before any put); ms: wall-clock time
 * of the call.  Every output nullable. */
int zvec_hip_sparse_put_info(zvec_hip_sparse_t h, int *route, uint64_t *moved_elems, uint32_t *chunk_elems, double *ms);
/* either output nullable */
int zvec_hip_sparse_count(zvec_hip_sparse_t h, uint64_t *rows, uint64_t *elements);
/* get_sparse_vector_by_id: row `pos` as stored, bit for bit (halves come back as halves).  *count always; indices / values
 * (room for *count entries, at most 4096) may each be NULL: a size query.  ZVEC_HIP_ERR_NO_EXIST beyond the last row. */
int zvec_hip_sparse_get_vector(zvec_hip_sparse_t h, uint64_t pos, uint32_t *count, uint32_t *indices, void *values);
/* search_impl / search_bf_impl(sparse_count, sparse_indices, sparse_query, qmeta, count, ctx) (flat_sparse_search.h:58-148):
 * `count` queries, query q being q_counts[q] pairs, runs back to back.  Outputs as zvec_hip_flat_search. */
int zvec_hip_sparse_search(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                           const void *q_values, uint32_t count, uint32_t topk, float threshold,
                           const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
/* The same with the queries' pairs, the bitset and the outputs in device memory; enqueues on `stream` and returns.  q_counts
 * stays a HOST array: the host cuts the batch into query blocks by length before it launches anything. */
int zvec_hip_sparse_search_dev(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts,
                               const uint32_t *d_q_indices, const void *d_q_values, uint32_t count, uint32_t topk,
                               float threshold, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                               float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* zvec_hip_sparse_search_dev for `count` DENSE device queries of `dim` elements of the handle's value type, `ld` elements apart:
 * their non-zeros are gathered into the context's workspace, the lengths come to the host (the call's one wait), and the search
 * above runs on them unchanged.  See Rows and queries from device memory above. */
int zvec_hip_sparse_search_dense_dev(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t dim,
                                     uint64_t ld, uint32_t topk, float threshold, const uint64_t *d_exclude_bitset,
                                     uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* FlatSparseStreamer::search_bf_by_p_keys_impl (flat_sparse_streamer.cc:324-349; FlatSparseSearcher, flat_sparse_searcher.cc:
 * 98-103; FlatSparseEntity::search_p_keys, flat_sparse_entity.h:63-77): query q against rows ids[offsets[q] .. offsets[q+1])
 * only (offsets[count + 1], offsets[0] == 0; ids may be NULL when every list is empty).  Queries and outputs as
 * zvec_hip_sparse_search; see Listed rows above. */
int zvec_hip_sparse_search_by_ids(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts,
                                  const uint32_t *q_indices, const void *q_values, uint32_t count, const uint32_t *ids,
                                  const uint32_t *offsets, uint32_t topk, float threshold, const uint64_t *exclude_bitset,
                                  uint64_t *out_keys, float *out_scores, uint32_t *out_counts);
/* IndexMetric::batch_distance (index_metric.h:85-87) over sparse rows, scored as search_p_keys scores its keys
 * (flat_sparse_entity.h:63-77): one query of q_count pairs against n listed positions, scores only, in the listed order; a
 * position beyond the rows, and a hole, scores +inf.  n == 0 returns 0 and writes nothing. */
int zvec_hip_sparse_batch_distance(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, uint32_t q_count, const uint32_t *q_indices,
                                   const void *q_values, const uint32_t *positions, uint32_t n, float *out_scores);
/* The term-major twin of the rows; see Inverted lists above. */
int zvec_hip_sparse_set_inverted(zvec_hip_sparse_t h, int enable);
/* enabled: asked for; bytes: device memory the lists hold now (0 before the first build); terms: distinct stored indices at the last
 * build; tile_rows: consecutive positions one work item of the search accumulates (a constant of the library, reported whether the
 * lists are on or off); builds: builds since the handle was created.  Every output nullable. */
int zvec_hip_sparse_inverted_info(zvec_hip_sparse_t h, int *enabled, uint64_t *bytes, uint64_t *terms, uint32_t *tile_rows,
                                  uint64_t *builds);
/* The lists as they are held, copied to host memory: terms[*nterms] ascending and distinct, list_off[*nterms + 1] (the last one is
 * *elems), ppos[*elems] ascending inside every list, pval[*elems] in the handle's value type, bit for bit as stored.  Lists that are
 * out of date are rebuilt first, as by a search.  *nterms and *elems are always written; the array pointers may be NULL to ask for
 * the sizes only.  terms_cap counts the entries of `terms` (list_off has room for terms_cap + 1), elems_cap those of ppos and pval:
 * ZVEC_HIP_ERR_OUT_OF_RANGE when a capacity of a non-NULL array is too small, ZVEC_HIP_ERR_UNSUPPORTED while the lists are off. */
int zvec_hip_sparse_inverted_export(zvec_hip_sparse_t h, uint32_t *terms, uint64_t terms_cap, uint64_t *list_off, uint32_t *ppos,
                                    void *pval, uint64_t elems_cap, uint64_t *nterms, uint64_t *elems);
/* The build that made the lists held now: route 0 = host, 1 = device (option "sparse_inverted_build"), -1 while nothing is built;
 * passes: 8-bit digit passes of the device build's sort, ceil(bits(OR of the stored indices) / 8), 0 on the host route; block_elems:
 * elements one work-group of the device sort's scatter handles (a constant of the library, reported before any build); ms: wall-clock
 * time of the build.  Every output nullable. */
int zvec_hip_sparse_inverted_build_info(zvec_hip_sparse_t h, int *route, uint32_t *passes, uint32_t *block_elems, double *ms);
/* Group-by over every row (FlatSparseEntity::search_group, flat_sparse_entity.h:79-103); see Group-by above. */
int zvec_hip_sparse_search_grouped(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                                   const void *q_values, uint32_t count, const uint32_t *group_of_position, uint32_t ngroups,
                                   uint32_t group_num, uint32_t group_topk, float threshold, const uint64_t *exclude_bitset,
                                   uint32_t *out_groups, uint32_t *out_ngroups, uint64_t *out_keys, float *out_scores,
                                   uint32_t *out_counts);
/* Group-by over listed rows (FlatSparseEntity::search_group_p_keys, flat_sparse_entity.h:105-128): query q against rows
 * ids[offsets[q] .. offsets[q+1]) only, as zvec_hip_sparse_search_by_ids lists them. */
int zvec_hip_sparse_search_grouped_by_ids(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts,
                                          const uint32_t *q_indices, const void *q_values, uint32_t count, const uint32_t *ids,
                                          const uint32_t *offsets, const uint32_t *group_of_position, uint32_t ngroups,
                                          uint32_t group_num, uint32_t group_topk, float threshold,
                                          const uint64_t *exclude_bitset, uint32_t *out_groups, uint32_t *out_ngroups,
                                          uint64_t *out_keys, float *out_scores, uint32_t *out_counts);

/* ---- HNSW: search on a built graph ----------------------------------------------------------
 * stands behind HnswSearcher::search_impl (src/core/algorithm/hnsw/hnsw_searcher.cc) above its brute-force hand-over: the walk of
 * HnswAlgorithm::search, select_entry_point and search_neighbors (hnsw_algorithm.cc:83-278), restated in DESIGN §3c, one wave per
 * query.  The handle loads a graph that is already built, or builds one from rows (zvec_hip_hnsw_build, below), and takes more rows
 * afterwards (zvec_hip_hnsw_add, below); deleting nodes, reading the
 * reference's dumped HNSW segments (hnsw_searcher_entity.cc), the cosine metric and group-by are not served.  Small indexes
 * (doc_cnt <= bruteforce_threshold) are the caller's to hand to a flat handle.
 *   - ZVEC_HIP_METRIC_L2 (score = squared distance) or ZVEC_HIP_METRIC_IP (score = MINUS the dot product, as on the flat
 *     index); every other metric, and a dim above 4096: ZVEC_HIP_ERR_UNSUPPORTED;
 *   - Element type.  A handle serves ONE element type: ZVEC_HIP_DT_FP32 (float) or, through zvec_hip_hnsw_create_typed,
 *     ZVEC_HIP_DT_FP16 (IEEE binary16, 2 bytes) — the reference's HNSW after HalfFloatConverter / HalfFloatReformer.  Every `rows`,
 *     `queries` and get_vectors `out` pointer below, host or device, is a `const void *` / `void *` read as elements of the handle's
 *     type, the way zvec_hip_flat_* treats `vecs`; scores are fp32 for either type.  Halves are stored as halves (half the bytes
 *     held, half the bytes a distance fetches).  Each is widened to fp32 where it is read, which is exact (subnormals included,
 *     nothing flushed), and from there on the arithmetic is the fp32 handle's, operation for operation and in the same order
 *     (the reference widens too: distance_matrix_fp16.i, _mm256_cvtph_ps into fp32 accumulators).  So an fp16 handle answers — lists,
 *     counts, statistics, built and appended graphs and their counters — bit for bit as an fp32 handle given the widened rows and
 *     queries would.  No half-precision arithmetic.  Values must be finite: inf and NaN are not checked for and give unspecified
 *     results.  DESIGN §3c "fp16 rows".
 *   - a node is its position 0 .. n-1; exclude_bitset, threshold, out_counts and the fill of the places past out_counts[q]
 *     (key 2^64 - 1, score +inf) are those of zvec_hip_flat_search; an excluded node is walked through but never returned;
 *   - lists are ascending by (score, node); of two candidates or results at one distance the one with the smaller node comes first,
 *     and the largest by (distance, node) leaves a full set — the reference's KeyValueHeap leaves equal keys in heap order. */
typedef struct zvec_hip_hnsw_s *zvec_hip_hnsw_t;
/* the fp32 creator: dtype must be ZVEC_HIP_DT_FP32; every other type is ZVEC_HIP_ERR_UNSUPPORTED here, ZVEC_HIP_DT_FP16 included
 * (callers of this entry hand over float pointers; that behaviour is kept exactly) */
int zvec_hip_hnsw_create(uint32_t dim, int dtype, int metric, int device, zvec_hip_hnsw_t *out);
/* dtype: ZVEC_HIP_DT_FP32 or ZVEC_HIP_DT_FP16.  Any other type or metric returns ZVEC_HIP_ERR_UNSUPPORTED and leaves *out untouched.
 * With ZVEC_HIP_DT_FP32 this is zvec_hip_hnsw_create. */
int zvec_hip_hnsw_create_typed(uint32_t dim, int dtype, int metric, int device, zvec_hip_hnsw_t *out);
/* the element type the handle was created with */
int zvec_hip_hnsw_dtype(zvec_hip_hnsw_t h, int *dtype);
int zvec_hip_hnsw_destroy(zvec_hip_hnsw_t h);
/* HnswSearcher::load in the shape of plain host arrays — what HnswEntity serves the algorithm: get_vector / get_key (rows [n][dim],
 * keys [n], NULL = the position), get_neighbors(0, id) (nbr0 [n][m0] with cnt0 [n] valid entries each), get_neighbors(level >= 1, id)
 * (upper_of [n]: index into the upper table or 0xffffffff for a node of level 0 only; nbr_up [n_upper][max_level][m] with
 * cnt_up [n_upper][max_level], level l at slot l - 1, count 0 above a node's own level), entry_point() and cur_max_level().
 * max_level == 0: the upper arrays are not read.  InvalidArgument (-31), the handle untouched, for: a neighbour >= n, a count above
 * m0 / m, entry_point >= n, upper_of beyond n_upper, and — with max_level >= 1 — an entry point or an upper-level neighbour without
 * upper lists.  A second load replaces the first; n == 0 is a valid empty index (every search answers with empty lists). */
int zvec_hip_hnsw_load(zvec_hip_hnsw_t h, uint64_t n, const void *rows, const uint64_t *keys, uint32_t m0, const uint32_t *nbr0,
                       const uint32_t *cnt0, uint32_t max_level, uint32_t m, uint32_t n_upper, const uint32_t *upper_of,
                       const uint32_t *nbr_up, const uint32_t *cnt_up, uint32_t entry_point);
/* what load took, read back (every pointer nullable): the shape, rows by position (HnswEntity::get_vector), the other arrays */
int zvec_hip_hnsw_info(zvec_hip_hnsw_t h, uint64_t *n, uint32_t *dim, uint32_t *m0, uint32_t *max_level, uint32_t *m, uint32_t *n_upper,
                       uint32_t *entry_point);
int zvec_hip_hnsw_get_vectors(zvec_hip_hnsw_t h, const uint64_t *positions, uint64_t n, void *out);
int zvec_hip_hnsw_export(zvec_hip_hnsw_t h, uint64_t *keys, uint32_t *nbr0, uint32_t *cnt0, uint32_t *upper_of, uint32_t *nbr_up,
                         uint32_t *cnt_up);
/* HnswSearcher::search_impl(query, qmeta, count, ctx): queries [count][dim] of the handle's element type.  ef: HnswContext's ef (kDefaultEf = 500,
 * hnsw_params.h); the walk runs with max(ef, topk), above 512 Unsupported (-12).  max_scan: the context's scan limit
 * (reach_scan_limit), counted in distances computed, 0 = n.  Batches go in slices of queries that keep the walk's workspace within
 * the "hnsw_ws_bytes" option (1024 .. 2^30, default 2^30): ceil(n / 32) * 4 bytes per query, plus 8 * min(max_scan, n) bytes per
 * query when min(max_scan, n) > 1024; the same results either way. */
int zvec_hip_hnsw_search(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count, uint32_t topk, uint32_t ef,
                         uint32_t max_scan, float threshold, const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                         uint32_t *out_counts);
int zvec_hip_hnsw_search_dev(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk, uint32_t ef,
                             uint32_t max_scan, float threshold, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                             float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* HnswContext's debugging counters of the last search of `h` on the context (stats_get_vector's rows, stats_get_neighbors at level 0),
 * for its first `count` queries: distances computed, nodes expanded on level 0, and the slices the batch went in (each nullable).
 * Waits for the context's stream.  NoReady (-21) when the context's last search was not one of `h` or was shorter. */
int zvec_hip_hnsw_last_stats(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t *out_scanned, uint32_t *out_hops,
                             uint32_t *out_slices);

/* ---- HNSW: building a graph from rows --------------------------------------------------------
 * stands behind HnswBuilder::train / build (hnsw_builder.cc) and HnswAlgorithm::add_node (hnsw_algorithm.cc:31-81).  The reference
 * inserts node by node under locks and its graph depends on thread timing; this build inserts in ROUNDS: every node of a round
 * searches the graph as it stood when the round began, then the links are written (DESIGN §3c "Building" is the specification).
 * With s nodes in the graph a round takes clamp(s / round_div, 1, round_max) nodes in index order — options "hnsw_build_round_div"
 * (0 .. 2^20, default 16; 0 = one node per round, the sequential order) and "hnsw_build_round_max" (1 .. 2^20, default 4096) —
 * and a node above the current top level is a round of its own.  The result depends on nothing but the arguments and the two options.
 * A field of the parameters left 0 takes the reference's default (hnsw_builder.cc:36-99, hnsw_entity.h): m 50 (upper levels),
 * m0 2 * m, ef_construction 500, prune_cnt m, scaling_factor m; min_neighbors 0 is its default. */
typedef struct zvec_hip_hnsw_build_params {
  uint32_t m, m0, ef_construction, prune_cnt, min_neighbors, scaling_factor;
  uint64_t seed;                       /* of the level generator, when no levels are passed */
} zvec_hip_hnsw_build_params;
typedef struct zvec_hip_hnsw_build_info {
  uint32_t rounds;                     /* after the seed node */
  uint32_t slices;                     /* the most slices one round's insert phase went in ("hnsw_ws_bytes") */
  uint32_t top, entry_point;           /* HnswEntity::cur_max_level(), entry_point() after the build */
  uint64_t dists;                      /* distances the insert phase computed: walks, and candidate-to-kept pairs of the selections */
  uint64_t requests;                   /* reverse links asked for = neighbours selected */
  uint64_t prunes;                     /* requests that met a full list (reverse_update_neighbors past its early return) */
  double insert_ms, reverse_ms;        /* device time of the insert kernels / of sort, grouping and the reverse kernels */
} zvec_hip_hnsw_build_info;
#define ZVEC_HIP_HNSW_BUILD_MAX_LEVEL 15
/* HnswAlgorithm::get_random_level in integer arithmetic (the same levels from C and from Python): with
 * r = splitmix64(seed + i * 0x9E3779B97F4A7C15) >> 11, where splitmix64(x) is the output of the SplitMix64 generator whose state
 * before the call is x, the level of node i is the number of k >= 1 with r * scaling_factor^k < 2^53, at most 15:
 * P(level >= k) = scaling_factor^-k.  Host only.  InvalidArgument for a scaling_factor outside 5 .. 1000 (hnsw_builder.cc:84). */
int zvec_hip_hnsw_build_levels(uint64_t n, uint32_t scaling_factor, uint64_t seed, uint32_t *out_levels);
/* HnswBuilder::build: rows [n][dim] of the handle's element type (host), keys [n] or NULL = the position, levels [n] (each <= 15) or NULL = generated.
 * Replaces the handle's arrays whole under its exclusive lock, like load; search, info, export and get_vectors then serve the built
 * graph (upper table: upper_of = rank among the nodes of level >= 1, stride = the largest level).  n == 0 and n == 1 are valid.
 * Unsupported (-12): ef_construction > 512, m0 > 256, m > 128.  InvalidArgument (-31): min_neighbors above m or m0, a level above 15,
 * a generated level asked for with scaling_factor outside 5 .. 1000.  The insert phase of a round goes in slices of nodes whose
 * visited bits (ceil(s / 32) * 4 bytes a node with s nodes in the graph) and candidate regions (8 * s bytes a node once s > 1024)
 * stay within "hnsw_ws_bytes"; the same graph either way.  The handle remembers the parameters for later adds. */
int zvec_hip_hnsw_build(zvec_hip_hnsw_t h, uint64_t n, const void *rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                        const uint32_t *levels);
/* the same with rows [n][dim] in device memory (keys and levels stay host arrays); synchronous */
int zvec_hip_hnsw_build_dev(zvec_hip_hnsw_t h, uint64_t n, const void *d_rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                            const uint32_t *levels);
/* what the last build of `h` did; NoReady (-21) before the first one */
int zvec_hip_hnsw_last_build_info(zvec_hip_hnsw_t h, zvec_hip_hnsw_build_info *out);

/* ---- HNSW: appending rows to a graph ---------------------------------------------------------
 * stands behind HnswStreamer::add_impl / add_with_id_impl (src/core/algorithm/hnsw/hnsw_streamer.cc:426-585), which end in
 * HnswAlgorithm::add_node(id, level, ctx): documents arrive after the index exists, and searches run between the arrivals.  The new
 * rows take the positions n .. n + count - 1 and are inserted by the build's own rounds, started at s = n nodes (DESIGN §3c
 * "Appending" is the specification): build(A) then add(B) gives the graph of one build of all rows, except that a round ends at the
 * call boundary.  With "hnsw_build_round_div" 0, or one row per call, that is the sequential graph.  A call does no work in
 * proportion to n unless an array must grow or the upper table must be re-strided.  A round of one node applies its reverse links
 * without sorting them (its targets are distinct and have one source each).  Adds and searches on one handle exclude each other. */
typedef struct zvec_hip_hnsw_add_info {
  uint32_t rounds, slices, top, entry_point;       /* as zvec_hip_hnsw_build_info, for this call alone; top / entry_point after it */
  uint64_t dists, requests, prunes;
  double insert_ms, reverse_ms;
  uint64_t first, count;               /* the call's rows took the positions first .. first + count - 1 */
  uint32_t rounds_one;                 /* of `rounds`, those of one node: reverse links applied without sort and grouping */
  uint32_t grew_rows, grew_upper;      /* 1: the arrays per row / per upper node were moved into larger ones by this call */
  uint32_t restrided;                  /* 1: the call held a node above the largest level, and the upper table was re-strided (or made) */
  uint64_t cap_rows, cap_upper;        /* rows / upper nodes the arrays have room for after the call */
} zvec_hip_hnsw_add_info;
/* HnswStreamer::add_impl for count rows at once: rows [count][dim] of the handle's element type (host), keys [count] or NULL = the position, levels [count]
 * (each <= 15) or NULL = the level zvec_hip_hnsw_build_levels(n + count, scaling_factor, seed) gives each global position, which does
 * not depend on how the rows were split into calls.  p: NULL, or a field left 0, means the value of the handle's last build, and on a
 * handle that load filled the reference's default (as zvec_hip_hnsw_build).  InvalidArgument (-31): an m0 that is neither 0 nor the
 * graph's once it has nodes, an m that is neither 0 nor the graph's once it has upper lists, min_neighbors above m or m0, a level
 * above 15, rows NULL with count > 0.  Unsupported (-12): the build's limits.  OutOfRange (-17): n + count >=
 * 0xfffffff0.  Every argument is validated before the handle is touched.  count == 0 succeeds and changes nothing.  On a handle that
 * holds no graph the call is a build of these rows (node 0 is the seed).  The arrays grow geometrically (device-to-device copies);
 * a call with a node above the largest level re-strides the upper table once, before its first round, so that export always has the
 * layout of a build: upper_of = rank among the nodes of level >= 1, stride = the largest level. */
int zvec_hip_hnsw_add(zvec_hip_hnsw_t h, uint64_t count, const void *rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                      const uint32_t *levels);
/* the same with rows [count][dim] in device memory (keys and levels stay host arrays); synchronous like build_dev */
int zvec_hip_hnsw_add_dev(zvec_hip_hnsw_t h, uint64_t count, const void *d_rows, const uint64_t *keys,
                          const zvec_hip_hnsw_build_params *p, const uint32_t *levels);
/* HnswStreamerEntity's chunked storage in one step: room for `rows` rows and `upper_nodes` nodes of level >= 1, so that adds up to
 * there move nothing.  Never shrinks.  upper_nodes == 0: min(rows, rows / (scaling_factor - 1) + 64) with the scaling_factor of the
 * last build (the reference's default, m, on a loaded handle) — the expectation rows / scaling_factor times sf / (sf - 1), plus 64.
 * On a handle that holds no graph yet the sizes are kept for the first add.  load and build allocate exactly what they need. */
int zvec_hip_hnsw_reserve(zvec_hip_hnsw_t h, uint64_t rows, uint64_t upper_nodes);
/* what the last add of `h` did; NoReady (-21) before the first one.  zvec_hip_hnsw_last_build_info keeps describing the last build. */
int zvec_hip_hnsw_last_add_info(zvec_hip_hnsw_t h, zvec_hip_hnsw_add_info *out);

#ifdef __cplusplus
}
#endif
#endif /* ZVEC_HIP_H_ */
