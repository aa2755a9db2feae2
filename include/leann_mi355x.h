/*
 * leann_mi355x.h -- C ABI of libleann_mi355x.so, the MI355X (gfx950) native replacement for the
 * query-time selective-recompute beam search of LEANN.
 *
 * Every entry point names the reference interface it replaces (paths relative to the LEANN tree,
 * packages/...).  The reference reaches its native code through SWIG (faiss fork) and pybind11
 * (DiskANN fork); both forks are un-vendored submodules, so the binding surface is taken from the
 * Python call sites.  Plain C: pointers + sizes, no torch / C++ types.  All functions return 0 on
 * success or a negative LM_E* code; lm_last_error() gives the thread-local message.  Nothing throws
 * across this boundary.  Pointer arguments named d_* are DEVICE (HBM) pointers, everything else is
 * host memory.  A handle is not re-entrant: one search at a time per lm_index.
 */
#ifndef LEANN_MI355X_H
#define LEANN_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LM_OK 0
#define LM_EINVAL (-1)   /* bad argument                 -> Python ValueError      */
#define LM_ENOENT (-2)   /* file missing                 -> FileNotFoundError      */
#define LM_EFORMAT (-3)  /* malformed index file         -> ValueError             */
#define LM_EHIP (-4)     /* HIP runtime failure / no GPU -> RuntimeError           */
#define LM_ESTATE (-5)   /* e.g. recompute requested but no provider attached -> RuntimeError */
#define LM_EPROVIDER (-6)/* embedding provider callback failed                     */

#define LM_METRIC_INNER_PRODUCT 0 /* faiss.METRIC_INNER_PRODUCT: "mips", "cosine" (hnsw_backend.py:25-29) */
#define LM_METRIC_L2 1            /* faiss.METRIC_L2 */

#define LM_DTYPE_F32 0
#define LM_DTYPE_F16 1

typedef struct lm_index lm_index;     /* HBM-resident compact-CSR graph + search workspace */
typedef struct lm_tokens lm_tokens;   /* HBM-resident pre-tokenised passage store           */

/* ---- errors / device ------------------------------------------------------------------- */
const char *lm_last_error(void);
int lm_device_count(void);           /* 0 when no HIP device is visible */
const char *lm_version(void);
/* Revision of THIS interface: bumped whenever an entry point, a struct layout or an enum of this header changes incompatibly (6: round 6 --
 * lm_kernel_timing_read takes the caller's capacity; lm_search_params.batch_size has a meaning; LM_KT_COUNT grew in round 5).  A binding
 * compares lm_abi_revision() with the LM_ABI_REVISION it was written against before it calls anything else. */
#define LM_ABI_REVISION 6
int lm_abi_revision(void);

/* ---- index lifetime ---------------------------------------------------------------------
 * Replaces faiss.read_index(str(index_file), faiss.IO_FLAG_MMAP, HNSWIndexConfig{is_compact,
 * is_recompute})                                   leann_backend_hnsw/hnsw_backend.py:145-151.
 * Parses the compact-CSR file written by convert_to_csr.py:182-237 (or the original IHNf layout,
 * :264-301,439-479) and uploads level_ptr / node_offsets / neighbors / levels to HBM.  If the file
 * carries flat embedding storage it is attached as the stored-embedding table. */
int lm_index_read(const char *path, int device, lm_index **out);

/* Same, from arrays already in host memory (layout of convert_to_csr.py:494-548). */
int lm_index_create_from_csr(int64_t ntotal, int32_t d, int32_t metric,
                             const uint64_t *node_offsets /* ntotal+1 */,
                             const uint64_t *level_ptr, int64_t n_level_ptr,
                             const int32_t *neighbors, int64_t n_neighbors,
                             const int32_t *levels /* ntotal */,
                             int32_t entry_point, int32_t max_level, int device, lm_index **out);

/* An index that is a live VIEW of device-resident level adjacencies: the graph a caller is building with lm_select_neighbors and
 * lm_graph_add_links, searched in place.  The handle holds no copy of the graph.  (csrc/lm_view_impl.h)
 *   levels   HOST array of n_levels descriptors, levels[l] = level l; the device arrays they point to are BORROWED: the caller keeps
 *            them alive (and at the same addresses) for as long as the handle is searched.
 * Graph.  The neighbours of node v at level l are the non-empty slots of v's row in levels[l].d_adj, in slot order; the row index is
 * v's position in levels[l].d_nodes, found by binary search.  A node that level l does not list has no neighbours there and is never
 * dereferenced.  Level 0 must be the identity level (d_nodes == NULL, n_rows == ntotal).  max_level = n_levels - 1.
 * That d_nodes is strictly ascending is the caller's promise: it is NOT checked (the array lives on the device; checking it would
 * need a device read).  A list that is not sorted makes nodes unfindable, nothing worse: only rows below n_rows are read.
 * Live.  A search reads the arrays as they are when its kernel runs, in stream order: after lm_graph_add_links (or any other writer)
 * on the index's stream (lm_index_set_stream), the next search sees the new lists.  The handle is not re-created for this.
 * Equivalence.  With recompute = 0 and an attached table (lm_index_attach_table, either location, fp32 or fp16), lm_index_search* on
 * the view returns what lm_index_search* returns on the CSR index in which node v carries levels 0 .. top(v) -- top(v) = the highest
 * level that lists v -- and each list holds the non-empty slots of v's row in slot order: labels, distance bits, ndis, nexpand and
 * nrounds are identical, for any efSearch, beam_size, check_relative_distance, k and max_batch; hence also identical to
 * oracle/lm_oracle.c:orc_search on that CSR.  A query's result does not depend on the other queries of the call nor on how max_batch
 * cuts the call into passes.
 * lm_index_info: max_degree0 = levels[0].cap, max_degree_up = the largest upper cap, n_neighbors = the sum of n_rows * cap (slots,
 * not links); the other fields keep their meaning.
 * What a view does not serve -- each returns LM_ESTATE before anything is staged or launched, the outputs untouched: a search with
 * recompute = 1, batch_size > 0 or pq_pruning_ratio > 0; a search while option "persistent_table" is 0 (a view has the persistent
 * launch only) or without a table; lm_index_search_filtered*; lm_pq_attach*, lm_pq_batch_search*, lm_pq_flat_search* on the handle;
 * lm_index_set_hub_cache.  lm_index_search_exact* reads only the table and keeps working.
 * LDS rule: with maxnew = max(beam_size * levels[0].cap, largest upper cap, 1) and P(x) = the next power of two, a search needs
 * (2 * max(efSearch, k) + P(maxnew)) * 8 + 4 * maxnew <= 150 KiB (the persistent launch's own rule with the capacity in place of the
 * largest degree); otherwise LM_EINVAL, the outputs untouched -- a view has no lock-step fallback.  beam_size > 64: LM_EINVAL.
 * Option "persistent_wave": -1 (auto) and 0 give the 256-thread workgroup per query (a view knows no mean degree), 1 the wave per
 * query; both give the same bits.
 * LM_EINVAL at creation, no handle returned: NULL levels or out; n_levels < 1; ntotal < 0 or > INT32_MAX; an unsupported d (the
 * widths the search kernels cover: d padded to 64..384, 512, 768, 1024) or metric; a level with cap < 1, n_rows < 0 or
 * n_rows > ntotal; level 0 not the identity level; an upper level with n_rows > 0 and NULL d_nodes (unless n_rows == ntotal: the
 * identity); NULL d_adj with n_rows > 0; entry_point outside [0, ntotal) when ntotal > 0.  ntotal == 0 gives a valid handle whose
 * searches fill the empty values.  lm_index_free frees the handle, never the level arrays. */
typedef struct {
    const int32_t *d_nodes; /* n_rows node ids, strictly ascending; NULL = identity (row r is node r), then n_rows == ntotal */
    const int32_t *d_adj;   /* [n_rows][cap], lm_graph_add_links' layout: a slot value outside [0, ntotal) is EMPTY, holes tolerated */
    int64_t n_rows;
    int32_t cap;
} lm_graph_level;
int lm_index_create_view(int64_t ntotal, int32_t d, int32_t metric, const lm_graph_level *levels /* host array */,
                         int32_t n_levels, int32_t entry_point, int device, lm_index **out);
void lm_index_free(lm_index *idx);

typedef struct {
    int64_t ntotal;
    int32_t d;
    int32_t d_padded;       /* row stride of embeddings handed to the kernels (multiple of 64) */
    int32_t metric;
    int32_t entry_point;
    int32_t max_level;
    int32_t max_degree0;    /* largest level-0 neighbour list */
    int32_t max_degree_up;  /* largest upper-level neighbour list */
    int64_t n_neighbors;
    int32_t has_table;      /* stored embeddings attached (non-pruned index) */
    int32_t has_provider;
    int32_t device;
} lm_index_info_t;
int lm_index_info(const lm_index *idx, lm_index_info_t *out);

/* ---- embedding sources --------------------------------------------------------------------
 * Stored embeddings (recompute_embeddings=False on a non-pruned index, hnsw_backend.py:189-193):
 * rows of `table` are gathered straight from HBM by the distance kernel.
 * location 0: host pointer, copied (and zero-padded to d_padded) into library-owned HBM;
 * location 1: device pointer with row stride d_padded, borrowed (caller keeps it alive). */
int lm_index_attach_table(lm_index *idx, const void *table, int32_t dtype, int64_t ntotal, int32_t d,
                          int32_t location);

/* Recompute provider: replaces the per-hop ZMQ REQ of the faiss fork to the embedding server
 * ([[ids],[query]] -> distances / [ids] -> embeddings, hnsw_embedding_server.py:148-284).
 * Called once per search round, on the index's stream, with the SORTED, DE-DUPLICATED node ids
 * of that round in device memory.  (One opt-in exception: with the index option "single_query_direct" a ONE-query pass hands over
 * its new-list as it is -- every id once, in discovery order, not sorted.)  The callback must enqueue (on `stream`) work that produces
 * fp32 embeddings [n][d_padded] (zero padded) in device memory and store that buffer's address
 * in *d_out; the buffer must stay valid until the next callback or the end of the search.
 * Return 0 on success; any other value aborts the search with LM_EPROVIDER. */
typedef int (*lm_provider_fn)(void *user, const int32_t *d_ids, int32_t n, void **d_out, void *stream);
int lm_index_set_provider(lm_index *idx, lm_provider_fn fn, void *user);

/* Hub-embedding cache (LEANN paper section 5: caching the embeddings of the highest-degree ~10 % nodes): the rows
 * of d_embeddings [n][d_padded] (fp32, device) are copied into HBM owned by the index; nodes listed in `ids` (host,
 * unique) are never sent to the provider again.  n = 0 clears the cache.  Cf. num_nodes_to_cache of the DiskANN
 * backend (diskann_backend.py:345). */
int lm_index_set_hub_cache(lm_index *idx, const int32_t *ids, int32_t n, const float *d_embeddings);

/* hipStream_t all kernels of this index are enqueued on (default: the null stream). */
int lm_index_set_stream(lm_index *idx, void *hip_stream);

/* ---- search ---------------------------------------------------------------------------------
 * Mirrors faiss.SearchParametersHNSW as filled in hnsw_backend.py:203-234. */
typedef struct {
    int32_t efSearch;                /* complexity                               :206 */
    int32_t beam_size;               /* beam_width: pops per query per round     :207 */
    int32_t check_relative_distance; /* 0 for OpenAI-cosine models               :209-217 */
    float pq_pruning_ratio;          /* prune_ratio: two-level search (paper Alg. 2), needs lm_pq_attach; only the
                                        fraction 1-ratio of the candidates, ranked by PQ-ADC distance, is
                                        recomputed exactly.  0 = off                                    :220 */
    int32_t local_prune;             /* pruning_strategy == "local": rank this hop's neighbours only    :223-225 */
    float send_neigh_times_ratio;    /* > 1e-6: "proportional": quota from this hop's count, taken from the
                                        per-query approximate queue; else "global": everything unconsumed in
                                        the top (1-ratio) fraction of the approximate queue            :226-231 */
    int32_t batch_size;              /* "Neighbor processing batch size" :163,181,234 -- the paper's dynamic batching (section 4.2):
                                        > 0: after its beam_size pops a query keeps popping its best unexpanded candidate, one at a
                                        time and under the same stop rules, while the round's new-list (unvisited neighbours gathered
                                        so far) is shorter than batch_size -- fewer, fuller recompute forwards per search (a one-query
                                        search at efSearch 64: ~75 rounds of ~10 chunks -> ~20 rounds of ~64 at batch_size 64) for a
                                        few per cent more distance evaluations; the pops are chosen on the pool as it stood at the
                                        start of the round.  0 (the reference's default): off, results unchanged bit for bit.
                                        Rounds batch ACROSS queries as well, whatever this says.  oracle/lm_oracle.c restates it. */
    int32_t zmq_port;                /* accepted, unused: the encoder is in-process   :205 */
    int32_t recompute;               /* 1: use the provider, 0: use the attached table */
    int32_t max_batch;               /* queries in flight per pass (0 = default 4096) */
    int32_t recompute_memo;          /* 1 (default): within ONE pass of a search call (<= max_batch queries) every
                                        node is recomputed at most once -- fresh embeddings stay in HBM until the
                                        pass returns (N x d_padded x 4 bytes at most, grown on demand; results are
                                        identical, only nunique drops); a one-query pass skips it (its visited
                                        set already guarantees it).  0: dedup per lock-step round only, nothing
                                        kept between rounds.  Cf. the reference's own dedup_node_dis ("cache and
                                        reuse distance computations", diskann_backend.py:394,413,463). */
} lm_search_params;
void lm_search_params_default(lm_search_params *p);

/* Replaces index.search(n, swig_ptr(x), k, swig_ptr(D), swig_ptr(I), params)
 *                                                           hnsw_backend.py:241-248.
 * x: n x d fp32 queries (host).  distances: n x k fp32, labels: n x k int64, caller-allocated
 * (hnsw_backend.py:236-238).  l2: squared L2 ascending; inner product: +IP descending.
 * Unfilled slots: label -1, distance +inf (l2) / -inf (ip).
 * LDS rule of a CSR index: with maxnew = max(beam_size * largest level-0 degree, largest upper-level degree, 1) -- and, where
 * batch_size > 0, at least batch_size - 1 + largest level-0 degree -- and P(x) = the next power of two, a stored-embedding search
 * that the persistent launch serves (recompute = 0, no pq_pruning_ratio, batch_size = 0, beam_size <= 64, options "persistent_table" 1
 * and "update_variant" 0) needs (2 * max(efSearch, k) + P(maxnew)) * 8 + 4 * maxnew <= 150 KiB of LDS; every other search, and that
 * one where it needs more, runs the lock-step rounds, which need (2 * max(efSearch, k) + P(maxnew)) * 8 <= 64 KiB.  What fits neither
 * is LM_EINVAL (lm_last_error names the LDS), decided in 64-bit arithmetic before the search workspace is allocated or anything is launched: the
 * outputs are untouched and the handle serves the next call.  That covers any beam_size and batch_size up to INT32_MAX. */
int lm_index_search(lm_index *idx, int64_t n, const float *x, int32_t k, float *distances,
                    int64_t *labels, const lm_search_params *params);
/* Same with queries and results resident in HBM (no PCIe in the timed region). */
int lm_index_search_device(lm_index *idx, int64_t n, const float *d_x, int32_t k, float *d_distances,
                           int64_t *d_labels, const lm_search_params *params);

typedef struct {
    int64_t ndis;         /* (query,node) distance evaluations of the last search            */
    int64_t nunique;      /* embeddings requested from the provider (after cross-query dedup) */
    int64_t nrounds;      /* lock-step rounds                                                 */
    int64_t nexpand;      /* level-0 expansions                                               */
    int64_t update_launches; /* launches of the fused distance+beam-update kernel            */
    double update_ms;     /* summed HIP-event time of those launches (profiling on)          */
    double expand_ms;     /* summed HIP-event time of the expand(+uniq) kernels              */
    double provider_ms;   /* summed HIP-event time spent in provider work                    */
    int64_t nadc;         /* PQ-ADC evaluations of the two-level search (pq_pruning_ratio > 0) */
    double update_span_ms; /* profiling on: summed execution span (max end - min start over workgroups, device
                              wall clock) of the fused update kernel = what rocprofv3 reports as its duration */
    int64_t update_span_launches;
} lm_search_stats;
int lm_index_get_stats(const lm_index *idx, lm_search_stats *out);
int lm_index_set_profiling(lm_index *idx, int32_t enable); /* HIP events around kernels */
/* Mean event-pair time around an empty kernel (us): the fixed part of every update_ms/launch. */
int lm_index_event_overhead_us(lm_index *idx, double *out_us);
/* Tuning knobs (A/B measurements): "update_variant" 0 = auto (default), 3 / 4 = the fused distance + beam-update kernel with a
 * wave / a workgroup per query.  "persistent_table" 1 (default) = stored-embedding searches run as ONE persistent
 * launch per batch, 0 = lock-step rounds (a FILTERED stored-table search, lm_index_search_filtered*, runs the lock-step rounds whatever this says); "persistent_wave" -1 (auto) / 0 / 1 = its workgroup- or wave-per-query form.
 * "pq_threads" 256 / 512 / 1024 (default) = workgroup width of the PQ traversal.  "memo_initial_rows" = first allocation of the
 * per-call recompute memo in rows (0 = default: max(65536, 1024 per query of the pass)); it doubles on demand, never beyond N.
 * "pq_rerank_expanded" 0 (default) / 1: which set the DiskANN-style path's exact rerank ranks -- 0 the final candidate list (what
 * diskann_backend.py:444-449 describes: "fetch embeddings for the final candidate set only"), 1 EVERY node the traversal expanded
 * (upstream DiskANN's full_retset, PQFlashIndex::cached_beam_search: a superset of the final list; up to 4 x complexity <= 8192 nodes
 * per query are recorded, a query that expands more falls back to its final list and is counted in "pq_rerank_overflow").
 * "single_query_direct" 0 (default) / 1: a one-query recompute pass without a memo hands its new-list to the provider as it is (unique ids
 * in discovery order; three launches per round fewer: no request bitmap, no unique-list kernels); same results and counts.  Written after
 * round 4's GPU budget was spent: emulation-validated, not yet timed on hardware.
 * "speculate" S (0 = off, <= 64) / "speculate_max_batch" (default 2): speculative prefetch of a small recompute batch -- a round's forward
 * also embeds the unvisited neighbours of the S best candidates that are not expanded yet, into the per-call memo, so that later rounds
 * find their new nodes there and need no forward (a one-query search is ~100 rounds of ~50 dependent launches: launch latency).  Labels,
 * distances and distance-evaluation counts are those of S = 0; only the provider's request lists differ (more ids in fewer calls).
 * lm_index_get_option reads a value back ("pq_rerank_overflow": queries that fell back since the option was last set;
 * "filtered_allowed_evals": see lm_index_search_filtered). */
int lm_index_set_option(lm_index *idx, const char *name, int64_t value);
int lm_index_get_option(const lm_index *idx, const char *name, int64_t *value);

/* ---- DiskANN-style path: PQ-ADC traversal + deferred exact rerank ---------------------------------
 * Replaces _diskannpy.StaticDiskFloatIndex(metric, prefix, threads, cache, mechanism, zmq_port,
 * pq_prefix, partition_prefix)            leann_backend_diskann/diskann_backend.py:371-380
 * and  .batch_search(query, B, top_k, complexity, beam_width, num_threads, use_deferred_fetch,
 * skip_search_reorder, recompute_neighbors, dedup_node_dis, prune_ratio, batch_recompute,
 * use_global_pruning)                                                  diskann_backend.py:453-467.
 * The graph is the lm_index' level-0 graph entered at entry_point (the medoid for a Vamana graph);
 * lm_pq_attach adds the product quantiser: m sub-quantisers x 256 centroids x (d/m) floats and the
 * N x m code bytes (the role of <prefix>_pq_pivots.bin / _pq_compressed.bin).  Traversal uses PQ
 * distances only; with use_deferred_fetch the final candidate list (<= complexity per query) is
 * re-ranked with exact distances of embeddings fetched ONCE through the provider (:444-449); without
 * it, stored embeddings are used when attached, else the PQ order is returned. */
int lm_pq_attach(lm_index *idx, int32_t m, const float *codebooks, const uint8_t *codes, int64_t ntotal);
/* The same with the sub-quantisers' dimension ranges given explicitly -- the chunking of a stock DiskANN bundle
 * (<prefix>_pq_pivots.bin: 256 full-dimension pivots + centroid + chunk_offsets, diskann_backend.py:151-162): chunk j covers
 * dimensions [chunk_offsets[j], chunk_offsets[j+1]), lengths may differ and may be 0, chunk_offsets[m] <= d (trailing dimensions
 * carry no code: the augmentation coordinate of a MIPS bundle).  codebooks: chunk j's 256 centroids x len_j floats at float
 * offset 256 * chunk_offsets[j].  m % 4 == 0 (pad the code rows with empty chunks).  leann_amd/diskann_files.py converts the files. */
int lm_pq_attach_chunked(lm_index *idx, int32_t m, const int32_t *chunk_offsets, const float *codebooks, const uint8_t *codes,
                         int64_t ntotal);
typedef struct {
    int32_t complexity;          /* L: candidate list size                 :456 */
    int32_t beam_width;          /* W: nodes expanded per iteration (<=64) :457 */
    int32_t num_threads;         /* accepted, unused                       :459 */
    int32_t use_deferred_fetch;  /* = recompute_embeddings                 :450,460 */
    int32_t skip_search_reorder; /* return PQ order / distances            :461 */
    int32_t recompute_neighbors; /* must be 0 -- what the reference passes (:451,462); non-zero: LM_EINVAL */
    /* The four knobs below parametrise the PER-HOP neighbour recomputation of the fork's batch_search (which neighbours' exact distances
     * are recomputed, and how those recomputations are cached / batched).  The reference switches that recomputation OFF for every
     * search ("Do not recompute neighbor distances along the path", :444-451: recompute_neighors = False), so they cannot change its
     * results; here the traversal is PQ-only by construction and they are accepted and have NO effect (the Python host logs that
     * once when a non-default value arrives: leann_amd/backend.py).  The exact rerank is a single batch whatever batch_recompute says. */
    int32_t dedup_node_dis;      /* :463 inert (see above) */
    float prune_ratio;           /* :464 inert */
    int32_t batch_recompute;     /* :465 inert */
    int32_t use_global_pruning;  /* :466 inert */
} lm_pq_search_params;
void lm_pq_search_params_default(lm_pq_search_params *p);
int lm_pq_batch_search(lm_index *idx, int64_t n, const float *x, int32_t k, const lm_pq_search_params *params,
                       int64_t *labels, float *distances);
int lm_pq_batch_search_device(lm_index *idx, int64_t n, const float *d_x, int32_t k,
                              const lm_pq_search_params *params, int64_t *d_labels, float *d_distances);

/* ---- stand-alone kernels (parity tests, shard merge) ----------------------------------------
 * Distances of query row qidx[i] against embedding row ids[i] with the canonical reduction of
 * oracle/lm_oracle.c:orc_dist.  d_table rows have stride d_padded; d_q is nq x d_padded. */
int lm_dist_gather(const void *d_table, int32_t dtype, int32_t d_padded, int32_t metric,
                   const float *d_q, const int32_t *d_qidx, const int32_t *d_ids, int64_t npairs,
                   float *d_out, void *stream);
/* Per-query merge of S per-shard top-k lists (60M-chunk config; ids already global, -1 = empty):
 * in: S x B x k, out: B x k, ordered by (internal distance, id). */
int lm_topk_merge(const int64_t *d_in_ids, const float *d_in_dist, int32_t S, int32_t B, int32_t k,
                  int32_t metric, int64_t *d_out_ids, float *d_out_dist, void *stream);
/* Index build time: the select-neighbours heuristic of HNSW construction (Malkov & Yashunin Alg. 4 = faiss shrink_neighbor_list), which
 * faiss runs inside index.add under index.hnsw.efConstruction (leann_backend_hnsw/hnsw_backend.py:66-94) and the LEANN paper's Alg. 3
 * (high-degree-preserving pruning) calls again; n rows at once, every pairwise distance by the canonical reduction of
 * oracle/lm_oracle.c:orc_dist.
 *   d_table [ntable][d_padded]  fp32 or fp16 rows, zero padded (lm_dist_gather's layout);
 *   d_cand  [n][K]              candidate row ids, best first; an id < 0 or >= ntable is an EMPTY slot: never kept, never dereferenced;
 *   d_dist  [n][K]              the candidates' INTERNAL distances to their row's base node (squared L2, or -ip: smaller is closer),
 *                               taken as given, not recomputed;
 *   d_keep  [n][K]              out: 1 = kept, 0 = not.
 * Strict pass: scan j = 0 .. K-1; skip empty slots; stop keeping once m are kept; keep j unless some already kept i has
 * dist(cand[j], cand[i]) <= d_dist[j] (plain IEEE comparison: NaN never dominates).  Relaxed pass, only when alpha != 1 (DiskANN
 * occlude_list): scan the candidates not yet kept, in order, while fewer than m are kept, with thr[j] in place of d_dist[j], tested
 * against everything kept so far; a2 = alpha * alpha in fp32, thr = d / a2 (L2), thr = -(1.0f - (1.0f + d) / a2) (inner product of
 * unit vectors).  fp32 throughout, no contraction.
 * LM_EINVAL (before anything is launched): d_padded % 64 != 0 or a width the search kernels do not cover, K < 1 or K > LM_SELECT_MAX_K,
 * m < 1, alpha < 1 or not finite, n < 0.  n == 0: LM_OK.
 * LM_SELECT_MAX_K: the kept set is a K-bit mask in registers.  The batched builder reaches K = k_cand + 1 + cap = 193 at M = 32
 * (257 at M = 64) when it refines level 0, and 2 cap = 128 when it shrinks an overflowing list. */
#define LM_SELECT_MAX_K 512
int lm_select_neighbors(const void *d_table, int32_t dtype, int64_t ntable, int32_t d_padded, int32_t metric,
                        const int32_t *d_cand, const float *d_dist, int64_t n, int32_t K, int32_t m, float alpha,
                        uint8_t *d_keep, void *stream);
/* Index build time: link insertion.  faiss links every inserted node inside index.add (HNSW::add_link, which calls shrink_neighbor_list on
 * a list that overflows; leann_backend_hnsw/hnsw_backend.py:66-94); the batched builder adds a whole batch's forward and reverse edges at
 * once.  This call merges the directed edges src -> dst into the affected rows of one level's fixed-capacity adjacency, IN PLACE.
 * (csrc/lm_link_impl.h)
 *   d_table [n][d_padded]   fp32 or fp16 rows, zero padded (lm_select_neighbors' layout); row i = the vector of node i of this level;
 *   d_adj   [n][cap]        the level's adjacency; a slot value outside [0, n) is EMPTY (holes are tolerated);
 *   d_dist  [n][cap]        the INTERNAL distances of its links (squared L2, or -ip: smaller is closer);
 *   d_deg   [n]             OUTPUT only: the number of links of every row this call rewrites;
 *   d_src / d_dst / d_w [ne]   the edges to add; d_w holds internal distances, taken as given, not recomputed.
 * An edge is INVALID when src or dst is outside [0, n) or src == dst: it is ignored and never dereferenced.  A row is AFFECTED when it is
 * the src of at least one valid edge.  For every affected row v:
 *   1. Candidates: the non-empty slots c = 0 .. cap-1 of row v in slot order, each with d_dist[v][c]; then the valid edges e with
 *      src[e] == v in ascending e, each with d_w[e].
 *   2. Dedupe by dst, the first occurrence wins: an existing entry beats any incoming edge, among incoming edges the lowest e wins; the
 *      loser's weight is discarded even if it is smaller.
 *   3. Order by the key (internal distance, dst) ascending: NaN ranks as +inf, -0 as +0, ties go to the lower dst.
 *   4. Truncate to the first 2 * cap.
 *   5. If at most cap remain they are the new list as they stand (no selection, even if one dominates another: faiss add_link).  Otherwise
 *      the new list is what lm_select_neighbors' rule keeps with K = 2 * cap, m = cap on these candidates and their distances in this
 *      order: the strict pass, then the relaxed pass when alpha != 1; pairwise distances by the canonical reduction orc_dist, fp32
 *      throughout, no contraction.
 *   6. The kept entries go left-packed, in order, into d_adj[v] / d_dist[v] -- every distance with the bits it came with (a NaN stays that
 *      NaN, -0 stays -0) --, the remaining slots get -1 and +inf, d_deg[v] = the count.
 * Rows that are not affected are not written: every byte of their d_adj, d_dist and d_deg stays.  The result is a function of the input
 * bits alone (not of the order in which atomics land or rows are scheduled); no floating-point atomics.
 * A row may receive any number of edges.  LM_LINK_STAGE edges of a row are staged on chip at a time; larger rows take more passes over
 * their bucket and are just as exact.
 * Workspace: lm_graph_add_links_workspace_bytes(n, ne), a pure function of its arguments (0 for arguments the call rejects, and when
 * n == 0 or ne == 0: nothing is needed then).  d_workspace must be 4-byte aligned (it is carved into int32 / float arrays at multiples
 * of 256 bytes from its base; any hipMalloc'ed pointer is).
 * Cost that does not depend on the edges: one 1024-lane workgroup walks all n row counters on every call (1024 rows per step), and the row
 * kernel's grid is min(n, ne) workgroups, of which those beyond the number of affected rows leave at once.  Neither is measured yet at
 * n >> 1M; the builder calls this with n = one level's node count.
 * LM_EINVAL (before anything is launched, the buffers untouched): d_padded % 64 != 0 or a width the search kernels do not cover, unknown
 * dtype or metric, cap < 1 or 2 * cap > LM_SELECT_MAX_K, alpha < 1 or not finite, negative n or ne, n or ne > INT32_MAX, a NULL buffer
 * where one is needed, a d_workspace that is not 4-byte aligned, workspace_bytes below lm_graph_add_links_workspace_bytes(n, ne).  ne == 0 or n == 0: LM_OK, nothing is written. */
#define LM_LINK_STAGE 128
size_t lm_graph_add_links_workspace_bytes(int64_t n, int64_t ne);
int lm_graph_add_links(const void *d_table, int32_t dtype, int32_t d_padded, int32_t metric, int32_t *d_adj, float *d_dist,
                       int32_t *d_deg, int64_t n, int32_t cap, const int32_t *d_src, const int32_t *d_dst, const float *d_w, int64_t ne,
                       float alpha, void *d_workspace, size_t workspace_bytes, void *stream);
/* Index build time: high-degree-preserving pruning of the level-0 graph (LEANN paper, Algorithm 3): the few nodes most lists point at keep
 * their full lists, every other node re-selects at most m_low links, and every kept link is offered in both directions.  The reference
 * ships graphs pruned this way (its HNSW backend's is_compact / recompute index); here it is one call, nothing returns to the host.
 * (csrc/lm_prune_impl.h)
 *   d_table   [n][d_padded]  fp32 or fp16 rows, zero padded (lm_graph_add_links' layout);
 *   d_adj_in  [n][cap]       the level-0 adjacency in lm_graph_add_links' layout; read only;
 *   d_adj_out / d_dist_out [n][cap], d_deg_out [n]   out: the pruned level, EVERY row written; buffers other than the input;
 *   d_hubs    [n_hubs]       out, or NULL: the hubs, in the order of step 3;
 *   d_indeg   [n]            out, or NULL: the in-degrees of step 2.
 * The contract, per call:
 *   1. Usable slot: slot c of row v is usable when its value u is in [0, n) and u != v.  Every other slot is empty; holes are tolerated;
 *      duplicates within a row are taken as they are.
 *   2. In-degree: indeg[u] = the number of usable slots, over all rows, whose value is u.
 *   3. Hubs: H = the first n_hubs nodes under the key (indeg descending, id ascending) -- a total order: ties at the cut go to the lower id.
 *   4. Quota: quota[v] = cap for v in H, else mq = min(m_low, cap).
 *   5. Kept links and edges: row v keeps its first quota[v] usable slots in slot order.  With base[v] = the sum of quota[v'] over v' < v
 *      and (v, u) the r-th kept link of v, j = base[v] + r: edge 2j is v -> u, edge 2j + 1 is u -> v, both with the weight w = the canonical
 *      internal distance orc_dist of row v as the query and row u as the row (squared L2, or -ip; fp32, fp16 rows widened first; a NaN
 *      result is stored as the quiet NaN 0x7FC00000: IEEE 754 leaves the sign and payload of a computed NaN to the platform).  Every
 *      j < base[n] that no kept link fills (a row with fewer usable slots than its quota) gives two INVALID edges (src = dst = -1); nothing
 *      is dereferenced for them.  ne = 2 * base[n] = 2 * (n_hubs * cap + (n - n_hubs) * mq): a function of the arguments alone.
 *   6. Result: d_adj_out / d_dist_out / d_deg_out are what lm_graph_add_links leaves when it is called ONCE with these ne edges, this
 *      alpha, cap and table on an empty graph (every slot -1, every distance +inf, every degree 0): its steps 1-6 as stated above.  Rows
 *      that receive no valid edge stay empty with degree 0.  One call, not chunks: the result is a function of the input bits alone.
 * No floating-point atomics (integer atomics count, nothing else); no host synchronisation, allocation or device-to-host copy: everything
 * is enqueued on `stream`.
 * Workspace: lm_graph_prune_hubs_workspace_bytes(n, cap, m_low, n_hubs), a pure function of its arguments that includes
 * lm_graph_add_links_workspace_bytes(n, ne); 0 for arguments the call rejects and for n == 0.  d_workspace must be 8-byte aligned.
 * Cost that does not depend on the graph: one 1024-lane workgroup walks all n nodes once more than lm_graph_add_links does (hub ranks and
 * base[]); with d_hubs the hub keys are sorted by a bitonic network (one launch per step above 512 keys).
 * LM_EINVAL (before anything is launched, the buffers untouched): whatever lm_graph_add_links rejects for dtype, d_padded, metric, cap and
 * alpha; m_low < 1; n_hubs < 0 or > n; n < 0, n * cap > INT32_MAX or ne > INT32_MAX; a NULL d_table, d_adj_in, d_adj_out, d_dist_out,
 * d_deg_out or d_workspace; d_adj_out == d_adj_in; a misaligned d_workspace or workspace_bytes below the function above.  n == 0: LM_OK. */
size_t lm_graph_prune_hubs_workspace_bytes(int64_t n, int32_t cap, int32_t m_low, int64_t n_hubs);
int lm_graph_prune_hubs(const void *d_table, int32_t dtype, int32_t d_padded, int32_t metric, const int32_t *d_adj_in, int64_t n,
                        int32_t cap, int32_t m_low, int64_t n_hubs, float alpha, int32_t *d_adj_out, float *d_dist_out,
                        int32_t *d_deg_out, int32_t *d_hubs /* [n_hubs] or NULL */, int32_t *d_indeg /* [n] or NULL */,
                        void *d_workspace, size_t workspace_bytes, void *stream);
/* Index build time: ONE insert step of the batched HNSW builder on a view index -- search the level as it stands, form every row's
 * candidates, select neighbours, link both directions.  The reference does all of it inside faiss' index.add
 * (leann_backend_hnsw/hnsw_backend.py:66-94); the four calls above are its pieces, this call is the step that makes a builder of them, so
 * that a plain-C host can build an index and the glue between the kernels has a pinned result.  (csrc/lm_insert_impl.h)
 *   view     a handle from lm_index_create_view with a table attached (fp32 or fp16, owned or borrowed); n = its ntotal, cap = its
 *            levels[0].cap;
 *   d_batch  [b]        the node ids to insert (replace == 0) or to refine (replace == 1);
 *   d_adj    [n][cap]   the very pointer the view holds as level 0; d_dist [n][cap] and d_deg [n]: that level's other two arrays, in
 *                       lm_graph_add_links' layout;
 *   K = kk when replace == 0, kk + cap when replace == 1;
 *   d_cand_out / d_cdist_out / d_keep_out [b][K]   out, or NULL: the candidates of steps 3-5 and the keep mask of step 6.
 * Everything is enqueued on the index's stream (lm_index_set_stream).  The index owns every intermediate buffer (queries, search result,
 * candidates, keep mask, edges, the link insertion's workspace): they grow on demand and are freed with the index; a call that rejects its
 * arguments allocates nothing.
 * The contract, per call and for every row i of the batch, v = d_batch[i]:
 *   1. Query: the table row of v as fp32 -- its first d values, fp16 widened exactly.  v outside [0, n): the row is VOID; its query is all
 *      zeros, nothing is dereferenced for it, its candidates are all empty, it emits only invalid edges and clears nothing.
 *   2. Search: S(i) = the kk (label, distance) pairs that lm_index_search_device(view, b, queries, kk, ..., params) returns for that query:
 *      the view's own search, bit for bit, with every rule and rejection of a view search, on the level as it stands when the call begins.
 *      The INTERNAL distance of an entry is squared L2, or the negated inner product: the exact negation of what the search decodes.
 *   3. Candidates, replace == 0: the kk entries of S(i) in the order returned (a label outside [0, n) is empty).
 *   4. Candidates, replace == 1: the concatenation of S(i), with every entry whose label is v (or outside [0, n)) made empty, and the cap
 *      slots of row v of d_adj / d_dist in slot order (a slot value outside [0, n) is empty).  Dedupe by id: the first occurrence in the
 *      concatenation survives -- a search entry beats a stored slot --, later ones become empty.  The non-empty entries are ordered by the
 *      key (internal distance ascending, position in the concatenation ascending), -0 counting as +0; empty entries follow.  Every row is
 *      read as it was when the call began.
 *   5. Non-finite distances: in both modes an entry whose internal distance is not finite (+-inf, NaN) is empty.  In step 4 it is dropped
 *      after the dedupe (it still shadows the later occurrences of its id) and before the ordering.  Empty entries have id -1 and distance
 *      +inf; every other entry keeps the distance bits it came with.  d_cand_out / d_cdist_out receive exactly these K entries per row.
 *   6. Selection: keep[i][.] = what lm_select_neighbors leaves for (cand, dist, K, m, alpha) on the view's table: its rule as it stands,
 *      the strict pass, then the relaxed pass when alpha != 1.  d_keep_out receives it.
 *   7. Edges: ne = 2 * b * m.  With (v, u, w) the r-th kept candidate of row i in candidate order (r < m): edge i * m + r is v -> u with
 *      weight w, edge b * m + i * m + r is u -> v with weight w; every other edge index is INVALID (src = dst = -1).  The valid edges thus
 *      come as all forward edges row-major, then all reverse edges, and lm_graph_add_links' tie rule "the lowest e wins" decides on them.
 *   8. Clearing: when replace == 1 every non-void row v of the batch is cleared (adj -1, dist +inf, deg 0), after all candidates have been
 *      formed and before step 9.
 *   9. Linking: d_adj / d_dist / d_deg become what lm_graph_add_links leaves when called ONCE with these ne edges, this alpha, cap and
 *      table: its steps 1-6 as written.  Rows that receive no valid edge and were not cleared keep every byte.
 * Duplicate ids in d_batch are tolerated: every occurrence is processed as stated (the edges repeat and step 9 dedupes them, clearing is
 * idempotent); the result is still a function of the input bits alone.
 * No floating-point atomics; no host synchronisation, allocation inside the kernels, or device-to-host copy other than what the view
 * search itself does (its one counter read per pass); lm_index_get_stats afterwards reads as after that search.
 * Rejections, each before anything is staged or launched, all buffers untouched.  LM_EINVAL: a NULL handle, params or level array, NULL
 * d_batch with b > 0; b < 0 or 2 * b * m > INT32_MAX; replace not 0 or 1; kk < 1, m < 1, K > LM_SELECT_MAX_K; whatever lm_graph_add_links
 * rejects for cap and alpha; d_adj different from the view's level-0 array.  LM_ESTATE: a handle that is not a view; no table attached.
 * Everything the view search rejects for params and k = kk comes back with the search's own code (recompute, batch_size,
 * pq_pruning_ratio, the LDS rule, beam_size > 64, option persistent_table 0).  b == 0: LM_OK, nothing is written. */
int lm_graph_insert_batch(lm_index *view, const int32_t *d_batch, int64_t b, int32_t replace, int32_t kk, int32_t m, float alpha,
                          const lm_search_params *params, int32_t *d_adj, float *d_dist, int32_t *d_deg,
                          int32_t *d_cand_out /* [b][K] or NULL */, float *d_cdist_out /* [b][K] or NULL */, uint8_t *d_keep_out /* [b][K] or NULL */);
/* Exact top-k over a stored-embedding table = oracle/lm_oracle.c:orc_bruteforce_topk (the paper's IndexFlatIP baseline) plus an allow-list.  The
 * reference has no such path: leann/api.py:785-790 applies metadata_filters AFTER the graph search, so a filtered query returns fewer than top_k
 * hits; here the filter is part of the scan and the result is the best k of the allowed rows.  (csrc/lm_exact_impl.h)
 *   d_table [ntable][d_padded]  fp32 or fp16 rows, zero padded (lm_dist_gather's layout);
 *   d_q     [nq][d_padded]      fp32, zero padded;
 *   d_allow                     NULL = every row, else ceil(ntable / 32) words: row i takes part iff bit i & 31 of d_allow[i >> 5] is set; bits at
 *                               positions >= ntable of the last word are ignored, whatever their value;
 *   d_distances / d_labels [nq][k]   out: squared L2 ascending, or +ip descending; slots beyond the number of participating rows get label -1
 *                               and distance +inf (L2) / -inf (ip).
 * The contract is the arithmetic.  Every (query, row) distance is the canonical reduction orc_dist (16 lanes per row, four fmaf chains per lane,
 * xor-8/4/2/1 butterfly; internal distance = squared L2 or -ip), no matrix cores, no other summation order.  Ranking is by the key
 * (internal distance, id) ascending: NaN ranks as +inf, -0 as +0, ties go to the lower id.  Returned distances are what the key decodes to
 * (L2: the key's distance; ip: its negation, so an inner product of exactly 0 comes back as -0.0, as from the oracle).  The result depends on the
 * input bits only: however the rows are cut into slices, labels and distance bits are the same.
 * Slicing (a pure function of ntable and nq, never of the device): nqt = max(1, ceil(nq / 8)) query tiles;
 * s0 = clamp(ceil(ntable / 1024), 1, max(1, 512 / nqt)); rows per slice = max(32, ceil(ntable / s0) rounded up to a multiple of 32);
 * S = max(1, ceil(ntable / rows)) slices.  One query: ntable <= 1024 is one slice, 1025..2048 two, 20000 twenty (the last of 544 rows).
 * The workspace holds the S partial lists per query: lm_exact_search_workspace_bytes = S * nq * k * 8.
 * LM_EINVAL (before anything is launched): d_padded % 64 != 0 or a width the search kernels do not cover, unknown dtype or metric, k < 1 or
 * k > LM_EXACT_MAX_K, negative nq / ntable, ntable > INT32_MAX, a NULL buffer where one is needed, workspace_bytes below
 * lm_exact_search_workspace_bytes(ntable, nq, k).  nq == 0: LM_OK.  ntable == 0: every slot gets the empty values. */
#define LM_EXACT_MAX_K 256
size_t lm_exact_search_workspace_bytes(int64_t ntable, int64_t nq, int32_t k);
int lm_exact_search(const void *d_table, int32_t dtype, int64_t ntable, int32_t d_padded, int32_t metric, const float *d_q, int64_t nq,
                    int32_t k, const uint32_t *d_allow, float *d_distances, int64_t *d_labels, void *d_workspace, size_t workspace_bytes,
                    void *stream);
/* The same on the index's attached table (library-owned or borrowed), on the index's stream, with a workspace the index owns (apart from the
 * graph search's).  Queries are [n][d], as for lm_index_search*; `allow` of the host form is a HOST array (or NULL), uploaded per call.
 * LM_ESTATE without an attached table. */
int lm_index_search_exact(lm_index *idx, int64_t n, const float *x, int32_t k, const uint32_t *allow, float *distances, int64_t *labels);
int lm_index_search_exact_device(lm_index *idx, int64_t n, const float *d_x, int32_t k, const uint32_t *d_allow, float *d_distances,
                                 int64_t *d_labels);
/* Filtered graph search: lm_index_search with an allow-list, for the index that has neither a stored table (lm_index_search_exact) nor PQ codes
 * (lm_pq_flat_search) -- a pruned HNSW graph searched with selective recompute -- and for any other index lm_index_search serves.  faiss filters
 * inside the graph search (HNSW::search_from_candidates with an IDSelector): every evaluated node steers the walk, only selected nodes enter the
 * result heap.  The reference filters AFTER the search (leann/api.py:785-790) and keeps what is left of the pool.  (csrc/lm_filter_impl.h)
 *   allow / d_allow   lm_exact_search's layout and rules: NULL = every node, else ceil(ntotal / 32) words, ONE bitmap for the whole call; node i may
 *                     enter the result iff bit i & 31 of word i >> 5 is set; bits at positions >= ntotal are ignored, whatever their value.  The
 *                     host form takes a HOST array, uploaded per call into a buffer the index owns and grows; the device form borrows the caller's.
 * Contract.  For each query let E be the set of nodes whose exact distance the level-0 beam search evaluates: the seed that the upper-level
 * descent hands to level 0, and every node that enters a new-list while the query is in its beam phase (dynamic batching's extra pops
 * included).  Nodes evaluated only during the upper-level descent are not in E.  The result is the best k of E n allowed under the key (internal
 * distance, id) ascending -- NaN ranks as +inf, -0 as +0, ties go to the lower id --, decoded as lm_index_search decodes a pool key (ip: the
 * negation, so an inner product of exactly 0 comes back as -0.0); slots beyond |E n allowed| get label -1 and +inf (L2) / -inf (ip).
 * The walk is exactly that of lm_index_search with the same params: pops, stop rules, batch_size, beam_size, the memo, the hub cache and
 * "speculate" -- the allow-list never influences it.  Hence
 *   1. with allow == NULL or a bitmap of all ones, labels and distance bits are those of lm_index_search (its pool keeps the best
 *      max(efSearch, k) of E);
 *   2. with any allow-list, ndis, nexpand, nrounds, nunique and the provider's per-round request lists are those of lm_index_search;
 *   3. a query's result does not depend on the other queries of the call, nor on how max_batch cuts the call into passes.
 * A selective filter can still return FEWER than k hits: only nodes the walk evaluates can be returned, and the walk goes where the query
 * is, not where the allowed nodes are.  The remedy is a larger efSearch, or lm_index_search_exact / lm_pq_flat_search where the index has a
 * table / PQ codes: those rank every allowed row.
 * Both sources: params->recompute = 1 (provider: with and without the per-call memo, with a hub cache, built-in or foreign provider) and
 * recompute = 0 (attached fp32 / fp16 table; the lock-step rounds, not the persistent launch).  Each allowed node's distance is computed a
 * second time by the collecting kernel, from the row the round has just fetched.
 * Rejections come before anything is staged or launched, the outputs stay untouched: LM_EINVAL for everything lm_index_search rejects (NULL
 * index / params / buffer, n < 0, k < 1, efSearch < 1, batch_size < 0) and for pq_pruning_ratio > 0 (the two-level search does not evaluate
 * every new node exactly: E is not defined there); LM_ESTATE as for lm_index_search (recompute without a provider, recompute = 0 without a
 * table).  n == 0: LM_OK.  An empty index: every slot gets the empty values.
 * Stats: lm_index_get_stats as after lm_index_search (same meaning, same values -- nrounds included: where lm_index_search would run the
 * persistent stored-table launch, a call cut into passes by max_batch reports its longest pass there and here);  lm_index_get_option(idx, "filtered_allowed_evals", &v) reads,
 * for the last filtered call, the number of (query, node) pairs that passed the allow test = the sum of |E n allowed| over the queries.
 * The index owns the result lists' workspace, apart from the other paths'. */
int lm_index_search_filtered(lm_index *idx, int64_t n, const float *x, int32_t k, const uint32_t *allow, float *distances, int64_t *labels,
                             const lm_search_params *params);
int lm_index_search_filtered_device(lm_index *idx, int64_t n, const float *d_x, int32_t k, const uint32_t *d_allow, float *d_distances,
                                    int64_t *d_labels, const lm_search_params *params);
/* Flat PQ scan: the L best rows of an N x m code array by ADC distance, with an allow-list -- the filtered search of an index that stores no
 * embeddings (it keeps its PQ codes and the recompute provider).  No graph is walked, so a filter cannot disconnect it, and the allow-list is
 * part of the scan: rejected rows are never loaded.  (csrc/lm_pq_flat_impl.h)
 *   d_codes [ntotal][m]          code bytes (lm_pq_attach's layout), 4-byte aligned (the rows are read as dwords; 16-byte alignment lets
 *                                the kernel fetch a row as 16-byte pieces at m = 16, 32, 48, 64, 96, 128);
 *   chunk_offsets                HOST array of m + 1 offsets by the rules of lm_pq_attach_chunked (chunk_offsets[m] <= d), NULL = uniform d / m;
 *   d_codebooks                  lm_pq_attach's layout: chunk j's 256 centroids x len_j floats at float offset 256 * chunk_offsets[j];
 *   d_q [nq][ldq]                fp32 queries, ldq >= d;
 *   d_allow                      lm_exact_search's layout and rules (NULL = every row; bits at positions >= ntotal are ignored);
 *   d_distances / d_labels [nq][L]   out: ADC distance ascending (L2) or its negation descending (ip), decoded as k_finalize decodes a pool key;
 *                                slots beyond the number of participating rows get label -1 and +inf (L2) / -inf (ip).
 * The contract is the arithmetic of oracle/lm_oracle_pq.c.  Lookup table (orc_pq_lut): LUT[j][c] = the sequential fmaf sum over the chunk's
 * dimensions of (q - centroid)^2 (L2) or of q * centroid, negated (ip); a zero-length chunk gives 0 (-0 under ip).  Distance (orc_pq_adc):
 * adc = (p0 + p1) + (p2 + p3), p_r = the sequential fp32 sum over j = r, r + 4, ... of LUT[j][code[j]]; no other order, no contraction.
 * Ranking is by the key (adc, id) ascending: NaN ranks as +inf, -0 as +0, ties go to the lower id.  The result depends on the input bits
 * only: however the rows are cut into slices, labels and distance bits are the same.
 * Slicing (a pure function of ntotal, nq, m and L, never of the device):
 *   per_q = 1024 m + 16 L + 10240 bytes of LDS per query (its table, two lists of L keys, 1280 pending keys);
 *   qt    = min(8, floor(161792 / per_q)) queries per tile (one at m = 96, two at m = 48, eight at m = 8 and L <= 112);
 *   nqt   = max(1, ceil(nq / qt)) query tiles;  s0 = clamp(ceil(ntotal / 2048), 1, max(1, 512 / nqt));
 *   rows per slice = max(32, ceil(ntotal / s0) rounded up to a multiple of 32);  S = max(1, ceil(ntotal / rows)) slices.
 * One query: ntotal <= 2048 is one slice, 2049 .. 4096 two, 4097 three, 20000 ten (nine of 2016 rows and a last one of 1856), 1M rows 489
 * of 2048.  The workspace holds the S partial lists per query: lm_pq_scan_workspace_bytes = S * nq * L * 8 (0 for arguments lm_pq_scan rejects).
 * LM_EINVAL (before anything is launched): m < 1, m % 4 != 0 or m > 4096; offsets that do not start at 0, decrease or end past d; uniform
 * layout with d % m != 0; ldq < d; L < 1 or L > LM_PQ_FLAT_MAX_L; qt == 0 (table + lists do not fit the 160 KB LDS); unknown metric; negative
 * nq / ntotal, ntotal > INT32_MAX; d_codes not 4-byte aligned; a NULL buffer where one is needed; workspace_bytes below lm_pq_scan_workspace_bytes(ntotal, nq, m, L).
 * nq == 0: LM_OK.  ntotal == 0: every slot gets the empty values. */
#define LM_PQ_FLAT_MAX_L 1024
size_t lm_pq_scan_workspace_bytes(int64_t ntotal, int64_t nq, int32_t m, int32_t L);
int lm_pq_scan(const uint8_t *d_codes, int64_t ntotal, int32_t m, const int32_t *chunk_offsets, const float *d_codebooks, int32_t d,
               int32_t metric, const float *d_q, int64_t nq, int32_t ldq, int32_t L, const uint32_t *d_allow, float *d_distances,
               int64_t *d_labels, void *d_workspace, size_t workspace_bytes, void *stream);
/* The same on the index's attached quantiser and stream, followed by the tail of lm_pq_batch_search: L = max(params->complexity, k) rows
 * per query come out of the scan; with use_deferred_fetch and a provider they are re-ranked by exact distances of embeddings fetched in
 * ONE provider call (the sorted unique union of the lists), else by the stored table if there is one, else -- or with skip_search_reorder --
 * the PQ order stands; then the best k go out.  beam_width and the inert knobs are accepted and unused; recompute_neighbors != 0: LM_EINVAL.
 * `allow` of the host form is a HOST array (or NULL), uploaded per call.  LM_EINVAL also for complexity < 1, k < 1, max(complexity, k) >
 * LM_PQ_FLAT_MAX_L or a scan state that does not fit the LDS (lm_pq_scan's rule).  LM_ESTATE without attached codes, or when deferred fetch is
 * asked for with neither a provider nor a table.  Every rejection comes before anything is staged or launched: the outputs stay untouched.  Stats: ndis = ADC evaluations (allowed rows x queries), nunique = rows requested from the
 * provider, nrounds = 1, nexpand = 0.  The index owns the scan's workspace, apart from the other paths'. */
int lm_pq_flat_search(lm_index *idx, int64_t n, const float *x, int32_t k, const lm_pq_search_params *params, const uint32_t *allow,
                      int64_t *labels, float *distances);
int lm_pq_flat_search_device(lm_index *idx, int64_t n, const float *d_x, int32_t k, const lm_pq_search_params *params,
                             const uint32_t *d_allow, int64_t *d_labels, float *d_distances);
/* Filtered PQ traversal: lm_pq_batch_search with an allow-list -- the filter applied INSIDE the DiskANN-style walk, as faiss and
 * lm_index_search_filtered apply theirs: every evaluated node steers the search, only allowed nodes enter the result.  The reference filters
 * AFTER the search (leann/api.py:785-790) and keeps the allowed among the L of the final list; lm_pq_flat_search ranks every allowed row but
 * reads the whole code array per query tile.  (csrc/lm_pq_impl.h: k_pq_traverse<NTH, true>)
 *   allow / d_allow   lm_exact_search's layout and rules: NULL = every node, else ceil(ntotal / 32) words, ONE bitmap for the whole call; bits at
 *                     positions >= ntotal are ignored, whatever their value.  The host form takes a HOST array, uploaded per call into a buffer
 *                     the index owns and grows (lm_index_search_filtered's); the device form borrows the caller's.
 * Contract.
 *   The walk.  It is exactly lm_pq_batch_search's with the same params: the lookup table, the entry point, the visited set, the W closest
 *     unexpanded entries of the list of L = max(complexity, k), the stop rule.  The allow-list never influences the walk.
 *   The evaluated set E(q): every node whose ADC distance the traversal computes -- the entry point and every fresh node of every hop.
 *     |E(q)| is the query's share of ndis.
 *   The allowed candidates F(q): the first L of E(q) n allowed under the key (adc, id) ascending -- NaN ranks as +inf, -0 as +0, ties go to
 *     the lower id.
 *   The tail: lm_pq_batch_search's, applied to F in place of the final list.  With use_deferred_fetch and a provider there is ONE provider
 *     call per pass, for the sorted unique union of the F lists; otherwise the stored table is used if one is attached; otherwise -- or with
 *     skip_search_reorder -- the PQ order stands.  Then the best k go out; empty slots get label -1 and +inf (L2) / -inf (ip).
 *   Option "pq_rerank_expanded" has NO effect on this call: F is what gets ranked.
 * Hence
 *   1. with allow == NULL or a bitmap of all ones, labels and distance bits are those of lm_pq_batch_search at "pq_rerank_expanded" 0 (its
 *      final list is the best L of E);
 *   2. with any allow-list, ndis, nexpand and nrounds are those of lm_pq_batch_search; nunique is the number of rows requested for F;
 *   3. a query's result does not depend on the other queries of the call, nor on how the call is cut into passes.
 * A selective filter can still return FEWER than k hits: only nodes the walk evaluates can be returned (lm_pq_flat_search ranks every
 * allowed row).  lm_index_get_option(idx, "filtered_allowed_evals", &v) reads, after this call too, the sum of |E(q) n allowed| over the
 * queries; with allow == NULL it equals ndis.
 * LDS rule.  The kernel keeps the lookup table, the walk's list and merge output, the hop's new keys and ids, the allowed-only list and FS
 * staging keys in one workgroup's LDS.  FS = 64 for every (m, L, W, level-0 degree): a constant, so that the rule below is linear in L.  With
 * new = max(W * max level-0 degree, 1) (the workspace's size; a graph with upper levels: at least their largest degree) and P(new) = new rounded up to a power of two, the call needs
 *     1024 m + 24 L + 8 P(new) + 4 new + 8 FS  <=  161792 bytes (158 KiB)
 * (lm_pq_batch_search: 1024 m + 16 L + 8 P(new) + 4 new).  At m = 96, W = 64, degree 64: L <= 576.
 * Rejections come before anything is staged or launched, the outputs stay untouched: everything lm_pq_batch_search rejects, with the same
 * codes (LM_EINVAL: NULL index / params / buffer, n < 0, k < 1, complexity < 1, recompute_neighbors != 0, beam_width > 64, more than 8192
 * candidates per query into an exact rerank; LM_ESTATE: no codes attached, deferred fetch with neither a provider nor a table), and
 * LM_EINVAL when the state does not fit the LDS by the rule above.  n == 0: LM_OK.  An empty index: every slot gets the empty values.
 * All three workgroup widths of option "pq_threads" give the same bits. */
int lm_pq_batch_search_filtered(lm_index *idx, int64_t n, const float *x, int32_t k, const lm_pq_search_params *params,
                                const uint32_t *allow, int64_t *labels, float *distances);
int lm_pq_batch_search_filtered_device(lm_index *idx, int64_t n, const float *d_x, int32_t k, const lm_pq_search_params *params,
                                       const uint32_t *d_allow, int64_t *d_labels, float *d_distances);
/* Index build time: the product quantiser that lm_pq_attach / lm_pq_attach_chunked take, made by the library -- nearest-centroid
 * assignment (lm_pq_encode) and Lloyd iterations over a sample (lm_pq_train); the role of DiskANN's generate_pq_pivots /
 * generate_pq_data_from_pivots behind diskann_backend.py:105-111 (leann_amd/pq.py holds the torch forms).
 *   d_x            n (or s) rows of fp32 or fp16 with row stride ld elements (ld >= d): a raw [n][d] array and the zero-padded
 *                  stored-embedding table are both passed as they are;
 *   chunk_offsets  HOST array of m + 1 ints: chunk j covers dimensions [chunk_offsets[j], chunk_offsets[j+1]), lengths may differ
 *                  and may be 0, chunk_offsets[m] <= d; NULL = the uniform layout, m chunks of d / m;
 *   d_codebooks    lm_pq_attach's layout exactly: chunk j's 256 centroids x len_j floats at float offset 256 * chunk_offsets[j]
 *                  (uniform: [m][256][d/m]); lm_pq_train reads the initial centroids from it and writes the trained ones to it;
 *   d_codes        out, [n][m] bytes.
 * The contract is the arithmetic.  Assignment (both entry points), chunk j of row v, ALWAYS squared L2 whatever the index metric (as in
 * faiss and DiskANN):  dist_c = acc after { acc = 0.0f; for t = 0 .. len_j - 1: diff = x[lo + t] - cb[c][t]; acc = fmaf(diff, diff, acc) }
 * for c = 0 .. 255 -- oracle/lm_oracle_pq.c:orc_pq_lut's L2 form with the row as the query, fp16 rows widened first (exact) --; then
 * { code = 0; best = +inf; for c ascending: if (dist_c < best) { best = dist_c; code = c; } }: ties go to the lowest c, a NaN distance never
 * wins, a chunk whose distances are all NaN or whose length is 0 gets code 0.
 * Update (lm_pq_train, after each assignment): for every (j, c) with count > 0 and every coordinate t,
 * { sum = 0.0f; for rows v ASCENDING with code[v][j] == c: sum = sum + x[v][lo + t]; }  cb[c][t] = sum / (float)count -- IEEE fp32, no
 * contraction; a centroid with count == 0 stays as it was.  `iters` rounds of assignment + update; iters == 0 leaves the codebooks
 * untouched.  No floating-point atomics: the trained codebooks are a function of the input bits alone.
 * LM_EINVAL (before anything is launched): a NULL buffer with n > 0, an unknown dtype, ld < d, m < 1 or m > 4096, uniform layout with
 * d % m != 0, chunk_offsets[0] != 0, decreasing offsets, chunk_offsets[m] > d, a chunk longer than LM_PQ_MAX_SUB (a chunk's 256
 * centroids then fit in 64 KB of LDS), negative n / s / iters, workspace_bytes < lm_pq_train_workspace_bytes(s, d, m).
 * n == 0 / s == 0: LM_OK.  m % 4 is NOT required here (lm_pq_attach requires it: padding the code rows stays the caller's job). */
#define LM_PQ_MAX_SUB 64
int lm_pq_encode(const void *d_x, int32_t dtype, int64_t n, int32_t ld, int32_t d, int32_t m, const int32_t *chunk_offsets,
                 const float *d_codebooks, uint8_t *d_codes, void *stream);
int lm_pq_train(const void *d_x, int32_t dtype, int64_t s, int32_t ld, int32_t d, int32_t m, const int32_t *chunk_offsets,
                int32_t iters, float *d_codebooks, void *d_workspace, size_t workspace_bytes, void *stream);
size_t lm_pq_train_workspace_bytes(int64_t s, int32_t d, int32_t m);

/* ---- fused encoder elementwise ops ---------------------------------------------------------------
 * out = LayerNorm(x + residual) * gamma + beta over the last dim; fp16 in/out, fp32 arithmetic;
 * residual may be NULL.  Part of the BERT forward inside compute_embeddings
 * (leann/embedding_compute.py:229-239).  The GEMMs and the attention of that forward are the hand-written MFMA kernels below
 * (hidden 384: lm_qkv_h384_f16, lm_attn_varlen_hd32_f16, lm_layer_tail_h384_f16); no library call is on the default path. */
int lm_add_layernorm_f16(const void *d_x, const void *d_residual, const void *d_gamma, const void *d_beta,
                         void *d_out, int64_t rows, int32_t hidden, float eps, void *stream);

/* Fused self-attention for packed variable-length sequences, head_dim 32 (hidden = heads*32), lengths 1..256:
 * d_qkv [total_tokens][3][heads][32] fp16 (the QKV GEMM output), d_cu_seqlens int32[n_seqs+1],
 * d_out [total_tokens][heads*32] fp16.  softmax(QK^T/sqrt(32))V per (sequence, head), MFMA 32x32x16 f16. */
int lm_attn_varlen_hd32_f16(const void *d_qkv, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t heads,
                            int32_t max_len, void *d_out, void *stream);

/* The same kernel for head_dim 32 or 64 (hidden = heads * head_dim; 64: bge-base / contriever, lengths 1..512; 32: lengths 1..256):
 * d_qkv [total_tokens][3][heads][head_dim] fp16, d_out [total_tokens][heads * head_dim] fp16. */
int lm_attn_varlen_f16(const void *d_qkv, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t heads, int32_t head_dim,
                       int32_t max_len, void *d_out, void *stream);

/* Embedding front end in one pass: d_out[r] = LayerNorm(half(word[tok[r]] + type0) + pos_table[pos[r]]);
 * tables and output fp16, hidden <= 768.  Replaces the three gathers/adds before the embedding LayerNorm of
 * the BERT forward (leann/embedding_compute.py:229-239).  On the Python host's default path (LEANN_MI355X_EMBED=0 selects
 * the torch ops for A/B runs). */
int lm_embed_layernorm_f16(const int32_t *d_tok, const int32_t *d_pos, const void *d_word, const void *d_pos_table,
                           const void *d_type0, const void *d_gamma, const void *d_beta, void *d_out, int64_t rows,
                           int32_t hidden, float eps, void *stream);

/* Packing front end: padded token ids [n][t] + lengths + cumulative lengths (int32[n+1]) -> packed token ids and
 * positions [total].  Replaces the masked selects before the first encoder layer.  On the default path (LEANN_MI355X_PACK=0 = torch ops, A/B). */
int lm_pack_tokens(const int32_t *d_ids, const int32_t *d_lens, const int32_t *d_cu_seqlens, int32_t n, int32_t t,
                   int32_t *d_tok, int32_t *d_pos, void *stream);

/* Mean pooling over the tokens of each packed sequence (+ optional L2 normalisation), fp16 in, fp32 out
 * [n_seqs][hidden]; fixed summation order (deterministic).  sentence-transformers Pooling as done in
 * leann/embedding_compute.py:323-334.  On the default path (LEANN_MI355X_POOL=0 = torch ops, A/B). */
int lm_meanpool_varlen_f16(const void *d_x, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t hidden,
                           int32_t normalize, float *d_out, void *stream);

/* The second half of a BERT layer with hidden size 384 in ONE kernel (csrc/lm_layer_tail_h384.hip) -- attention output projection,
 * residual, LayerNorm, then the feed-forward block with its residual and LayerNorm:
 *   x     = LayerNorm(resid + attn W_o^T + b_o) * gamma1 + beta1          (never written to HBM)
 *   d_out = LayerNorm(x + GELU(x W1^T + b1) W2^T + b2) * gamma + beta,    attn / resid / d_out [tokens][384] fp16,
 * biases fp32, GELU = exact erf form, MFMA 32x32x16 f16 with the ffn-wide intermediate held in accumulators (never written to HBM).
 * The three weight matrices are passed as ready-made LDS IMAGES (written once per model by lm_layer_tail_pack_h384), so that the
 * kernel's weight stream is a linear LDS-DMA copy, and the two products of the feed-forward block alternate MFMA by MFMA on single
 * accumulator chains (no partial sums, no stage arithmetic: ~290 instructions per 48 MFMAs on its one wave per SIMD).  ffn a multiple
 * of 192 in [192, 1728]; other shapes: the general GEMM path (lm_gemm_f16).  DEFAULT path of the hidden-384 forward
 * (LEANN_MI355X_TAIL=0 in the Python host = lm_gemm_ws_h384_f16 + lm_add_layernorm_f16 + lm_gemm_f16 x 2 + lm_add_layernorm_f16, A/B).
 * Part of the BERT forward in compute_embeddings (leann/embedding_compute.py:229-239).  (Generations 1-3 of this kernel are history:
 * generation 3 survives only in the diagnosis build, csrc/diag/, as scripts/kbench.cpp's A/B reference.) */
int lm_layer_tail_h384_f16(const void *d_attn, const void *d_resid, const void *d_wo_img, const float *d_bo,
                           const void *d_gamma1, const void *d_beta1, float eps1, const void *d_w1_img, const float *d_b1,
                           const void *d_w2_img, const float *d_b2, const void *d_gamma, const void *d_beta, void *d_out,
                           int64_t tokens, int32_t ffn, float eps, void *stream);
/* d_wo_slabs = W_o as [12][384][32] (slab s = input features 32 s .. 32 s + 31, natural order: leann_amd/encoder.py pack_wo_slabs),
 * d_w1_acc = W1 [ffn][384] with its COLUMNS in accumulator order (pack_w1_acc_order), d_w2_slabs = W2 as [ffn/32][384][32] with the k
 * order of fused_mlp_k_permutation (pack_w2_fused_mlp) -> the images lm_layer_tail_h384_f16 streams (same sizes; XOR-swizzled 16-byte chunks: what makes the
 * kernel's ds_read_b128 fragment reads bank-conflict free).  Device to device, on `stream`. */
int lm_layer_tail_pack_h384(const void *d_wo_slabs, const void *d_w1_acc, const void *d_w2_slabs, int32_t ffn, void *d_wo_img,
                            void *d_w1_img, void *d_w2_img, void *stream);

/* The FIRST half of a BERT layer with hidden size 384 = 12 heads x 32 in ONE kernel (csrc/lm_qkv_attn_h384.hip, round 6): QKV projection fused into
 * self-attention -- d_out[tokens][384] = concat_h softmax(Q_h K_h^T / sqrt(32)) V_h with [Q | K | V] = x W_qkv^T + b_qkv computed per (sequence, head)
 * on chip: Q, K, V never go to HBM (as two kernels they were a 604 MB write + 604 MB read per 262 k tokens around 201 MB of x and 201 MB of output).
 * d_x [tokens][384] fp16 packed sequences, d_cu_seqlens int32[n_seqs + 1], lengths 1..256; d_wqkv_img = lm_qkv_pack_h384's image of the nn.Linear
 * weight [1152][384] (rows W_q | W_k | W_v), d_bqkv fp32[1152].  Replaces the model.encode() call's per-layer QKV GEMM + attention
 * (leann/embedding_compute.py:229-239) on large hidden-384 forwards of long sequences (lm_h384_first_half_form below says when); the stand-alone pair stays
 * the default elsewhere. */
int lm_qkv_attn_h384_f16(const void *d_x, const void *d_wqkv_img, const float *d_bqkv, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t max_len,
                         int64_t total_tokens, void *d_out, void *stream);
/* Which kernels the first half (QKV projection + attention) of a LARGE hidden-384 layer runs on, for a model with `heads` heads and a forward of n_seqs
 * sequences / total_tokens tokens whose longest sequence is max_len -- the one decision lm_bert_h384_forward_packed and a host that launches kernel by
 * kernel share: 0 = lm_qkv_attn_h384_f16 (forwards whose MEAN length is >= 216: its cost per sequence is the same from 129 to 256 tokens, it wins on
 * long sequences and ties on the benchmark corpus' N(180, 50) lengths; LEANN_MI355X_FUSED_QKV_ATTN=1 forces it, =0 forbids it), 1 = lm_qkv_h384_f16
 * (head-major output) + attention generation 3, 2 = the pair over the [tokens][1152] layout (other head counts / lengths,
 * LEANN_MI355X_QKV_LAYOUT=0, the older attention generations' switches). */
int lm_h384_first_half_form(int32_t heads, int32_t max_len, int64_t total_tokens, int32_t n_seqs);

/* Weight-STREAMING form of the 384-input linear layer (csrc/lm_qkv_h384.hip): d_out[tokens][n_out] = x W^T + b, n_out a multiple of
 * 128 in [256, 6144], d_w_img = lm_qkv_pack_h384's image of the nn.Linear weight [n_out][384] (same size).  x is read once (a wave holds
 * its 32 token rows as MFMA B fragments for the whole kernel), W streams through a four-stage LDS ring shared by eight waves -- two per
 * SIMD, ~230 registers each -- and a slab's 32 x 32 results leave through a per-wave LDS tile as full 128-byte lines.  The QKV projection
 * of the hidden-384 forward (leann/embedding_compute.py:229-239). */
int lm_qkv_h384_f16(const void *d_x, const void *d_w_img, const float *d_bias, int32_t n_out, void *d_out, int64_t tokens,
                    void *stream);
int lm_qkv_pack_h384(const void *d_w, int32_t n_out, void *d_w_img, void *stream); /* device to device, on `stream` */

/* Weight-stationary form of the 384-input linear layer (csrc/lm_gemm_ws_h384.hip): d_out[tokens][n_out] = x W^T + b with
 * d_w = the nn.Linear weight itself, [n_out][384] fp16 row major (no packing), n_out a multiple of 192 (<= 6144).  A
 * workgroup keeps its 192 x 384 weight block resident in LDS and streams token tiles past it (no per-slab barriers, two
 * waves per SIMD).  The QKV projection of lm_bert_h384_forward_packed when the model carries no wqkv_img (and of the Python host under
 * LEANN_MI355X_QKV=0, A/B); with the layer tail switched off also the output projection, followed by lm_add_layernorm_f16. */
int lm_gemm_ws_h384_f16(const void *d_x, const void *d_w, const float *d_bias, int32_t n_out, void *d_out, int64_t tokens,
                        void *stream);

/* General fp16 linear layer (csrc/lm_gemm_f16.hip):  d_out[tokens][n_out] = epi(x[tokens][k_in] W^T + b), d_w = the nn.Linear weight
 * itself ([n_out][k_in] fp16 row major, no packing, < 4 GiB), bias fp32, n_out % 128 == 0, k_in % 128 == 0; any token count.
 * epilogue: 0 = none, 1 = exact-erf GELU, 2 = + d_residual[tokens][n_out] (fp16), 3 = both.  256 x 256 workgroup tiles (128 x 128
 * when n_out % 256 != 0), MFMA 32x32x16 f16, operands staged L2 -> LDS by global_load_lds through two stages.  The GEMMs of the BERT
 * forward in compute_embeddings (leann/embedding_compute.py:229-239) for models whose hidden size is not 384 (bge-base,
 * contriever: 768): QKV projection (epilogue 0), attention output projection (2), feed-forward products (1, 2). */
int lm_gemm_f16(const void *d_x, const void *d_w, const float *d_bias, const void *d_residual, int32_t epilogue, int32_t n_out,
                int32_t k_in, void *d_out, int64_t tokens, void *stream);

/* ---- the whole packed BERT forward (hidden 384, mean or CLS pooling) in one call ---------------------
 * Replaces compute_embeddings' model.encode() (leann/embedding_compute.py:229-239) for sentence-transformers models of the
 * all-MiniLM family: embedding front end, per layer {lm_gemm_ws_h384_f16 (QKV), lm_attn_varlen_hd32_f16,
 * lm_layer_tail_h384_f16}, lm_meanpool_varlen_f16 / lm_clspool_varlen_f16 -- one foreign-function call per recompute round
 * instead of ~3 L + 2.  ffn a multiple of 192 in [192, 1728] (other widths: lm_bert_forward_packed).
 * All pointers are device pointers except `layers` (host array).  Weight layouts as documented at the entry points named above
 * (the three images of lm_layer_tail_pack_h384; leann_amd/encoder.py: pack_tail_images).  d_out: fp32 [n_seqs][384]. */
typedef struct lm_bert_h384_layer {
    const void *wqkv;  /* [1152][384] fp16, nn.Linear layout */
    const float *bqkv; /* [1152] */
    const void *wo_img; /* lm_layer_tail_pack_h384's image of [12][384][32] */
    const float *bo;
    const void *ln1_gamma, *ln1_beta; /* fp16 [384] */
    const void *w1_img;               /* ... of [ffn][384], columns in accumulator order */
    const float *b1;
    const void *w2_img; /* ... of [ffn/32][384][32] */
    const float *b2;
    const void *ln2_gamma, *ln2_beta;
    /* Optional (all three or none): the plain nn.Linear weights [384][384], [ffn][384], [384][ffn] fp16.  With them a forward of at
     * most LM_BERT_SMALL_TOKENS tokens (a one-query search round recomputes ~10 chunks) runs every layer on the general kernels --
     * lm_gemm_f16 x 4 + attention + lm_add_layernorm_f16 x 2: many small workgroups spread over the chip -- instead of the fused
     * layer tail, whose 128-token workgroup is one ~77 us dependency chain however few tokens it holds (MI355X, 200k-chunk index,
     * B = 1 search: p50 59.7 -> 47.2 ms with the limit at 6144 tokens in round 3; round 4 measured the crossover again -- 6144 /
     * 16384 / 32768 tokens: B = 1 p50 44.9 / 39.3 / 40.0 ms, B = 4 70.1 / 56.5 / 56.7 ms, B = 16 115.2 / 107.9 / 108.6 ms -- and moved
     * it to 16384; round 6, with the QKV projection of the next size class on the general GEMM (LM_BERT_QKV_GEMM_TOKENS below) and rounds that
     * dynamic batching makes 5 - 10 x larger: 4096 / 8192 / 16384 tokens: B = 1 p50 37.8 / 37.9 / 38.2 ms at batch_size 0, 13.1 / 13.0 / 14.0 ms at 64,
     * 11.9 / 11.8 / 11.9 ms at 128, B = 16 86.4 / 86.6 / 89.1 ms -- moved to 8192: profiles/r6_latency_b1_forward_size_limits_200k.jsonl).  Same
     * arithmetic up to fp16 rounding of the intermediate activations. */
    const void *wo, *w1, *w2;
    /* Optional: lm_qkv_pack_h384's image of wqkv.  With it the large-forward QKV projection runs on the weight-streaming kernel
     * (lm_qkv_h384_f16: x read once, two waves per SIMD); NULL = the weight-stationary one (lm_gemm_ws_h384_f16 on wqkv). */
    const void *wqkv_img;
} lm_bert_h384_layer;
#define LM_BERT_SMALL_TOKENS 8192
/* Round 6: between the small-forward form and the streaming QKV kernel.  A LARGE-form forward of at most this many tokens takes its QKV projection
 * from the general GEMM (lm_gemm_f16 on wqkv, then attention over the [tokens][1152] layout) instead of the weight-streaming kernel, whose 256-token
 * workgroup is a ~45 us chain however few of the 256 CUs the forward fills: 12,288 / 24,576 / 49,152 tokens: 18.6 / 32.2 / 62.4 us against 45.8 /
 * 53.8 / 65.3 us (profiles/r6_kbench_layer_kernels_at_small_forward_sizes.jsonl) -- the rounds of a small-batch search under dynamic batching
 * (batch_size 64 ... 128: 12 k ... 35 k tokens).  The fused layer tail stays (64 / 80 us at those sizes against ~100 / ~160 for the five launches it
 * replaces).  LEANN_MI355X_QKV_GEMM_TOKENS overrides (0 = never; LEANN_MI355X_SMALL_TOKENS=0, "the large-forward kernels at every size", implies 0). */
#define LM_BERT_QKV_GEMM_TOKENS 45056

typedef struct lm_bert_h384 {
    int32_t n_layers, heads, ffn, normalize;
    int32_t pooling; /* 0 = mean over the tokens (all-MiniLM), 1 = CLS (bge-small) */
    float ln_eps;
    const void *word, *pos_table, *type0, *emb_gamma, *emb_beta; /* fp16 */
    const lm_bert_h384_layer *layers;                           /* host array of n_layers entries */
} lm_bert_h384;

size_t lm_bert_h384_workspace_bytes(int64_t total_tokens); /* sized for either layer form (ffn <= 2560) */
int lm_bert_h384_forward_packed(const lm_bert_h384 *m, const int32_t *d_tok, const int32_t *d_pos, const int32_t *d_cu_seqlens,
                                int32_t n_seqs, int64_t total_tokens, int32_t max_len, void *d_workspace, size_t workspace_bytes,
                                float *d_out, void *stream);

/* ---- the whole packed BERT forward, general widths, in one call (csrc/lm_encoder_forward.cpp) -------
 * The same replacement of compute_embeddings' model.encode() (leann/embedding_compute.py:229-239) for BERT-architecture models the
 * hidden-384 kernels do not cover (bge-base-en-v1.5, contriever: hidden 768, head_dim 64, CLS or mean pooling): embedding front end,
 * per layer {lm_gemm_f16 (QKV) | lm_attn_varlen_f16 | lm_gemm_f16 (+ residual) | lm_add_layernorm_f16 | lm_gemm_f16 (+ GELU) |
 * lm_gemm_f16 (+ residual) | lm_add_layernorm_f16}, lm_meanpool_varlen_f16 / lm_clspool_varlen_f16 -- the launch sequence of
 * leann_amd/encoder.py: EncoderLayer._forward_packed_general, as one foreign-function call.  Weights are the nn.Linear tensors
 * themselves (fp16 [n_out][k_in], biases fp32, LayerNorm parameters fp16).  Envelope: hidden % 128 == 0 and <= 768, ffn % 128 == 0,
 * head_dim = hidden / heads = 32 (chunk lengths <= 256) or 64 (<= 512).  d_out: fp32 [n_seqs][hidden]. */
typedef struct lm_bert_layer {
    const void *wqkv;  /* [3 hidden][hidden] */
    const float *bqkv;
    const void *wo;    /* [hidden][hidden] */
    const float *bo;
    const void *ln1_gamma, *ln1_beta;
    const void *w1;    /* [ffn][hidden] */
    const float *b1;
    const void *w2;    /* [hidden][ffn] */
    const float *b2;
    const void *ln2_gamma, *ln2_beta;
} lm_bert_layer;

typedef struct lm_bert {
    int32_t hidden, n_layers, heads, ffn;
    int32_t pooling;   /* 0 = mean over the tokens, 1 = CLS (first token) */
    int32_t normalize; /* L2-normalise the pooled vector */
    float ln_eps;
    const void *word, *pos_table, *type0, *emb_gamma, *emb_beta; /* fp16 */
    const lm_bert_layer *layers;                                  /* host array of n_layers entries */
} lm_bert;

size_t lm_bert_workspace_bytes(const lm_bert *m, int64_t total_tokens);
int lm_bert_forward_packed(const lm_bert *m, const int32_t *d_tok, const int32_t *d_pos, const int32_t *d_cu_seqlens, int32_t n_seqs,
                           int64_t total_tokens, int32_t max_len, void *d_workspace, size_t workspace_bytes, float *d_out, void *stream);
/* CLS pooling of packed sequences (+ optional L2 normalisation): d_out[s] = float(x[first token of s]); fp16 in, fp32 out. */
int lm_clspool_varlen_f16(const void *d_x, const int32_t *d_cu_seqlens, int32_t n_seqs, int32_t hidden, int32_t normalize,
                          float *d_out, void *stream);

/* ---- token store ---------------------------------------------------------------------------
 * Replaces PassageManager.get_passage (leann/api.py:203-215) + tokenisation inside
 * compute_embeddings (leann/embedding_compute.py:229-239) at query time: passages are tokenised
 * once at load and kept packed in HBM (u16 ids, vocab < 65536). */
int lm_tokens_create(const uint16_t *tokens, const uint64_t *offsets /* n+1 */, int64_t n, int device,
                     lm_tokens **out);
void lm_tokens_free(lm_tokens *t);
/* d_out_ids: n x T int32 (pad_id beyond the chunk length, chunks truncated to T);
 * d_out_len: n int32. */
int lm_tokens_gather(const lm_tokens *t, const int32_t *d_ids, int32_t n, int32_t T, int32_t pad_id,
                     int32_t *d_out_ids, int32_t *d_out_len, void *stream);
int64_t lm_tokens_count(const lm_tokens *t);

/* ---- the built-in recompute provider (csrc/lm_recompute.hip) ------------------------------------
 * One recompute round trip of the reference -- ZMQ REQ of the node ids, PassageManager.get_passage per id, tokeniser,
 * model.encode() (hnsw_embedding_server.py:148-284, leann/api.py:203-215, leann/embedding_compute.py:229-239) -- as library code:
 * ids -> token store -> packed forward -> fp32 [n][hidden], no interpreter in the search loop.  `model` (the struct and its `layers`
 * array are copied; the device weights they point to must outlive the handle) and `tokens` as above; chunks are truncated to
 * max_seq_len (1..256) tokens; a call with more than max_tokens_per_forward tokens runs as several forwards (bounds by cumulative
 * token count, as leann_amd/encoder.py: encode_tokens_packed cuts them).  Envelope: lm_bert_h384_forward_packed's
 * (lm_recompute_create: hidden 384, the fused kernels) or lm_bert_forward_packed's (lm_recompute_create_general: e.g. bge-base,
 * 768-d; max_seq_len up to 512 at head_dim 64); the embeddings are fp32 [n][hidden].
 *   lm_index_set_recompute(idx, rc)  attaches it as the index's embedding provider (NULL detaches) and lets the search loop
 *                                    compute the round's chunk lengths before its own per-round device-to-host copy: ONE host
 *                                    synchronisation per round (lm_index_set_provider with a foreign callback: the callback's own);
 *   lm_recompute_provider            the same object as a plain lm_provider_fn (user = the handle), e.g. for lm_index_set_provider;
 *   lm_recompute_embed               embeddings of n chunk ids into the caller's fp32 [n][hidden] buffer (index build time).
 *
 * Lanes (lm_recompute_set_option / lm_recompute_get_option; added without a new ABI revision: no existing entry point, struct or enum
 * changed).  A forward is a chain of ~20 dependent launches, and each launch drains the chip before the next starts.  With "lanes" 2 or 3 the
 * handle owns 1 or 2 non-blocking streams next to the caller's and a call's forwards run on them concurrently: a call within the token
 * budget is split into that many contiguous chunk ranges of about equal token count -- only if every part holds more than
 * "lane_min_tokens" tokens (>= 256; default LM_RC_LANE_MIN_TOKENS, no smaller than the large-forward thresholds above) --, a call
 * above the budget deals its forwards round-robin to the lanes.  Every part runs the kernels chosen for the whole, and a chunk's
 * embedding does not depend on its neighbours in a forward, so the embeddings are the same bits at every lane count.  The lanes start
 * behind everything queued on the caller's stream before the call, and the caller's stream waits for all of them before the call
 * returns: what the caller queues next is ordered as with one lane.  "lanes" 1 is the single-stream provider.  The environment variable
 * LEANN_MI355X_FORWARD_LANES (1..3), read once at create, overrides the default LM_RC_DEFAULT_LANES (A/B).  Set options between calls,
 * from the thread that makes them.  lm_recompute_stats.forwards counts a forward once however many parts it ran as;
 * lm_recompute_get_option "parts" (read-only) counts the parts. */
#define LM_RC_LANE_MIN_TOKENS LM_BERT_QKV_GEMM_TOKENS
#define LM_RC_DEFAULT_LANES 3
typedef struct lm_recompute lm_recompute;
typedef struct lm_recompute_stats {
    int64_t calls, chunks, tokens, forwards, host_syncs;
} lm_recompute_stats;
int lm_recompute_create(const lm_bert_h384 *model, const lm_tokens *tokens, int32_t max_seq_len, int64_t max_tokens_per_forward,
                        lm_recompute **out);
int lm_recompute_create_general(const lm_bert *model, const lm_tokens *tokens, int32_t max_seq_len, int64_t max_tokens_per_forward,
                                lm_recompute **out);
void lm_recompute_free(lm_recompute *rc);
int lm_recompute_provider(void *user, const int32_t *d_ids, int32_t n, void **d_out, void *stream);
int lm_recompute_embed(lm_recompute *rc, const int32_t *d_ids, int32_t n, float *d_out, void *stream);
int lm_recompute_get_stats(const lm_recompute *rc, lm_recompute_stats *out);
int lm_recompute_set_option(lm_recompute *rc, const char *name, int64_t value);
int lm_recompute_get_option(const lm_recompute *rc, const char *name, int64_t *out);
int lm_index_set_recompute(lm_index *idx, lm_recompute *rc);

/* ---- measurement: event pairs around the library's own launches of the encoder's MFMA kernels (csrc/lm_timing.cpp) ----
 * One HIP event pair per launch, recorded on the stream the kernel is launched on, for the kernels whose bit is set in `mask`
 * (bit LM_KT_*); 0 = off (the default: a disabled launch pays one atomic load).  Works on every launch path -- the one-call forwards,
 * the built-in recompute provider inside lm_index_search*, single entry points.  lm_kernel_timing_read waits for the pairs recorded
 * so far and returns, per kernel, launches / summed milliseconds / summed algorithmic flops since the last reset (attention's
 * flops, 4 H sum(len^2), are summed on the device from the launch's own cumulative lengths).  bench.py's `roofline` is built from these over its timed region. */
#define LM_KT_LAYER_TAIL 0 /* lm_layer_tail_h384_f16 */
#define LM_KT_GEMM_WS 1    /* lm_gemm_ws_h384_f16 */
#define LM_KT_ATTN 2       /* lm_attn_varlen_hd32_f16 / lm_attn_varlen_f16 */
#define LM_KT_GEMM_F16 3   /* lm_gemm_f16 */
#define LM_KT_QKV 4        /* lm_qkv_h384_f16 (the weight-streaming QKV projection of the large hidden-384 forwards) */
#define LM_KT_QKV_ATTN 5   /* lm_qkv_attn_h384_f16 (QKV projection fused into attention: the first half of a hidden-384 layer of the large forwards) */
#define LM_KT_COUNT 6
typedef struct lm_kernel_time {
    const char *name;
    int64_t launches;
    double ms, work;
} lm_kernel_time;
int lm_kernel_timing_enable(uint32_t mask);
/* out[0 .. min(capacity, LM_KT_COUNT)) are written (a caller built against an older, shorter LM_KT_COUNT is never overrun). */
int lm_kernel_timing_read(lm_kernel_time *out, int32_t capacity, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* LEANN_MI355X_H */
