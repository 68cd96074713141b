/*
 * pt_api.h -- C ABI of libpt_hip.so, the MI355X (gfx950) implementation of the
 * point-based detail-transfer hot path of
 * horizon-research/3D-Reconstruction-From-Point-Cloud.
 *
 * The reference has no FFI / plugin layer: its hot path is inline
 * code in main().  Each entry point below names the reference lines it replaces;
 * INTEGRATION.md shows the patch a maintainer applies to src/pointsTransfer.cpp.
 *
 * Conventions
 *   - every function returns 0 on success, a negative pt_status otherwise; nothing
 *     throws across the boundary; pt_last_error() gives the text of the last failure;
 *   - the caller owns every buffer; nothing passed in is retained after return unless
 *     stated ("_dev" functions read device pointers during the call only);
 *   - one context per calling thread and per GPU (one process per GPU for multi-GPU);
 *   - neighbours of a target are returned ascending under the total order
 *     (d2 as IEEE double, original index as uint32) with
 *       d2 = (dx*dx + dy*dy) + dz*dz,  dx = (double)t.x - (double)p.x,  no FMA
 *     -- bit-for-bit src/Distance.h:6-11 as the reference's Release flags compile it;
 *   - `idx` values are positions in the caller's ORIGINAL cloud order (or the global
 *     indices given to pt_build_soa_indexed); missing neighbours (k > N) are
 *     PT_NOIDX with d2 = +inf;
 *   - planar xyz: `xyz` points at 3*n elements, x[0..n) then y[0..n) then z[0..n).
 *   - there is NO CPU fallback: every compute entry point fails with PT_ERR_HIP when no
 *     gfx950 device is usable.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_NOIDX 0xFFFFFFFFu
#define PT_MAX_K 32

typedef enum {
  PT_OK = 0,
  PT_ERR_ARG = -1,      /* bad argument (null pointer, k out of range, n too large ...) */
  PT_ERR_HIP = -2,      /* HIP runtime error / no device */
  PT_ERR_STATE = -3,    /* call order (query before build ...) */
  PT_ERR_NOMEM = -4,    /* device allocation failed */
  PT_ERR_UNSUPPORTED = -5
} pt_status;

typedef enum { PT_F32 = 0, PT_F16 = 1, PT_F64 = 2 } pt_xyz_type;
typedef enum { PT_DIST_UNIFORM = 0, PT_DIST_CLUSTERED = 1 } pt_synth_dist;
typedef enum { PT_BLEND_MEAN = 0, PT_BLEND_INV_D2 = 1 } pt_blend_mode;

/* The reference's record (src/Point.h:1-6), sizeof == 80, offsets 0/24/48/64/72.
 * include/Point.h carries the C++ struct with the reference's member functions;
 * this POD twin is what crosses the C boundary. */
typedef struct pt_point {
  double ver[3];
  double normal[3];
  int32_t color[3];
  int32_t _pad;
  double U;
  double V;
} pt_point;

typedef struct pt_ctx pt_ctx;

/* per-phase device timings (HIP events on the context's stream) and byte accounting */
typedef struct pt_stats_t {
  uint64_t n_source, n_target; int32_t k, _pad;
  double ms_build;          /* grid build over the source cloud (last build) */
  double ms_sort_targets;   /* target binning (last query) */
  double ms_query;          /* k-NN kernel (last query) */
  double ms_blend;          /* attribute gather + blend (last blend) */
  double ms_pca;            /* PCA normals (last pca) */
  uint64_t bytes_alg_build; /* N*(2s+4) */
  uint64_t bytes_alg_query; /* N*s + M*s + M*k*16 + M*(4k+24) */
  int32_t grid_dim[3];      /* cells per axis */
  int32_t n_levels;         /* partition passes used by the build (1 or 2) + finalize */
  double cell_size;
  uint64_t n_cells;
  uint64_t device_bytes;    /* bytes currently allocated by the context */
  /* per-kernel device times of the last build / query (HIP events on the launch stream), ms:
   * [0] bbox reduce + readback, [1] pass-1 histogram, [2] pass-1 scatter, [3] pass-2 histogram + block scan,
   * [4] pass-2 scatter, [5] finalize (cell sort), [6] target sort (all passes), [7] k-NN kernel */
  double ms_kernel[8];
  uint64_t n_leftover;      /* targets of the last query that the tile kernel handed to the group kernel */
  double rho_occupied;      /* points per NON-EMPTY cell of the last build (0 when adaptive is off) */
  int32_t n_refine;         /* how many times the last build refined its cell size */
  int32_t bbox_guess;       /* last build: 0 the bounding box came from a pass of its own; 1 the grid was laid out from a sampled
                             * box and pass 1 verified it (big clouds); -1 the sampled box was too small and the build was redone */
  double ms_bake;           /* texture bake (+ edge padding) of the last pt_bake_texture / pt_bake_maps / pt_bake_maps_h, device time */
  uint32_t n_nodes;         /* last build: refined ("heavy") cells and sub-cells that carry an 8x8x8 sub-grid (0: none needed) */
  int32_t refine_levels;    /* ... and how many levels deep (<= 3) */
  uint32_t max_cell_points; /* points of the fullest grid cell of the last build (adaptive builds) */
  uint32_t n_wave;          /* last query: targets answered by the one-wave-per-target kernel (dense neighbourhoods) */
  int32_t pass1_pooled;     /* last build: 1 pass 1 took its bin regions from a sample (no histogram pass: big clouds, two-level sort);
                             * -1 a bin outgrew its sampled region and the build was redone with the exact pass 1; 0 exact pass 1 */
  int32_t stream_skipped;   /* last pt_stream_query: (chunk, forward sweep) steps it did not search because no target's bound reached the chunk's box */
  int32_t stream_revisited; /* ... and chunks its backward sweep brought back for targets that lay outside them before they had a list */
  int32_t pass2_pooled;     /* last build: 1 pass 2 took its block regions from the macro counts (no pass-2 histogram: a rebuild of a resident cloud the
                             * previous build found uniform, or -- round 4 -- a first build whose 1/64 sample said so); -1 a block outgrew its region and
                             * the build was redone exactly; 0 exact pass 2 */
  int32_t uniform_probe;    /* last build: 1 a 1/64 sample taken before the sort found the cloud uniform (pooled pass 2 on a FIRST build), -1 it did
                             * not, 0 not asked (small cloud, one- or three-level grid, or a previous build of this cloud already knew) */
  int32_t dup_leaves;       /* last build: leaves of refined cells found to hold ONE position more than 32 times (quantised clouds): a search reads their
                             * 32 lowest indices only */
  int32_t presort_refine;   /* last build: refinements of the cell size decided from the sample BEFORE the first sort (0 .. 3; first builds of clouds the
                             * sample found non-uniform); negative: the sort's own count overruled them (a cloud stored in spatial order) and the grid was
                             * laid out again */
  int32_t n_sorts;          /* last build: full sorts of the cloud it ran (1; more when the cell size was refined after a count, a sampled box or a
                             * pooled pass had to be redone) */
  int32_t ordered_input;    /* last build: 1 = the sample found the cloud stored in spatial order (of 64 consecutive points most share a block): regions and
                             * cell size are then not taken from a sample */
  /* The route of the last query (of pt_stream_query: its last searched chunk; of the exchange: its last search), reset by every query
   * and valid whether "sync" is set or not -- none of them needs a read-back the query does not make anyway. */
  uint32_t tile_variant[2]; /* the LDS tile kernel's instantiation: [0] its first launch, [1] the large-geometry retry launch over the blocks the
                             * two-per-CU geometry passed on; 0 = no such launch.  Bits (pt_tile_code in csrc/pt_tile_route.h): 0-5 K (the list
                             * width: 8, 16, 32), 6-11 KC (the pass-1 chain), 12-15 threads per workgroup / 64, 16 WIDE queue, 17 BLEND (fused
                             * blend), 18 DBL (fp64 cloud: fp32 shadow, exact records in pass 3), 19 BND (per-target bounds and / or the cap),
                             * 20 the launch ran over a list of blocks (tile_sparse, or the retry) */
  uint32_t tile_retry_blocks; /* blocks the retry launch took (0: none, or no two-per-CU geometry ran) */
  uint32_t query_route;     /* PT_ROUTE_* bits: the kernels the last query launched (a launch over a device-side list counts even when the list
                             * turns out empty -- its length stays on the device) */
  double ms_normals;        /* pt_estimate_normals: device time of the last call, every chunk's copy, search and PCA included (HIP events) */
  uint32_t n_normal_chunks; /* ... and the number of chunks it walked the cloud in */
  double ms_outliers;       /* pt_remove_outliers: device time of the last call -- every chunk's search and scores, the reductions, the mask, and under
                             * `apply` the compaction and the rebuild (HIP events) */
  uint32_t n_outlier_chunks; /* ... and the number of chunks it walked the cloud in */
  double ms_voxel;          /* pt_voxel_downsample: device time of the last call -- bounding box, keys, sort, reduction, and under `apply` the write-back and
                             * the rebuild (HIP events) */
  uint32_t n_voxel_passes;  /* ... and the radix passes its sort ran: ceil(key bits / 8), 0 when every axis has one voxel */
} pt_stats_t;
enum {
  PT_ROUTE_TILE = 1,        /* the LDS tile kernel */
  PT_ROUTE_GROUP = 2,       /* the 8-lanes-per-target kernel, plain */
  PT_ROUTE_GROUP_HIER = 4,  /* ... the variant that descends into refined cells */
  PT_ROUTE_WAVE = 8,        /* the one-wave-per-target kernel, plain */
  PT_ROUTE_WAVE_HIER = 16,  /* ... the variant that descends into refined cells */
  PT_ROUTE_BLEND_LIST = 32, /* a blend pass over the rows the tile kernel handed over (fused queries) */
  PT_ROUTE_BLEND_ALL = 64   /* a blend pass over every row (fused queries the tile kernel did not take) */
};

/* ---- context ------------------------------------------------------------------------ */
/* device_ids[0] is the GPU this context runs on (one process per GPU); n_devices must be 1. */
int  pt_ctx_create(pt_ctx** out, const int* device_ids, int n_devices);
void pt_ctx_destroy(pt_ctx*);
/* Plumbing: run all work of this context on the caller's hipStream_t (e.g. torch's current stream), so that
 * kernels queue behind whatever produced the device buffers handed in.  NULL = HIP's default stream;
 * pt_set_param(ctx, "own_stream", 1) returns to the context's own (non-blocking) stream.
 * Switching with work in flight ("sync" 0): when the stream really changes and the context has returned from a call with work still
 * queued that none of its host waits has covered since (a "sync" 1 call, pt_synchronize), the NEW stream is made to wait for what
 * the context queued on the OLD one -- one event recorded there, one hipStreamWaitEvent here, no host wait.  So a call after the
 * switch sees the results and the scratch buffers of the calls before it, and draining the new stream covers both.  This orders the
 * context's OWN work only: buffers the caller produces on another stream still need the caller's event, and the stream being left
 * must still exist at the switch.  The context learns that its work is done from its OWN waits only: a caller under "sync" 0 who is
 * about to destroy the stream the context runs on calls pt_synchronize first (or switches away first) -- a hipStreamSynchronize of
 * the caller's own leaves the context believing work is queued there, and the next switch fails with PT_ERR_HIP on the dead stream.
 * Under "sync" 1 every call has drained its stream and a switch costs nothing. */
int  pt_set_stream(pt_ctx*, void* hip_stream);
/* Tunables: "k_hint" (the k later queries will use: picks the cell density before a build; default 8), "rho" (points
 * per grid cell, set directly; default 4), "sync" (1 = every call blocks until
 * the GPU is done, default 1; 0 = _dev calls only enqueue -- see "sync" 0 below), "adaptive" (1 = refine the cell
 * size when non-empty cells hold far more than rho points, default; needs one host read-back per build), "tile" (0 = group kernel only, 1 = tile kernel +
 * group kernel for its leftovers with the geometry chosen from the cell density (default), 2 / 3 = force the small /
 * large tile geometry), "guess_min_points" (clouds at least this large lay their grid out from the bounding box of a
 * sample and verify it during the first partition pass instead of spending a pass on the exact box; default 8 Mi),
 * "pool_min_points" (clouds at least this large, on the two-level sort, size the bins of the first partition pass from a sample
 * instead of a histogram pass over the whole cloud -- with slack, and a flag that sends the build back to the exact histogram when a
 * bin outgrows its estimate; default 32 Mi, 0 = never), "pool2" (1, default: a rebuild of a resident cloud that the previous build
 * found uniform -- no refinement, occupied cells at rho -- also sizes the blocks of the second partition pass from the macro counts
 * instead of a histogram pass, verified the same way; 0 = never),
 * "refine_threshold" (grid cells holding more points than this get an 8x8x8 sub-grid, recursively up to three levels, which
 * searches descend into instead of scanning the cell end to end -- clouds with strong density contrast; default 8192, 0 = never),
 * "wave_min" (on such clouds a target whose 27 nearest cells hold at least this many points is answered by a whole wave instead of
 * an 8-lane group; default 1 = every target of such a cloud, 0 = never; "wave_force" = 1 applies that split to every cloud -- a testing hook), "refine_macros"
 * (the finest grid the refinement of the cell size may ask for, in 64^3-cell macro blocks: default 1024, at most 8192 -- grids beyond
 * 1024 macro blocks, which a cloud of more than ~1e9 points gets anyway, cost the sort one more partition pass),
 * "refine_cells_per_point" (that refinement also stops at this many grid cells per point; default 2), "grid_hint" (1,
 * default: pt_rebuild of the same resident cloud starts from the cell size the previous build ended with -- checked against the
 * occupancy it finds -- instead of searching for it again; 0: every build searches from scratch), "stream_bounds" (1, default:
 * pt_stream_query searches every chunk under the bounds the targets bring and defers / skips what is out of reach; 0: every target,
 * unbounded, in every chunk -- round 2's behaviour, kept as a measurement switch).
 * Round 4: "forget" (1: the next build of the resident cloud decides everything a FIRST build decides -- sampled bounding box, pooled
 * passes, the uniformity sample, the cell size: what bench.py times as its cold step), "dup_runs" (1, default: leaves of refined cells
 * that hold ONE position more than 32 times keep their 32 lowest indices in front and searches read that front only; 0 = off),
 * "tile_sparse" (the tile kernel over a list of the blocks that hold targets: 0 never, 1 always, 2 = on clouds that leave most of
 * their grid empty, default), "tile_contrast" (1: on clouds with strong density contrast the tile kernel runs first, k <= 24, and the
 * wave kernel takes what it leaves; 0, default: a wave per target -- measured faster), "local_ids" (1: the next slab build -- ascending
 * global indices, or a slab pt_build_synth generates -- keeps positions in its records and its own attribute records only; see
 * pt_set_attributes_local), "presort_refine" (1, default: the first build of a big cloud the sample finds non-uniform refines its cell size
 * from the sample's bound on the points per occupied cell, before the first sort; 0: after it, from the sort's count -- round 3's behaviour),
 * "normals_chunk" (points per chunk of the self-query passes: pt_estimate_normals, pt_remove_outliers -- it bounds their scratch memory;
 * default 8 Mi, at least 1024 -- PT_ERR_ARG below that; small values make a small cloud take many chunks, which is what tests use it for).
 *
 * "sync" 0, what it means.  Entry points that take HOST arrays are unchanged: the input may be reused and the outputs are complete when
 * the call returns (builds and pt_set_attributes* may leave their last kernels queued, behind which every later call of the context
 * runs).  The _dev entry points return without the trailing wait; their results are ordered on the context's stream (pt_synchronize,
 * or a consumer on the same stream).  Answers are the same bit for bit under either setting.  What differs:
 *   - statistics: the device times (ms_build, ms_sort_targets, ms_query, ms_blend, ms_pca, ms_kernel[], and ms_normals unless nrm_out
 *     is host memory) and n_leftover are refreshed under "sync" 1 only and keep their last values otherwise; tile_variant,
 *     tile_retry_blocks, query_route and n_wave are valid under both;
 *   - the tile kernel's leftovers at k <= 16 stay with the 8-lane group kernel, which reads the leftover list and its length on the
 *     device (PT_ROUTE_TILE | PT_ROUTE_GROUP); under "sync" 1, and at k > 16 under either setting, each gets a wave, sized by a
 *     read-back of that length (PT_ROUTE_TILE | PT_ROUTE_WAVE);
 *   - "only enqueue" holds for: pt_blend_dev, pt_blend_weighted_dev, pt_pca_normals_dev, pt_merge_candidates_dev,
 *     pt_resident_target_ids / _xyz / pt_resident_source_xyz, pt_targets_soa(on_device), and the queries (pt_query_resident,
 *     pt_query_blend_resident, pt_query_soa(on_device), pt_query_bounded_dev) on a cloud without refined cells or density contrast when
 *     either the group kernel runs alone ("tile" 0, bounded queries) or the tile kernel runs its large geometry over all blocks with
 *     k <= 16 ("tile" 3, or "tile" 1 where the cloud's regions exceed the two-per-CU budget; "tile_sparse" not taken);
 *   - the other query routes still wait ONCE on the host for a count that sizes their next launch: the length of the block list
 *     ("tile_sparse" 1, or 2 on clouds that leave most of their grid empty and on pt_estimate_normals' chunks); the retry count of a
 *     two-per-CU geometry ("tile" 2, or "tile" 1 where the regions fit it, k <= 24: at k <= 16 read at once, above shared with the
 *     next); the leftover list's length at k > 16; the wave lists' lengths on clouds with refined cells, refined cell size, density
 *     contrast or "wave_force".  pt_slab_need_dev waits for its host slab_bounds, pt_pack_requests_dev for the count it returns,
 *     pt_estimate_normals once per chunk as its query route does, and every build for its bounding box and occupancy;
 *   - pt_remove_outliers waits on the host wherever its query route waits, as pt_estimate_normals does, and once more for the reduction's
 *     result and n_kept, which size the compaction (under `apply` the rebuild waits as every build does); device outputs (keep_out,
 *     score_out with out_on_device) are ordered on the context's stream;
 *   - ms_outliers is refreshed under "sync" 1 only;
 *   - pt_voxel_downsample waits on the host twice -- for the bounding box, and for the number of occupied voxels, which sizes the reduction
 *     -- and under `apply` as every build does; device outputs (voxel_of_out, count_out with out_on_device) are ordered on the context's
 *     stream; ms_voxel is refreshed under "sync" 1 only.
 *
 * "max_dist" r (cloud units; r >= 0, +inf = off, the default; NaN or r < 0: PT_ERR_ARG): neighbours farther than r are not returned.
 * R2 = r * r is computed once in double, and a source point is in reach iff d2 <= R2 (d2 the metric above; inclusive, like
 * pt_query_bounded_dev).  Setting it needs no rebuild and keeps what the context learned for its next build.  While it is set:
 *   - every query result (pt_query_aos / _soa, pt_query_resident / _blend_resident / _resident_host, pt_stream_query, and the
 *     lists pt_exchange_merge_dev / _local / pt_query_exchange_blend complete) equals the uncapped result with every entry of
 *     d2 > R2 replaced by (PT_NOIDX, +inf), bit for bit; pt_query_bounded_dev bounds each target by min(bound2[t], R2);
 *   - pt_slab_need_dev, pt_pack_requests_dev and the exchange take min(d2[t][k-1], R2) as a target's reach (a short list reaches
 *     only the slabs within r), and request packets carry that reach as their bound;
 *   - the blends (pt_blend, pt_blend_dev, pt_query_blend_resident, pt_query_resident_host, pt_query_exchange_blend, the exchange's
 *     re-blend) blend a row with at least one entry over the entries it has (mean over their count, or normalised inverse-d2), and do
 *     NOT WRITE a row without any entry: rgb_out / nrm_out keep what the caller put there.  Uncapped, such rows get zeros, as ever.
 *     pt_blend_weighted is unchanged;
 *   - every context of a sharded job must use the same r: pt_exchange_merge_local returns PT_ERR_ARG when its contexts disagree, and
 *     the ranks of an RCCL job (pt_exchange_merge_dev) must set the same value -- like "local_ids", nothing checks it across processes.
 * pt_bake_texture takes the lists it is given (PT_NOIDX entries are skipped, as ever). */
int  pt_set_param(pt_ctx*, const char* name, double value);
const char* pt_last_error(pt_ctx*);
int  pt_stats(pt_ctx*, pt_stats_t* out);
int  pt_synchronize(pt_ctx*);

/* ---- build: replaces `Tree tree(points.begin(), points.end())`, pointsTransfer.cpp:259 ---- */
/* AoS reference records on the host (80-B stride); coordinates are kept as double on the GPU. */
int  pt_build_aos(pt_ctx*, const pt_point* cloud, uint64_t n);
/* Planar xyz of `xyz_type` (+ optional interleaved rgb u8[n][3] and normals f32[n][3]); host or
 * device memory according to on_device. PT_F16 clouds stay fp16 in the resident input (6 bytes per
 * point) and are widened -- exactly -- as the build reads them; answers are those of the fp32 cloud
 * holding the same values. */
/* Slabs that keep their OWN points' attribute records only (round 4): after pt_set_param("local_ids", 1), a
 * pt_build_soa_indexed whose global indices are STRICTLY ASCENDING (PT_ERR_ARG otherwise) sorts each point's position in the slab's
 * arrays into the records -- positions order like indices, so results are unchanged -- and pt_set_attributes_local uploads the records
 * of exactly those n points in that order (rgb [n][3], nrm [n][3]): 16 n bytes per GPU instead of 16 N.  Finished neighbour lists carry
 * global indices as ever.  pt_exchange_merge_* then sends every candidate's record with it and blends the completed rows from what
 * arrived; every rank of a job must run the same mode.  pt_blend_dev on such a context blends the entries that belong to this slab
 * (lists the exchange completed are blended by the exchange). */
int  pt_set_attributes_local(pt_ctx*, const uint8_t* rgb, const float* nrm, int on_device);
int  pt_build_soa(pt_ctx*, const void* xyz, int xyz_type, const uint8_t* rgb, const float* nrm,
                  uint64_t n, int on_device);
/* Same, for one spatial slab of a larger cloud: gidx[i] is the point's index in the whole cloud
 * (what queries return); attributes stay indexed by that global index, see pt_set_attributes. */
int  pt_build_soa_indexed(pt_ctx*, const void* xyz, int xyz_type, const uint32_t* gidx, uint64_t n,
                          int on_device);
/* Attribute table indexed by global index (the whole cloud's, on every GPU). */
int  pt_set_attributes(pt_ctx*, const uint8_t* rgb, const float* nrm, uint64_t n_total, int on_device);
/* The same table filled piecewise from HOST memory: records [first, first + count) of a table of n_total (the first call, or a
 * change of n_total, allocates it zeroed).  For hosts that hold the attributes in pieces -- the ranks of `pointsTransfer --gpus N`
 * each parse 1/N of the file and read the other pieces from the rendezvous directory -- so that no rank ever assembles the whole
 * table in host memory. */
int  pt_set_attributes_range(pt_ctx*, uint64_t first, uint64_t count, const uint8_t* rgb, const float* nrm, uint64_t n_total);
/* SURVEY.md Appendix C generator, on the device.  Keeps the points whose coordinate along
 * `slab_axis` lies in [slab_lo, slab_hi) (pass -inf/+inf, or slab_axis < 0, for the whole cloud);
 * indices stay global; the attribute table is generated for all n_total points. */
int  pt_build_synth(pt_ctx*, uint64_t n_total, uint64_t seed, int dist, int xyz_type,
                    int slab_axis, double slab_lo, double slab_hi);
/* Re-run the grid build over the resident source cloud (what a bench step times). */
int  pt_rebuild(pt_ctx*);
uint64_t pt_num_source(pt_ctx*);        /* points resident in this context (slab-local) */

/* ---- query: replaces the K_neighbor_search loop, pointsTransfer.cpp:462-479 ---------------- */
int  pt_query_aos(pt_ctx*, const pt_point* targets, uint64_t m, int k, uint32_t* idx, double* d2_or_null);
int  pt_query_soa(pt_ctx*, const void* xyz, int xyz_type, uint64_t m, int k, int on_device,
                  uint32_t* idx, double* d2_or_null);
/* Generate m targets on the device (stream 1 of the generator) into the context; query them with
 * pt_query_resident.  tgt_lo/hi restrict to targets whose slab_axis coordinate is in [lo,hi).  The clustered
 * distribution derives targets from the sources (strided subsample + jitter): call it after a pt_build_synth with
 * the same seed. */
int  pt_targets_synth(pt_ctx*, uint64_t m_total, uint64_t seed, int dist, int xyz_type,
                      int slab_axis, double slab_lo, double slab_hi);
/* Make the caller's own targets resident (planar xyz, host or device; or host AoS Point records = mesh vertices), so that
 * pt_query_resident / pt_query_blend_resident work on them.  Same type rule as the queries: the targets' type must be the
 * cloud's (fp16 is widened to fp32; AoS records are fp64 like a cloud built with pt_build_aos). */
int  pt_targets_soa(pt_ctx*, const void* xyz, int xyz_type, uint64_t m, int on_device);
int  pt_targets_aos(pt_ctx*, const pt_point* targets, uint64_t m);
uint64_t pt_num_targets(pt_ctx*);
/* Query the resident targets; idx/d2 are DEVICE buffers of m*k entries (d2 may be NULL). */
int  pt_query_resident(pt_ctx*, int k, uint32_t* idx_dev, double* d2_dev_or_null);
/* pt_query_resident and pt_blend_dev in ONE pass over the resident targets (north_star's "find the k nearest
 * and blend colour/normal onto the vertex"): where the LDS tile kernel answers (fp32 clouds, k <= 32) it gathers
 * the k attribute records of a target as soon as it has ranked them, so the gathers overlap the ranking of other
 * targets instead of forming a pass of their own.  Same outputs as the two calls; the blend sums the same fp64
 * terms in a different order (within the 1e-5 tolerance of the path, not bit-identical to pt_blend_dev).
 * rgb_out_dev / nrm_out_dev: device float[m*3], either may be NULL. */
int  pt_query_blend_resident(pt_ctx*, int k, int blend_mode, uint32_t* idx_dev, double* d2_dev_or_null,
                             float* rgb_out_dev, float* nrm_out_dev);
/* Global index (position in the whole target set) of each resident target, device u32[m]. */
/* The same for a C++ host that holds no device memory (the CLI's --synthetic): idx / d2 / rgb / nrm come back to HOST memory
 * ([m][k], [m][k], [m][3], [m][3], m = pt_num_targets; d2 / rgb / nrm may be NULL, blend_mode < 0 skips the blend). */
int  pt_query_resident_host(pt_ctx*, int k, int blend_mode, uint32_t* idx_out, double* d2_out_or_null, float* rgb_out_or_null, float* nrm_out_or_null);
int  pt_resident_target_ids(pt_ctx*, uint32_t* ids_dev);
/* Planar xyz (f32 or f64 as generated) of the resident targets, copied to a device buffer. */
int  pt_resident_target_xyz(pt_ctx*, void* xyz_dev);
/* Planar xyz of the resident SOURCE cloud as it is kept (f32, f64, or f16 for clouds built from PT_F16), copied to a device buffer of
 * 3 * pt_num_source values; *xyz_type_out (may be null) receives the element type.  Tests and probes read generated clouds with it. */
int  pt_resident_source_xyz(pt_ctx*, void* xyz_dev, int* xyz_type_out);

/* ---- blend: the only blend arithmetic of the reference is pointsTransfer.cpp:95-97 --------- */
/* host buffers in / out */
int  pt_blend(pt_ctx*, const uint32_t* idx, const double* d2_or_null, uint64_t m, int k, int mode,
              float* rgb_out, float* nrm_out);
/* device buffers in / out */
int  pt_blend_dev(pt_ctx*, const uint32_t* idx_dev, const double* d2_dev_or_null, uint64_t m, int k,
                  int mode, float* rgb_out_dev, float* nrm_out_dev);
/* The reference's own mix formula (src/pointsTransfer.cpp:95-97: `float c = bc0*c0 + bc1*c1 + bc2*c2`, double weights
 * times int colours summed left to right in double, stored to a float; :100-102 assign it to an unsigned char) for k
 * terms with CALLER-given weights w[m*k] -- with k = 3 and barycentric weights it is bit-for-bit that expression.  No
 * normalisation; entries with idx = PT_NOIDX contribute nothing; normals get the same arithmetic. */
int  pt_blend_weighted(pt_ctx*, const uint32_t* idx, const double* w, uint64_t m, int k, float* rgb_out, float* nrm_out);
int  pt_blend_weighted_dev(pt_ctx*, const uint32_t* idx_dev, const double* w_dev, uint64_t m, int k,
                           float* rgb_out_dev, float* nrm_out_dev);
/* PCA normal of the k neighbours (BASELINE config 3); needs the whole cloud resident (no slabs: PT_ERR_UNSUPPORTED).  Unit eigenvector
 * of the smallest eigenvalue of the covariance of the entries that name a point (idx != PT_NOIDX and idx < n), oriented so that its dot
 * product with the sum of those points' stored normals is >= 0 (its z component >= 0 where no attribute table is resident).  A row with
 * fewer than three such entries -- an empty row included -- gets (0, 0, 1).  That holds under a "max_dist" cap too: unlike the capped
 * blends, PCA writes every row. */
int  pt_pca_normals(pt_ctx*, const uint32_t* idx, uint64_t m, int k, float* nrm_out);
int  pt_pca_normals_dev(pt_ctx*, const uint32_t* idx_dev, uint64_t m, int k, float* nrm_out_dev);
/* pt_estimate_normals: normals for a resident cloud that ships without them (or whose normals are to be replaced), written into the
 * resident attribute table.  Needs a built, whole cloud: PT_ERR_STATE before a build, PT_ERR_UNSUPPORTED on a slab context
 * (pt_build_soa_indexed, a slab of pt_build_synth, "local_ids"), like PCA.  fp32, fp16 and fp64 clouds alike.
 * The normal of source point i:
 *   - take the neighbour list a pt_query_* call with the same k returns for a target at point i's own position, against the resident
 *     cloud: the k nearest source points under (d2, index) -- i itself, or a lower-indexed duplicate in front of it, among them -- and
 *     under a "max_dist" cap the capped list;
 *   - the unit eigenvector of the smallest eigenvalue of the covariance of those points: pt_pca_normals' definition to the letter, "fewer
 *     than three entries -> (0, 0, 1)" included (such a row is not oriented either).
 * Orientation (`orient`, a pt_orient_mode; the stored normals are never read, so the in-place write has no read / write hazard):
 *   PT_ORIENT_AXIS       dot(n, ref) >= 0; ref == NULL means (0, 0, 1), the convention of pt_pca_normals without a table;
 *   PT_ORIENT_VIEWPOINT  dot(n, ref - p_i) >= 0, evaluated in double; ref must not be NULL.
 * A dot product of exactly 0 keeps the eigenvector's sign as computed (pt_pca_normals' `ref < 0 ? -1 : 1`).  A non-finite ref, a zero
 * ref in AXIS mode, a NULL ref in VIEWPOINT mode, an unknown mode, or k outside [3, PT_MAX_K]: PT_ERR_ARG.
 * The result goes into the attribute table at the point's original index; colours are kept.  A cloud built without attributes gets a
 * table with zero colours, so blends, pt_bake_maps and a later pt_pca_normals -- which then ORIENTS BY THESE NORMALS instead of +z --
 * see a resident table afterwards.  nrm_out (may be NULL) receives float[n][3] by original index, in host or device memory according
 * to out_on_device.  n = 0: PT_OK, nothing is written.  Resident targets (pt_targets_*) are left as they were; the statistics of "the
 * last query" describe the last chunk's search, with ms_sort_targets / ms_query summed over the chunks ("sync" = 1).
 * Memory: the lists never exist for the whole cloud.  The pass walks the sorted records in chunks of c = "normals_chunk" points: each
 * chunk's records become the target records as they are (no target sort, nothing re-uploaded) and are searched by the usual routes.
 * Beyond the attribute table (16 n) and, for fp32 / fp16 clouds, one position table by original index (16 n), the scratch is
 *   c * (4 k + 2 r + 9) bytes (lists, two target record buffers of r = 16 or 32 bytes, leftover list, wave marks), 8 c more under a
 *   cap, 12 c more for a host nrm_out, plus 20 bytes per 512-cell grid block for the block tables -- nothing that grows with n * k.
 * pt_stats_t: ms_normals, n_normal_chunks. */
typedef enum { PT_ORIENT_AXIS = 0, PT_ORIENT_VIEWPOINT = 1 } pt_orient_mode;
int  pt_estimate_normals(pt_ctx*, int k, int orient, const double ref3_or_null[3], float* nrm_out_or_null, int out_on_device);

/* pt_remove_outliers: take stray points (flyers between surfaces, returns through windows, sky points) out of the resident cloud, on the
 * device: no [n][k] matrix crosses PCIe and nothing is uploaded again.  Needs a built, whole cloud: PT_ERR_STATE before a build (or when
 * an attribute table is resident whose n_total differs from n), PT_ERR_UNSUPPORTED on a slab context (pt_build_soa_indexed, a slab of
 * pt_build_synth, "local_ids") -- a slab does not hold its points' neighbours.  fp32, fp16 and fp64 clouds alike.
 * The list of point i is pt_estimate_normals' list: what a pt_query_* call with this k returns for a target at i's own position against
 * the resident cloud -- (d2, index) order, capped under "max_dist"; entry 0 is i itself or a lower-indexed duplicate, at d2 = 0.  c is the
 * number of its entries that name a point.
 *   PT_OUTLIER_STATISTICAL  k in [2, PT_MAX_K], param = alpha (finite, >= 0).  Score s_i = (sum over j = 1 .. c-1 of sqrt(d2_j)) / (c - 1) in
 *     double when c >= 2, added in list order from j = 1 up (an order that depends on nothing but k); +inf when c <= 1 -- a point alone
 *     under the cap, always removed.  Over the n_f points with finite scores: mean = sum(s) / n_f, stddev = sqrt(sum((s - mean)^2) / n_f)
 *     -- the population value, from a second pass over the scores, not from sum(s^2) -- and threshold T = mean + alpha * stddev (n_f = 0:
 *     all three are 0).  Point i is kept iff s_i <= T.  Both sums run over the score table BY ORIGINAL INDEX after the last chunk:
 *     workgroup w adds the finite scores of indices [4096 w, 4096 (w + 1)) (thread t those at t, t + 256, ... in that order, then a tree
 *     over the 256 threads) and one workgroup adds the partials the same way -- a grid fixed by n alone, no floating-point atomics.  So
 *     mean, stddev, T and the mask are bit-identical from run to run, for every "normals_chunk", every search route and every device.
 *   PT_OUTLIER_RADIUS  k = m + 1 in [2, PT_MAX_K], m the number of OTHER points required; param = r (finite, > 0).  For the length of the
 *     call the lists are searched under reach min(r, max_dist): R2 = r * r computed once in double, d2 <= R2 inclusive, exactly like
 *     "max_dist", which is unchanged when the call returns, whether it succeeds or fails.  Score = c - 1 as a double; i is kept iff
 *     c == k.  No floating-point sum is involved: the mask is exact.
 * Outputs: keep_out uint8[n_before] (1 = kept) and score_out double[n_before], both by original index, in host or device memory according to
 * out_on_device; either may be NULL.  result (may be NULL) is host memory: n_before, n_kept, n_scored (STATISTICAL: n_f; RADIUS: n_before)
 * and mean / stddev / threshold (RADIUS: 0, 0, k - 1).  n = 0: PT_OK, a zero result, nothing written.
 * apply = 0: the resident cloud -- source records, attribute table, resident targets -- is untouched, and so is what the context learned
 *   for its next build.
 * apply = 1, 0 < n_kept < n_before: the resident cloud becomes the kept points in their original relative order; the new index of a kept
 *   point is the number of kept points with a smaller original index (the cumulative sum of keep_out maps old to new).  The planar
 *   coordinates are compacted in the width they are held in (fp16, fp32, fp64), the attribute table likewise when one is resident,
 *   everything derived from the old cloud is dropped, and the grid is built over the result as over a new cloud.  Afterwards EVERY entry
 *   point behaves exactly as on a fresh context on which pt_build_soa (+ attributes) was called with the kept subset, results bit for
 *   bit: pt_num_source, every query, the blends, pt_estimate_normals, pt_pca_normals, pt_bake_maps, pt_resident_source_xyz.  Resident
 *   targets are left as they were.
 * apply = 1, n_kept = n_before: mask and scores are delivered, nothing is rebuilt, PT_OK.
 * apply = 1, n_kept = 0: PT_ERR_ARG ("would remove every point") after mask, scores and result have been delivered; the cloud is unchanged.
 * PT_ERR_ARG also for an unknown mode, k out of range, a param that is not finite or out of range.
 * Memory: the lists never exist for the whole cloud (chunks of c = "normals_chunk" points, as pt_estimate_normals).  Scratch:
 *   c * (12 k + 2 r + 9) bytes (index and d2 rows, two target record buffers of r = 16 or 32 bytes, leftover list, wave marks), 8 c more
 *   under a cap or in RADIUS mode, 20 bytes per 512-cell grid block, and 13 n + n / 100 bytes that stay with the context until it is
 *   destroyed: scores (8 n), the kept indices (4 n), the mask (n), and the mask's tile offsets (12 bytes per 2048 points) and the
 *   reductions' partials (12 bytes per 4096 points).
 *   The compaction gathers into the sort's own record buffers, which the rebuild overwrites anyway: no second copy of the cloud.
 * pt_stats_t: ms_outliers, n_outlier_chunks; the statistics of "the last query" are those of the last chunk, with ms_sort_targets /
 * ms_query summed over the chunks ("sync" 1). */
typedef enum { PT_OUTLIER_STATISTICAL = 0, PT_OUTLIER_RADIUS = 1 } pt_outlier_mode;
typedef struct pt_outlier_result_t {
  uint64_t n_before, n_kept;
  uint64_t n_scored;            /* STATISTICAL: points with a finite score (what mean / stddev run over); RADIUS: n_before */
  double mean, stddev, threshold;   /* STATISTICAL; RADIUS: 0, 0, k - 1 */
} pt_outlier_result_t;
int  pt_remove_outliers(pt_ctx*, int mode, int k, double param, int apply,
                        uint8_t* keep_out_or_null, double* score_out_or_null, int out_on_device,
                        pt_outlier_result_t* result_or_null);

/* pt_voxel_downsample: thin the resident cloud to one point per occupied voxel -- the centroid of the voxel's members, with their mean colour
 * and mean normal -- on the device: nothing is read back, thinned on the host and uploaded again.  It is the first step of the clean-up
 * stage: pt_remove_outliers and pt_estimate_normals cost a search per point and are normally run on the thinned cloud.  Needs a built,
 * whole cloud: PT_ERR_STATE before a build (or when an attribute table is resident whose n_total differs from n), PT_ERR_UNSUPPORTED on a
 * slab context (pt_build_soa_indexed, a slab of pt_build_synth, "local_ids").  fp32, fp16 and fp64 clouds alike.  "max_dist" plays no part.
 * Arguments: `voxel` (the voxel's side, cloud units) must be finite and > 0, `origin3_or_null` NULL or three finite doubles: PT_ERR_ARG otherwise.
 * Voxel of a point: coordinates are widened exactly to double; o is the caller's origin, or the exact per-axis minimum of the cloud (NULL);
 *   per axis i = floor((p - o) / voxel), the subtraction and the division each rounded once (a true division, no reciprocal).  The expression is
 *   monotone in p, so dims[a] = floor((max_a - o_a) / voxel) + 1 -- the voxels from the origin to the cloud's far face -- and the range check
 *   come from the bounding box alone.  Every index must lie in [0, 2^21): PT_ERR_ARG otherwise ("origin above the cloud": some point has a
 *   negative index; "voxel too small for the cloud's extent"), with the cloud unchanged and nothing written.
 * Order: occupied voxels are numbered 0 .. n_voxels - 1 in ascending (iz, iy, ix); a voxel's members are taken in ascending original index.
 * Result point j, from the c members of voxel j ranked 0 .. c - 1:
 *   position  per axis the BLOCKED SUM S of the coordinates as doubles, divided by (double)c with one division, rounded to the width the cloud
 *             is held in: fp64 as is, fp32 by round-to-nearest-even, fp16 by rounding to fp32 FIRST and then to fp16, both nearest-even (a
 *             direct double -> half conversion differs where the fp32 rounding lands on a tie of the fp16 grid);
 *   blocked sum  P_b = the left-to-right sum, starting from its first term, of ranks [256 b, 256 (b + 1)); S = the left-to-right sum of P_0,
 *             P_1, ...  For c <= 256 this is the plain sequential sum.  The order is a function of c alone -- of no tunable, route or device
 *             -- and no floating-point atomic is used: results are bit-identical from run to run.  A one-member voxel reproduces its point;
 *   colour    (attribute table resident) per byte of rgba the exact integer sum s of the members' bytes; the result byte is
 *             (2 s + c) / (2 c) in integer arithmetic: the mean, rounded half up;
 *   normal    per component the same blocked sum of the stored floats widened to double, divided by c, rounded to float.  NOT renormalised
 *             -- pt_bake_maps' convention for mixed normals: a mean of unit normals is shorter than 1 where they disagree.  To get unit
 *             normals back, run pt_estimate_normals on the thinned cloud.
 * Outputs: voxel_of_out uint32[n_before], the voxel number of every original point; count_out uint32, capacity n_before, entries
 *   [0, n_voxels) written; host or device memory according to out_on_device; either may be NULL.  result (may be NULL) is host memory.
 *   n = 0: PT_OK, a zero result, nothing written.
 * apply = 0: the resident cloud, the sorted records, the attribute table, the resident targets and what the context learned for its next
 *   build are untouched, bit for bit (the scratch is the call's own, never the sort's record buffers).
 * apply = 1: the resident cloud becomes the n_voxels result points in voxel order -- also when n_voxels == n_before: the order changes --
 *   and the attribute table is replaced likewise when one is resident; everything derived from the old cloud is dropped and the grid is
 *   built over the result as over a new cloud, exactly as pt_remove_outliers ends.  Afterwards EVERY entry point behaves as on a fresh
 *   context on which pt_build_soa (+ attributes) was called with those arrays, bit for bit.  Resident targets are left as they were.
 * Memory: with w = 4 or 8, the key's bytes (8 when the three axes need more than 32 bits together), the scratch is
 *   (2 w + 16) n + n / 4 bytes: two (key, index) buffers (2 (w + 4) n), the voxel starts (4 n), voxel_of (4 n), and the sort's per-tile digit
 *   counts (1 KB per 4096 points); 12 bytes per 2048 points of tile offsets on top.  The head marks, the counts, and for voxels of more
 *   than 256 members the block partials (2 slots of 68 bytes per 256 points) live in the (key, index) buffer the sort did not end in.  The
 *   scratch stays with the context until it is destroyed; under `apply` the result is written through the sort's record buffers, which the
 *   rebuild overwrites anyway.
 * pt_stats_t: ms_voxel, n_voxel_passes. */
typedef struct pt_voxel_result_t {
  uint64_t n_before, n_voxels;     /* points before; occupied voxels = points after */
  uint32_t max_count;              /* members of the fullest voxel */
  uint32_t dims[3];                /* voxels per axis, from the origin to the far face of the cloud's box */
  double   origin[3], voxel;       /* as used */
} pt_voxel_result_t;
int  pt_voxel_downsample(pt_ctx*, double voxel, const double origin3_or_null[3], int apply,
                         uint32_t* voxel_of_out_or_null, uint32_t* count_out_or_null, int out_on_device,
                         pt_voxel_result_t* result_or_null);

/* ---- multi-GPU merge ---------------------------------------------------------- */
/* G-way merge of candidate lists under (d2, idx): lists are [g][m][k] device arrays. */
int  pt_merge_candidates_dev(pt_ctx*, const uint32_t* idx_lists_dev, const double* d2_lists_dev, int g,
                             uint64_t m, int k, uint32_t* idx_out_dev, double* d2_out_dev);
/* For each target t and each slab s != my_slab, need[s*m + t] = 1 iff slab s can still hold one of
 * t's k nearest: dist2(t, slab interval) <= d2[t][k-1], or the list is not full.  This is
 * Distance::min_distance_to_rectangle (src/Distance.h:27-57) applied to slab boxes.
 * slab_bounds: G+1 ascending doubles on the host. */
int  pt_slab_need_dev(pt_ctx*, const void* tgt_xyz_dev, int xyz_type, const double* d2_dev, uint64_t m, int k,
                      int slab_axis, const double* slab_bounds, int g, int my_slab, uint8_t* need_dev);
/* pt_slab_need_dev and the selection of the targets that need another slab in one pass: those targets leave as request
 * packets pkt_out[c][5] = {x, y, z, current k-th d2, bitmask of the slabs to ask (exact in a double: g <= 52)} with
 * their rows in sel_out[c]; *count_out = c (host).  Both outputs must hold m entries; the order is unspecified. */
int  pt_pack_requests_dev(pt_ctx*, const void* tgt_xyz_dev, int xyz_type, const double* d2_dev, uint64_t m, int k,
                          int slab_axis, const double* slab_bounds, int g, int my_slab, uint32_t* sel_out_dev,
                          double* pkt_out_dev, uint32_t* count_out);
/* Bounded query for foreign targets: like pt_query_soa(on_device=1) but each target starts from the
 * radius bound2[t] (its current k-th squared distance; +inf = unbounded): only points with
 * d2 <= bound2[t] are returned. */
int  pt_query_bounded_dev(pt_ctx*, const void* xyz_dev, int xyz_type, const double* bound2_dev, uint64_t m,
                          int k, uint32_t* idx_dev, double* d2_dev);

/* ---- native slab exchange: RCCL over xGMI behind the C ABI, one rank per process and GPU ---------------
 * After every rank has searched its HOME targets in its own slab (pt_query_*), pt_exchange_merge_dev completes the lists:
 *   1. the targets whose k-th distance reaches another slab (Distance::min_distance_to_rectangle, src/Distance.h:27-57, on
 *      the slab boxes) are counted per destination; ONE all-gather ships the G x G count matrix (its read-back is the exchange's only host wait);
 *   2. grouped ncclSend / ncclRecv carry 32-byte request packets {x, y, z, k-th d2} owner to owner (all links at once);
 *   3. every rank answers what it received with a radius-bounded search of its slab;
 *   4. the k candidates per request travel back the same way and are merged under the total order (d2, index);
 *   5. optionally the rows that were completed get their blend redone (blend_mode >= 0 and rgb / nrm outputs given).
 * pt_comm_unique_id (any one rank) creates the 128-byte RCCL id the ranks share out of band; pt_comm_init joins the
 * communicator on the context's device -- call it before the heavy GPU work of the process.  bounds: world + 1 ascending
 * slab bounds along `axis` (first / last may be -inf / +inf).  librccl is loaded at pt_comm_* time (dlopen), not at link time.
 * pt_exchange_merge_local runs the same phases for G contexts of ONE process with device copies as transport (G logical
 * slabs on one GPU: what tests use where only one GPU exists). */
#define PT_COMM_ID_BYTES 128
typedef struct pt_exchange_stats_t {
  uint64_t crossing;        /* request packets this rank sent (a target needing two slabs counts twice) */
  uint64_t answered;        /* request packets this rank answered */
  uint64_t bytes_sent, bytes_received;   /* requests + answers, this rank */
  double ms;                /* device time of the whole exchange on this rank's stream (HIP events) */
} pt_exchange_stats_t;
int  pt_comm_unique_id(void* id_out);
int  pt_comm_init(pt_ctx*, int world, int rank, const void* id);
int  pt_comm_destroy(pt_ctx*);
/* Error-path teardown: ncclCommAbort instead of ncclCommDestroy -- never waits for peers (which may be waiting for this rank).
 * pt_comm_destroy and pt_ctx_destroy take this path by themselves once an RCCL call or any phase of an exchange has failed on
 * the context; a host that gives up for reasons of its own (a failed build, a bad input file) calls it before exiting. */
int  pt_comm_abort(pt_ctx*);
int  pt_exchange_merge_dev(pt_ctx*, const void* tgt_xyz_dev, int xyz_type, uint64_t m, int k, int slab_axis, const double* slab_bounds,
                           uint32_t* idx_dev, double* d2_dev, int blend_mode, float* rgb_dev, float* nrm_dev, pt_exchange_stats_t* stats_or_null);
/* One rank's whole query for a C++ host that holds no device memory: the home targets (planar host xyz) are searched in this
 * rank's slab with the blend fused in, completed by pt_exchange_merge_dev (world > 1), and idx / d2 / rgb / nrm come back to
 * host memory ([m][k], [m][k], [m][3], [m][3]; rgb / nrm may be NULL, blend_mode < 0 skips the blend). */
int  pt_query_exchange_blend(pt_ctx*, const void* tgt_xyz, int xyz_type, uint64_t m, int k, int slab_axis, const double* slab_bounds, int blend_mode,
                             uint32_t* idx_out, double* d2_out, float* rgb_out, float* nrm_out, pt_exchange_stats_t* stats_or_null);
int  pt_exchange_merge_local(pt_ctx* const* ctxs, int g, const void* const* tgt_xyz_dev, int xyz_type, const uint64_t* m, int k, int slab_axis,
                             const double* slab_bounds, uint32_t* const* idx_dev, double* const* d2_dev, int blend_mode, float* const* rgb_dev,
                             float* const* nrm_dev);

/* ---- streamed upload of a planar cloud: what a file reader feeds while it is still parsing ---------
 * Replaces the copy of the points into the tree, `Tree tree(points.begin(), points.end())` (src/pointsTransfer.cpp:259),
 * for callers that hold x[] y[] z[] (+ rgb, normals) instead of 80-byte records: 39 bytes per point cross PCIe instead of 80.
 *   pt_host_alloc / pt_host_free   page-locked host memory (what makes the copies below asynchronous)
 *   pt_upload_begin                reserve a cloud of n points of xyz_type (PT_F32 / PT_F64), with or without attributes
 *   pt_upload_range                enqueue records [first, first + count): x, y, z point at `count` coordinates each,
 *                                  rgb at count * 3 bytes, nrm at count * 3 floats (both may be NULL when begun without
 *                                  attributes).  Thread-safe: parser threads call it as their ranges complete.  The memory
 *                                  must stay valid until pt_upload_end returns.
 *   pt_upload_end                  wait for the copies, pack the attribute table and build the grid (as pt_build_soa). */
void* pt_host_alloc(uint64_t bytes);
void  pt_host_free(void*);
int   pt_upload_begin(pt_ctx*, uint64_t n, int xyz_type, int with_attributes);
int   pt_upload_range(pt_ctx*, uint64_t first, uint64_t count, const void* x, const void* y, const void* z,
                      const uint8_t* rgb, const float* nrm);
int   pt_upload_end(pt_ctx*);

/* ---- out-of-core source (reference README.md:3 "billions of points") ------------------------------------
 * Searches the RESIDENT targets (pt_targets_*) in a cloud that stays in host memory: the cloud is cut into chunks of
 * `chunk_points` consecutive points, every chunk is uploaded (the next one while the current one is being searched: keep
 * `xyz` in page-locked memory, pt_host_alloc, for that overlap), gridded and searched like a resident cloud, and the k best
 * of the chunk are merged into the running k best under the same total order (d2, index).  Indices are 64-bit -- a streamed
 * cloud may hold more than 2^32 points -- and are `first_id` + the point's position in `xyz`.  The result is bit-identical to
 * a resident search of the whole cloud.  Every target brings a bound to every chunk: its current k-th squared distance once it has a
 * list; nothing (an unbounded search) in the first chunk whose bounding box contains it; and "not now" for chunks it lies outside of
 * before it has a list -- those (target, chunk) pairs are taken up by a second, backward sweep, under a bound by then.  A chunk that
 * no target's bound reaches is not searched (forward sweep) or not even uploaded again (backward sweep): a cloud stored in spatial
 * order -- what scanners and tiled exports deliver -- costs each target its own neighbourhood's chunks, a cloud in random order costs
 * what it did before (every chunk covers everything: no pair is ever deferred, the backward sweep uploads nothing).
 * xyz: planar, n points of xyz_type (PT_F32 / PT_F64; the targets' type);
 * idx64_out / d2_out: host, [m][k].  Afterwards NO source cloud is resident in the context (the chunks lived in the stage
 * buffers): a later pt_query_* needs a pt_build_* first and fails with PT_ERR_STATE otherwise. */
int  pt_stream_query(pt_ctx*, const void* xyz, int xyz_type, uint64_t n, uint64_t chunk_points, uint64_t first_id, int k,
                     uint64_t* idx64_out, double* d2_out);

/* ---- texture bake: the consumer of the neighbour lists -------------------------------------
 * pt_bake_texture replaces the body of the reference's face loop after the search and its rasteriser
 * (src/pointsTransfer.cpp:466-581 and draw_triangle :66-107): per face, the union of its three corners' neighbour
 * lists, projection into the face plane, the in-triangle filter, a Delaunay triangulation of corners + interior
 * points, and barycentric rasterisation of every sub-triangle into a resolution x resolution BGRA atlas addressed
 * (resolution - j, i) as the reference does.  pad_ksize > 0 additionally applies the reference's edge padding
 * (:593-611: ksize x ksize dilate, ~alpha mask, saturating add; the reference uses 25) before the atlas is copied out.
 * The source cloud must be resident (pt_build_*); `mesh_vertices` are the reference's records (ver, color, U, V are
 * read), `faces` holds 3 vertex indices per face, `nbr_idx` is the [nv][k] index matrix a pt_query_* call returned
 * for those vertices.  All host memory; bgra_out receives resolution * resolution * 4 bytes (B, G, R, A).
 * Where the reference's result is decided by CGAL / OpenCV internals or by undefined behaviour the result is defined
 * by this build (oracle/pt_oracle.c states the definition; INTEGRATION.md lists the points). */
int  pt_bake_texture(pt_ctx*, const pt_point* mesh_vertices, uint64_t nv, const int32_t* faces, uint64_t nf,
                     const uint32_t* nbr_idx, int k, int resolution, int pad_ksize, uint8_t* bgra_out);
/* pt_bake_maps: the same face pass writing the colour atlas, an OBJECT-SPACE NORMAL MAP, or both, in one call -- one upload of
 * vertices, faces and lists and one face launch whatever `maps` is.  `maps` is a non-empty subset of PT_MAP_COLOR | PT_MAP_NORMAL; an
 * output whose bit is set must be non-null, one whose bit is clear is ignored (may be NULL).  Everything else -- arguments, state
 * rules, errors, pt_stats_t.ms_bake -- is pt_bake_texture's, and pt_bake_texture IS the PT_MAP_COLOR case of this call (same bytes).
 * The normal map ("Normal map"): per kept point a normal -- a corner's is the mesh vertex record's `normal`, an
 * interior point's is the source point's attribute normal as the caller uploaded it (float, widened to double; NOT normalised, so
 * a longer normal weighs more in the mix) -- and per covered pixel, with the barycentrics b of the colour mix,
 *   m = (b0 n0 + b1 n1) + b2 n2 per component,  l = sqrt((mx mx + my my) + mz mz),  u = m / l, or (0, 0, 1) unless 0 < l < inf,
 *   byte = (int)((u * 127.5 + 127.5) + 0.5) clamped to [0, 255],   pixel = {z, y, x, 255} in B, G, R, A order (R = x, G = y, B = z),
 * all in double, every operation rounded on its own.  The normals are held as doubles throughout: nothing is rounded to float.
 * The same (face, triangle) wins a pixel in both planes, so their alpha channels are equal; untouched pixels are 0.
 * The source normals are the ones the caller uploaded: a cloud built WITHOUT normals holds zero records, and a texel between such
 * points alone falls back to (0, 0, 1) -- estimate the cloud's normals first (pt_estimate_normals).  pad_ksize > 0 pads the normal
 * plane exactly like the colour plane (per-channel maximum of the window under ~alpha): the padded ring is there to keep bilinear
 * sampling off the background and is NOT unit length -- renormalise in the shader, as for any filtered normal map.
 * Device memory while the call runs, with P = resolution^2 pixels and m maps: 8 m P (keys) + 4 m P (resolved planes), and with padding
 * 4 m P + 4 P more -- all held until the planes are copied out: 1.3 GB for one padded map at 8192^2, 2.3 GB for both. */
enum { PT_MAP_COLOR = 1, PT_MAP_NORMAL = 2 };
int  pt_bake_maps(pt_ctx*, const pt_point* mesh_vertices, uint64_t nv, const int32_t* faces, uint64_t nf,
                  const uint32_t* nbr_idx, int k, int resolution, int pad_ksize, int maps,
                  uint8_t* color_bgra_out, uint8_t* normal_bgra_out);
/* pt_bake_maps_h: pt_bake_maps with a third plane, the HEIGHT MAP -- per texel the signed distance of the cloud from the face along
 * the face normal, the offset that parallax and displacement shaders read -- in the same call: one upload, one face launch whatever
 * `maps` is.  `maps` is a non-empty subset of PT_MAP_COLOR | PT_MAP_NORMAL | PT_MAP_HEIGHT; an output whose bit is set must be non-null,
 * one whose bit is clear is ignored (may be NULL).  height_range (H) must be finite and > 0 when PT_MAP_HEIGHT is set (PT_ERR_ARG
 * otherwise) and is ignored when it is clear.  State rules, the other errors and pt_stats_t.ms_bake are pt_bake_maps's (a resident
 * attribute table, PT_ERR_UNSUPPORTED on slab contexts, nf < 2^24), and pt_bake_maps IS the maps-within-{COLOR, NORMAL} case of this
 * call (same bytes); pt_bake_maps itself still refuses PT_MAP_HEIGHT.
 * The height map ("Height map"), all in double, every operation rounded on its own:
 *   face normal     with a = c1 - c0, b = c2 - c0, n = a x b:  ln = sqrt((nx nx + ny ny) + nz nz),  e3 = n / ln.  e1, e2, e3 (the bake's
 *                   plane frame) is right-handed: positive height is the side the face's winding faces
 *   heights         a corner's is 0; an interior kept point's is h = (dx e3x + dy e3y) + dz e3z with d = the source point (widened
 *                   exactly to double) - c0, the differences the projection forms.  Unless 0 < ln < inf every interior point of the
 *                   face has h = 0
 *   per pixel       m = (b0 h0 + b1 h1) + b2 h2 with the barycentrics b of the colour mix.  m not finite: byte = 128.  Otherwise
 *                   t = m / H,  u = t * 127.5 + 127.5,  byte = (int)min(max(u + 0.5, 0), 255):  0 -> 128, +H -> 255, -H -> 0, saturating
 *   pixel           {byte, byte, byte, 255} in B, G, R, A order (grey, so the padding's per-channel maximum and the PNG writer agree)
 * The same (face, triangle) wins a pixel in every requested plane, so their alpha channels are equal; untouched pixels are 0.  A face
 * with no interior point is 128 throughout.  Along a face's own edges the interior points' barycentrics vanish, so the height there
 * is 0: the field is continuous across faces and pinned to the mesh at its edges.  pad_ksize > 0 pads the height plane exactly like
 * the colour plane.
 * result_or_null->max_abs_height: the maximum of |h| over all interior kept points whose h is finite, across all well-formed faces;
 * 0 when there is none or when PT_MAP_HEIGHT is clear.  A maximum does not depend on the order of its terms: it is exact and the same
 * on every run.  The weights are >= 0 and sum to 1, so H >= max_abs_height means nothing saturates (up to the last rounding): bake
 * once with any H to learn it, then choose H.
 * Device memory while the call runs, with P = resolution^2 pixels and m <= 3 maps: 8 m P (keys) + 4 m P (resolved planes), and with
 * padding 4 m P + 4 P more -- all held until the planes are copied out: 3.4 GB for three padded maps at 8192^2. */
enum { PT_MAP_HEIGHT = 4 };
typedef struct pt_bake_result_t { double max_abs_height; } pt_bake_result_t;
int  pt_bake_maps_h(pt_ctx*, const pt_point* mesh_vertices, uint64_t nv, const int32_t* faces, uint64_t nf,
                    const uint32_t* nbr_idx, int k, int resolution, int pad_ksize, int maps, double height_range,
                    uint8_t* color_bgra_out, uint8_t* normal_bgra_out, uint8_t* height_bgra_out,
                    pt_bake_result_t* result_or_null);
/* The edge padding alone (reference :593-611) on a host BGRA image. */
int  pt_texture_pad(pt_ctx*, const uint8_t* bgra_in, int resolution, int ksize, uint8_t* bgra_out);

#ifdef __cplusplus
}
#endif
#endif /* PT_API_H */
