/*
 * C ABI of the MI355X-native KaMinPar label-propagation hot path.
 *
 * This is the drop-in boundary for the reference's LP operator seams:
 *   - kmp_lp_cluster_*  replaces Clusterer::compute_clustering behind
 *     kaminpar-shm/coarsening/clusterer.h:19-47 (LPClustering,
 *     lp_clusterer.cc:395) including set_max_cluster_weight /
 *     set_desired_cluster_count (clusterer.h:35-36);
 *   - kmp_lp_refine_*   replaces Refiner::refine behind
 *     kaminpar-shm/refinement/refiner.h:18-57 (LabelPropagationRefiner,
 *     lp_refiner.cc:370-372);
 *   - graph handles keep the reference CSR layout exactly
 *     (CSRGraphMemory, kaminpar-shm/datastructures/csr_graph.h:27-33:
 *     xadj[n+1], adjncy[m] with both arc directions, optional vwgt/adjwgt);
 *   - kmp_edge_cut mirrors metrics::edge_cut (kaminpar-shm/metrics.cc:37-59).
 *
 * Types follow include/kaminpar-shm/ckaminpar.h:27-52: NodeID/EdgeID u32
 * (u64 edge ids are a planned variant for >4G-arc graphs), NodeWeight/
 * EdgeWeight i32, BlockID u32, BlockWeight i64 here (the reference uses
 * NodeWeight-width block weights; i64 caps avoid overflow at scale-28).
 *
 * Plain pointers and sizes only; no torch types. Compute entry points
 * REQUIRE a GPU (they abort with a clear error if no HIP device is present);
 * graph generation/IO entry points are host-only.
 */
#ifndef KAMINPAR_LP_H
#define KAMINPAR_LP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kmp_graph_t kmp_graph_t; /* host-resident CSR graph */
typedef struct kmp_lp_t kmp_lp_t;       /* device-resident LP engine */

/* ---------------------------------------------------------------- graphs */

/* Copy a CSR graph (reference layout, csr_graph.h:27-33). vwgt/adjwgt may be
 * NULL for unit weights. Returns NULL on invalid input. */
kmp_graph_t *kmp_graph_from_csr(
    uint32_t n,
    uint64_t m,
    const uint32_t *xadj,
    const uint32_t *adjncy,
    const int32_t *vwgt,
    const int32_t *adjwgt
);

/* Graph500-parameter R-MAT generator (a=.57,b=.19,c=.19,d=.05), symmetrized
 * and deduplicated, unit weights; deterministic in (scale, edgefactor, seed).
 * n = 2^scale, #undirected edges before dedup = edgefactor * n. */
kmp_graph_t *kmp_gen_rmat(int scale, int edgefactor, uint64_t seed);

/* 2D random geometric graph on the unit square: n points, radius chosen for
 * the given average degree; deterministic in (n, avg_deg, seed). */
kmp_graph_t *kmp_gen_rgg2d(uint32_t n, double avg_deg, uint64_t seed);

/* METIS ASCII reader (kaminpar-io/metis_parser.h:17-25 format). */
kmp_graph_t *kmp_read_metis(const char *path);

/* METIS ASCII writer (counterpart of kmp_read_metis). */
int kmp_write_metis(const kmp_graph_t *g, const char *path);

/* ParHIP binary reader/writer (docs/graph_file_format.md "ParHIP Graph
 * File Format"; kaminpar-io/parhip_parser.cc:42-136): 24-byte header
 * (version bit-field, n, m), byte offsets, adjacency, optional weights.
 * Reader accepts 32- and 64-bit stored ids/weights that fit u32/i32;
 * writer emits 32-bit ids (64-bit offsets when the file is large). */
kmp_graph_t *kmp_read_parhip(const char *path);
int kmp_write_parhip(const kmp_graph_t *g, const char *path);

/* EdgeID-64 construction (ckaminpar.h:33-37 KAMINPAR_64BIT_EDGE_IDS
 * analogue): CSR with 64-bit offsets for graphs of >= 2^32 directed arcs.
 * Such graphs run on the LP engine (device offsets are always 64-bit);
 * host-side utilities (IO, rearrangement, host edge cut) require 32-bit. */
kmp_graph_t *kmp_graph_from_csr64(
    uint32_t n,
    uint64_t m,
    const uint64_t *xadj,
    const uint32_t *adjncy,
    const int32_t *vwgt,
    const int32_t *adjwgt
);
const uint64_t *kmp_graph_xadj64(const kmp_graph_t *g); /* null if 32-bit */

uint32_t kmp_graph_n(const kmp_graph_t *g);
uint64_t kmp_graph_m(const kmp_graph_t *g); /* number of directed arcs */
const uint32_t *kmp_graph_xadj(const kmp_graph_t *g);
const uint32_t *kmp_graph_adjncy(const kmp_graph_t *g);
const int32_t *kmp_graph_vwgt(const kmp_graph_t *g);     /* NULL if unit */
const int32_t *kmp_graph_adjwgt(const kmp_graph_t *g);   /* NULL if unit */
int64_t kmp_graph_total_node_weight(const kmp_graph_t *g);
void kmp_graph_free(kmp_graph_t *g);

/* Sequential host edge cut of a labelling (metrics.cc:73-84). */
int64_t kmp_edge_cut_host(const kmp_graph_t *g, const uint32_t *labels);

/* Degree-bucket rearrangement (the reference's default preprocessing,
 * NodeOrdering::DEGREE_BUCKETS: graphutils/permutator.h:30-128, stable
 * counting sort by floor_log2(deg)+1 with isolated vertices last).
 * perm_out[u_old] = u_new, n entries; returns the permuted graph. */
kmp_graph_t *kmp_rearrange_degree_buckets(const kmp_graph_t *g,
                                          uint32_t *perm_out);

/* Max block weight as the reference's PartitionContext computes it for
 * uniform epsilon (context.cc:27-39): (1+eps) * ceil(total_weight / k). */
int64_t kmp_max_block_weight(const kmp_graph_t *g, uint32_t k, double eps);

/* ------------------------------------------------------------- LP engine */

/* Run statistics, filled by the compute entry points. */
typedef struct kmp_lp_stats_t {
  uint64_t arcs_scanned;    /* directed arcs scanned over all sweeps */
  uint64_t moves;           /* committed moves */
  uint64_t phase_a_ns;      /* HIP-event time in gain/select kernels */
  uint64_t total_ns;        /* wall time of the LP region (device-synced) */
  uint64_t num_clusters;    /* clusterer: final non-empty clusters */
  int64_t edge_cut;         /* refiner: final cut (device-computed) */
} kmp_lp_stats_t;

/* Create an engine on the current HIP device and upload the graph.
 * Aborts (returns NULL + message on stderr) if no GPU is available. */
kmp_lp_t *kmp_lp_create(const kmp_graph_t *g);
void kmp_lp_free(kmp_lp_t *e);

/* Largest k of kmp_lp_refine and kmp_lp_balance. Labels, proposal targets
 * and the commit's sort keys are 32-bit, so nothing in the kernels sets a
 * tighter bound; 2^24 bounds the per-call k-sized device arrays (36 bytes per
 * block, ~600 MB) and the host's O(k) scans. kmp_lp_jet, kmp_lp_rebalance,
 * kmp_lp_underload and kmp_lp_extract_subgraphs keep k-sized LDS tables and
 * stay at k <= 2048. */
#define KMP_LP_MAX_K (1u << 24)

/* Deterministic LP refinement (chunk-synchronous schedule; see
 * oracle/lp_oracle.cpp header for the schedule contract). partition: in/out,
 * n entries, values < k <= KMP_LP_MAX_K. max_block_weights: k entries. Returns
 * the final edge cut, or -1 on error (k above the limit; for k > 2048 also a
 * label >= k; reported on stderr before anything is allocated).
 * partition == NULL: the resident form (see "resident labels" below).
 * Gain tiers by degree. k <= 2048: dense tables (deg <= 16 in registers,
 * <= 2048 a per-wave LDS table of k counters, above that a global row of k
 * counters per vertex). k > 2048: containers sized by degree, not by k
 * (deg <= 16 in registers, <= 512 a per-wave 1024-slot LDS hash, <= 1536 a
 * per-workgroup 4096-slot LDS hash, above that a pooled global hash); the
 * gathers read the u16 label shadow up to k = 65536 and the u32 labels
 * beyond. Both give the oracle's result bit for bit. */
int64_t kmp_lp_refine(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    uint32_t *partition,
    uint64_t seed,
    int iters,
    kmp_lp_stats_t *stats
);

/* Overload-balancer mode (the role of the reference's OVERLOAD_BALANCER
 * bracketing LP in the default refiner chain, presets.cc refinement
 * algorithms list): same deterministic schedule and commit as
 * kmp_lp_refine, but a vertex whose block exceeds its cap loses "stay" as
 * a candidate, so overloaded blocks shed boundary vertices to the best
 * admissible targets even at negative gain. Use before kmp_lp_refine when
 * the input partition may violate the caps. Returns the edge cut, or -1.
 * k <= KMP_LP_MAX_K, with kmp_lp_refine's tiers. Two parts run on the host at
 * any k: isolated vertices of over-cap blocks go to the lightest block with
 * room (lowest id on ties; blocks kept ordered by weight), and every chunk
 * scans the k downloaded weights for its fallback target
 * (kmp_lp_balance_host_ns). */
/* Underload-balancer mode (presets.cc:332-338 UNDERLOAD_BALANCER;
 * refinement/balancer/underload_balancer.cc semantics): fill blocks below
 * min_block_weights[b] with best-gain admissible vertices, never dropping a
 * source below its own minimum and never overshooting any maximum. A no-op
 * when all minima are already satisfied (the reference's refine() gate).
 * k <= 2048; -1 above. */
/* Clusterer::set_communities (coarsening/clusterer.h:35,
 * lp_clusterer.cc:61-66,193-194): when set (len n), kmp_lp_cluster never
 * merges vertices across community boundaries. NULL clears. The array's
 * maximum + 1 is kept as the communities' bound (see "V-cycle pieces"). */
int kmp_lp_set_communities(kmp_lp_t *e, const uint32_t *communities);

/* On-GPU degree-bucket rearrangement (permutator.cc:36-110 semantics,
 * bit-identical to kmp_rearrange_degree_buckets): rebuilds the engine's
 * device CSR in log2-degree-bucket order, writes perm_out[u_old] = u_new
 * (len n). Call before refine/cluster; map partitions through perm_out. */
int kmp_lp_rearrange_degree_buckets(kmp_lp_t *e, uint32_t *perm_out);

int64_t kmp_lp_underload(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    const int64_t *min_block_weights,
    uint32_t *partition,
    uint64_t seed,
    int iters,
    kmp_lp_stats_t *stats
);

int64_t kmp_lp_balance(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    uint32_t *partition,
    uint64_t seed,
    int iters,
    kmp_lp_stats_t *stats
);

/* Host time of the engine's last kmp_lp_balance call, in ns: out[0] the
 * isolated-vertex pre-pass (weights download included), out[1] the per-chunk
 * weight downloads + lightest-block-with-room scans, summed over the call. */
void kmp_lp_balance_host_ns(const kmp_lp_t *e, uint64_t out[2]);

/* ------------------------------------------------------------ Jet refiner
 * GPU restatement of the reference's Jet refiner
 * (kaminpar-shm/refinement/jet/jet_refiner.cc:94-234), the refiner to bind
 * behind refinement/refiner.h when LP alone is too weak and the graph is too
 * large for the CPU FM. Every iteration is synchronous on a snapshot:
 *   find     each unlocked boundary vertex picks the adjacent block with the
 *            largest connectivity (ties: smallest id) and keeps the move iff
 *            gain > -floor(temp * own connectivity)  (jet_refiner.cc:108-131)
 *   filter   the afterburner re-evaluates each candidate assuming neighbours
 *            with a higher gain (ties: lower id) already moved; moves with a
 *            positive re-evaluated gain are executed and locked for the next
 *            iteration, all other locks are cleared (jet_refiner.cc:133-190)
 *   balance  only if a block now exceeds its cap. balancer == 0: balance_iters
 *            sweeps of this engine's deterministic overload-balancer mode
 *            (kmp_lp_balance semantics, seed + global iteration index).
 *            balancer == 1: up to balance_passes passes of the selection
 *            rebalancer (kmp_lp_rebalance below), the rule of the reference's
 *            priority-queue OverloadBalancer
 *            (refinement/balancer/overload_balancer.cc:162-271, ordered by
 *            refinement/balancer/relative_gain.h) restated as fixed-shape
 *            passes; balance_iters and the seed are then ignored
 *   score    edge cut + feasibility; the best state seen is snapshotted and
 *            restored at the end of every round (jet_refiner.cc:196-231).
 * A state becomes the best iff it gains feasibility, or matches the best
 * state's feasibility with a cut <= the best cut. The fruitless counter grows
 * every iteration and resets when feasibility is gained or the cut improves
 * on the best cut by more than (1 - fruitless_threshold) * best cut.
 * Bit-identical to the numpy twins tests/jet_twin.py (balancer 0) and
 * tests/rebalance_twin.py (balancer 1). Always obtain the parameters from
 * kmp_jet_params_default and override fields: the struct grows at its end. */
#define KMP_JET_BALANCER_LP 0
#define KMP_JET_BALANCER_SELECT 1
typedef struct kmp_jet_params_t {
  int num_rounds;             /* >= 1; presets.cc:410-422 default 1 */
  int max_iterations;         /* per round, 0 = unbounded (default 0) */
  int max_fruitless;          /* per round, 0 = unbounded (default 12) */
  double fruitless_threshold; /* default 0.999 */
  double initial_gain_temp;   /* round 0 temperature */
  double final_gain_temp;     /* last round; one round runs at the mean */
  int balance_iters;          /* balancer sweeps per rebalance, >= 1 */
  int balancer;               /* 0 = LP balance sweeps (default), 1 = selection */
  int balance_passes;         /* balancer == 1: passes per rebalance, >= 1 (16) */
} kmp_jet_params_t;

/* Reference defaults (presets.cc:410-422): 1 round, unbounded iterations,
 * 12 fruitless iterations, threshold 0.999, gain temperature 0.75 on coarse
 * levels (coarse_level != 0) and 0.25 on the finest. balance_iters has no
 * reference counterpart; its default 2 is the measured choice (DESIGN.md
 * section 8: one sweep often fails to restore feasibility on R-MAT graphs,
 * and an infeasible iteration can never become the best state). balancer
 * defaults to 0 (the LP balance sweeps) and balance_passes to 16. */
kmp_jet_params_t kmp_jet_params_default(int coarse_level);

/* Largest k of kmp_lp_jet (its k-sized LDS tables). */
#define KMP_JET_MAX_K 2048u

/* 1 iff kmp_lp_jet accepts these parameters, 0 otherwise (NULL included).
 * Host-only: touches no engine and no GPU. */
int kmp_jet_params_valid(const kmp_jet_params_t *params);

typedef struct kmp_jet_stats_t {
  uint64_t iterations;      /* Jet iterations over all rounds */
  uint64_t balancer_calls;  /* iterations that needed the rebalance step */
  uint64_t jet_moves;       /* moves executed by the afterburner */
  uint64_t balancer_moves;  /* moves committed by the balance sweeps / admitted
                               by the selection rebalancer */
  uint64_t arcs_scanned;    /* arcs read by find + filter (balancer excluded) */
  uint64_t find_filter_ns;  /* HIP-event time in the find + filter kernels */
  uint64_t total_ns;        /* wall time of the whole call (device-synced) */
  int64_t edge_cut;         /* cut of the returned partition */
  uint64_t balancer_ns;     /* wall time of the rebalance steps (device-synced) */
  uint64_t balancer_passes; /* balancer == 1: passes over all rebalance steps */
  uint64_t feasible_iterations; /* iterations that ended within the caps */
} kmp_jet_stats_t;

/* partition: in/out, n entries, values < k <= 2048; NULL selects the resident
 * form (see "resident labels" below). Returns the cut of the
 * returned (best) partition, or -1 on error (k too large, a label >= k or
 * bad parameters, reported on stderr). For a feasible input the result is feasible and its
 * cut is never larger than the input's. At least one of max_iterations and
 * max_fruitless must be non-zero. */
int64_t kmp_lp_jet(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    uint32_t *partition,
    uint64_t seed,
    const kmp_jet_params_t *params,
    kmp_jet_stats_t *stats
);

/* ------------------------------------------------ selection rebalancer
 * Repairs an over-cap partition the way the reference's OverloadBalancer does
 * (refinement/balancer/overload_balancer.cc:162-271): every overloaded block
 * gives up the vertices with the best relative gain
 * (refinement/balancer/relative_gain.h) until its overload is covered. The
 * priority queue becomes score, sort, prefix-select and apply over a
 * snapshot. Pass p = 0, 1, ... is a pure function of the labels L, the block
 * weights W and the caps C; all arithmetic is integer (int64):
 *   tables   over[b] = W[b] - C[b] (source blocks: over > 0; none: stop),
 *            room[b] = C[b] - W[b], cum[b] = inclusive prefix sum of
 *            max(room, 0), R = cum[k - 1], t* = the block with the largest
 *            room (ties: smallest id)
 *   score    every vertex u of weight w >= 1 in a source block: conn[b] = the
 *            weight of u's arcs into block b, own = conn[L[u]]; block b is
 *            eligible iff b != L[u] and room[b] >= w. Target: the eligible
 *            block with the largest conn[b] > 0 (ties: smallest id). Without
 *            one: if R > 0, r = splitmix64((p << 32) | u) mod R (unsigned) and
 *            the first b with cum[b] > r, if room[b] >= w; else t*, if
 *            room[t*] >= w; else u is no candidate in this pass.
 *            gain = conn[target] - own (conn = 0 for a fallback target);
 *            key = min(gain * w, 2^31 - 1) << 20 if gain > 0, otherwise
 *            -(((-gain) << 20) / w) with a truncating division
 *   select   per source block, candidates by (key desc, id asc): u is
 *            selected iff the weight of the candidates before it is below
 *            over[block] -- the shortest prefix that covers the overload
 *   admit    per target t, selected moves by (key desc, id asc): a move is
 *            admitted iff W[t] + its inclusive prefix weight <= C[t]. Targets
 *            are never sources, so no cap is overshot and the total overload
 *            never grows; rejected moves are retried in the next pass
 *   apply    the admitted moves.
 * The call stops when no block is over its cap, after a pass that admits
 * nothing (stalled), or after max_passes passes. Bit-identical to the numpy
 * twin tests/rebalance_twin.py. */
typedef struct kmp_rebalance_stats_t {
  uint64_t passes;        /* passes run, a stalled last one included */
  uint64_t selected;      /* selected moves over all passes */
  uint64_t moves;         /* admitted (applied) moves */
  uint64_t arcs_scanned;  /* arcs of the scored vertices */
  uint64_t score_ns;      /* HIP-event time in the score step */
  uint64_t total_ns;      /* wall time of the whole call (device-synced) */
  int64_t edge_cut;       /* cut of the returned partition */
  int32_t feasible;       /* 1 iff every block is within its cap on return */
} kmp_rebalance_stats_t;

/* partition: in/out, n entries, values < k <= 2048 (NULL: the resident form,
 * see "resident labels" below); max_passes >= 1. Returns
 * the cut of the returned partition, or -1 on error (k too large, a label
 * >= k or max_passes < 1, reported on stderr). A feasible input is returned
 * unchanged with 0 passes; a stalled call returns what it reached with
 * feasible = 0. */
int64_t kmp_lp_rebalance(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    uint32_t *partition,
    int max_passes,
    kmp_rebalance_stats_t *stats
);

/* Deterministic LP clustering (coarsening instantiation; clusters start as
 * singletons, uniform cap, isolated-node + two-hop passes). clustering: out,
 * n entries; NULL skips the download and leaves the clustering resident only
 * (see "resident labels" below). Returns the number of non-empty clusters,
 * or -1 on error. */
int64_t kmp_lp_cluster(
    kmp_lp_t *e,
    int64_t max_cluster_weight,
    uint32_t desired_clusters,
    uint32_t *clustering,
    uint64_t seed,
    int iters,
    kmp_lp_stats_t *stats
);

/* --------------------------- sharded (multi-GPU) refinement sub-steps ----
 * One process per GPU; rank r of world R computes phase A for its slice of
 * each chunk's position range, the proposal lists are all-gathered by the
 * caller (RCCL via torch.distributed), and every rank runs the identical
 * deterministic commit, so all replicas stay bit-identical (mirrors the
 * ghost-label exchange of kaminpar-dist/coarsening/clustering/lp/
 * global_lp_clusterer.cc:480-594 with labels replicated instead of owned).
 *
 * Proposals are 16-byte records {u, to, rank_in_chunk, weight} (uint32x4). */

/* Initialize a sharded refinement run. partition: host, n entries. */
int kmp_lp_refine_begin(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    const uint32_t *partition,
    uint64_t seed
);

/* Number of chunks per sweep (fixed by the schedule). */
uint32_t kmp_lp_num_chunks(const kmp_lp_t *e);

/* Phase A for chunk `chunk` of sweep `iter`, positions [pos_lo, pos_hi).
 * Writes proposals to the DEVICE buffer d_out (capacity cap records) and
 * returns the record count (host), or -1 on error/overflow. */
int64_t kmp_lp_phase_a(
    kmp_lp_t *e, int iter, uint32_t chunk, uint32_t pos_lo, uint32_t pos_hi,
    void *d_out, uint32_t cap
);

/* Commit `count` proposals (DEVICE buffer d_props, 16B records; may be the
 * concatenation of all ranks' phase-A outputs in rank order) for chunk
 * `chunk` of sweep `iter`. Returns committed moves, or -1 on error. */
int64_t kmp_lp_commit(
    kmp_lp_t *e, int iter, uint32_t chunk, const void *d_props, uint32_t count
);

/* Finish a sharded run: download the partition, report stats. */
int64_t kmp_lp_refine_end(kmp_lp_t *e, uint32_t *partition, kmp_lp_stats_t *stats);

/* ------------------- device-resident stepping (benchmark region) ---------
 * The timed region excludes host transfers and the final edge-cut kernel,
 * matching the reference's LP-only timing
 * (shm_label_propagation_benchmark.cc:121-123). */
/* Sharded deterministic commit (multi-GPU): rank owns targets [c_lo,c_hi)
 * of the ALL-GATHERED proposal list (global rank order). Protocol per chunk
 * (mirrors kaminpar-dist/refinement/lp/lp_refiner.cc:296-333):
 *   shard_begin  -> local sort + full-admission departure contributions
 *                   into d_dep_out (k+1 i64; caller allreduce-sums = global)
 *   loop: shard_round(dep_global) -> d_delta_out (k+1; [k]=changed);
 *         caller allreduces, subtracts delta from dep_global, repeats
 *         until the summed changed flag is 0
 *   shard_finish_meta -> own targets' rank cutoffs + admitted arrivals
 *                   (caller allreduce-sums both = allgather)
 *   shard_apply  -> every rank applies the identical admitted set + weight
 *                   updates + active-set maintenance; returns moves.
 * All d_* pointers are DEVICE pointers. Bit-identical to kmp_lp_commit. */
/* Adopt an external HIP stream (e.g. torch's current stream) so the
 * multi-GPU collectives and the engine's kernels share one stream; pass
 * NULL to restore the engine's own stream. Engine must be idle. */
int kmp_lp_set_stream(kmp_lp_t *e, void *external_stream);

int kmp_lp_shard_begin(kmp_lp_t *e, uint32_t c_lo, uint32_t c_hi,
                       const void *d_props, uint32_t count, long long *d_dep_out);
int kmp_lp_shard_round(kmp_lp_t *e, uint32_t c_lo, uint32_t c_hi,
                       const long long *d_dep_global, long long *d_delta_out);
int kmp_lp_shard_finish_meta(kmp_lp_t *e, uint32_t c_lo, uint32_t c_hi,
                             unsigned long long *d_cutoff_out,
                             long long *d_arr_out);
int64_t kmp_lp_shard_apply(kmp_lp_t *e, int iter, uint32_t chunk,
                           const void *d_props, uint32_t count,
                           const unsigned long long *d_cutoff_all,
                           const long long *d_arr_all,
                           const long long *d_dep_global);

/* C++ RCCL distributed driver: the whole sharded-commit chunk loop with
 * collectives issued directly on the engine stream (the python/torch
 * orchestration has a measured ~0.65 ms/chunk host floor; this driver's
 * per-chunk host work is the fixpoint convergence readback only).
 * Bootstrap: rank 0 calls kmp_nccl_unique_id, the 128-byte id is
 * exchanged out of band (e.g. a torch.distributed broadcast), every rank
 * calls kmp_nccl_comm_init. nccl_comm may be NULL at world 1. */
int kmp_nccl_unique_id(void *out128);
void *kmp_nccl_comm_init(int world, int rank, const void *id128);
void kmp_nccl_comm_destroy(void *comm);
int64_t kmp_lp_refine_dist(
    kmp_lp_t *e,
    uint32_t k,
    const int64_t *max_block_weights,
    uint32_t *partition,
    uint64_t seed,
    int iters,
    void *nccl_comm,
    int rank,
    int world,
    kmp_lp_stats_t *stats
);

int kmp_lp_reset(kmp_lp_t *e);                     /* restore initial state (D2D) */
int64_t kmp_lp_run_sweeps(kmp_lp_t *e, int iters); /* the timed LP region */
int kmp_lp_get_stats(kmp_lp_t *e, kmp_lp_stats_t *stats); /* no cut/download */

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* KAMINPAR_LP_H */
/* ---------------------------------------------------------------- v1.1 ---
 * Cluster contraction on the GPU (restates
 * kaminpar-shm/coarsening/contraction/ semantics: coarse id = prefix rank of
 * occupied cluster ids, intra-cluster edges dropped, parallel edges merged
 * with summed weights, coarse adjacency sorted by (cu, cv)). Returns the
 * coarse node count; *coarse_out receives a new host graph handle and
 * mapping_out (n entries) the fine->coarse projection. -1 on error. */
#ifdef __cplusplus
extern "C" {
#endif
int64_t kmp_contract(
    kmp_lp_t *e,
    const uint32_t *clustering,
    uint32_t *mapping_out,
    kmp_graph_t **coarse_out
);

/* Contract and hand the coarse graph DIRECTLY to a new engine without the
 * host round-trip (device-resident multilevel chain; the coarse CSR stays
 * in HBM). mapping_out (n entries, host) is still produced. The new engine
 * owns the coarse graph; use kmp_lp_download_graph when a host copy is
 * needed (e.g. the coarsest level for initial partitioning). Identical
 * results to kmp_contract + kmp_lp_create on the downloaded graph.
 * clustering == NULL contracts the resident clustering of e (-1 unless e holds
 * one) in place; the new engine's isolated-vertex list is then found on the
 * device and the coarse xadj / vwgt never leave HBM. mapping_out == NULL
 * skips the mapping download. In every form the new engine keeps the device
 * mapping (4 bytes per vertex of e, freed with it) for kmp_lp_project. The
 * new engine is the same in every form. */
int64_t kmp_contract_engine(
    kmp_lp_t *e,
    const uint32_t *clustering,
    uint32_t *mapping_out,
    kmp_lp_t **coarse_eng_out
);

/* ------------------------------------- threshold edge sparsification
 * kmp_contract_engine with the reference's sparsifying coarsener
 * (kaminpar-shm/coarsening/sparsification_cluster_coarsener.cc, preset
 * linear-time-kway): after the contraction the heaviest coarse arcs are kept
 * up to a target and the ties at the threshold weight are sampled. The pass
 * runs on the contraction's device output, on the engine's stream, before the
 * new engine adopts it; nothing n- or m-sized reaches the host because of it.
 * With old_n, old_m the n and m of e, and c_n, c_m those of the contraction:
 *   target   min(edge_target_factor * old_m,
 *                density_target_factor * old_m / old_n * c_n), evaluated left
 *            to right in double, truncated, capped at old_m
 *   applied  iff c_m > laziness_factor * target (in double) and c_m > target;
 *            otherwise the call equals kmp_contract_engine exactly
 *   target < 2: every arc is dropped. Otherwise T is the (c_m - target + 1)-th
 *            smallest arc weight, larger = #{w > T}, equal = #{w == T},
 *            include = target - larger, and arc (u, v, w) is kept iff w > T, or
 *            w == T and h(u, v) * equal < include * 2^32 in 64-bit unsigned
 *            arithmetic. h is the low 32 bits of the 64-bit Murmur3 finalizer
 *            of ((max(u, v) << 32) | min(u, v)) + seed, the reference's dice;
 *            the integer comparison replaces its division in double (the one
 *            deviation, made so that device and CPU twin agree bit for bit).
 *            The predicate is symmetric, so the graph stays undirected; the
 *            kept count is near target, not equal to it.
 * Rows keep their order, xadj is rebuilt, arc and vertex weights, c_n and the
 * mapping are unchanged; vertices may become isolated. The new engine's m,
 * its isolated-vertex list and all other derived state come from the
 * sparsified graph, and it keeps the parent mapping (kmp_lp_project,
 * kmp_lp_restrict). A result with zero arcs is a legal engine. Bit-identical
 * to the numpy twin tests/sparsify_twin.py. */
typedef struct kmp_sparsify_params_t {
  double density_target_factor; /* default 0.5 */
  double edge_target_factor;    /* default 0.5 */
  double laziness_factor;       /* default 4 */
} kmp_sparsify_params_t;
kmp_sparsify_params_t kmp_sparsify_params_default(void);
/* 1 iff every factor is finite and > 0 and laziness_factor >= 1 */
int kmp_sparsify_params_valid(const kmp_sparsify_params_t *p);

typedef struct kmp_sparsify_stats_t {
  uint64_t applied;   /* 0 | 1 */
  uint64_t m_before;  /* c_m of the contraction */
  uint64_t m_after;   /* arcs of the new engine */
  uint64_t target;
  uint64_t threshold; /* T; 0 when not applied or target < 2, as the next three */
  uint64_t larger, equal, include;
  uint64_t pass_ns;   /* HIP-event time of the pass; 0 when not applied */
} kmp_sparsify_stats_t;

/* Arguments as kmp_contract_engine, in each of its forms. params == NULL
 * means kmp_sparsify_params_default(); invalid params return -1 with one line
 * on stderr before anything is launched. stats_out may be NULL. */
int64_t kmp_contract_engine_sparsified(
    kmp_lp_t *e,
    const uint32_t *clustering,
    uint32_t *mapping_out,
    const kmp_sparsify_params_t *params,
    uint64_t seed,
    kmp_lp_t **coarse_eng_out,
    kmp_sparsify_stats_t *stats_out
);

/* ------------------------------------------------------ resident labels
 * An engine's own label array can carry a partition or a clustering from one
 * call to the next, so that nothing of size n crosses PCIe between the stages
 * of the multilevel chain. The engine records what the array holds:
 *   nothing     after kmp_lp_create, and in a new engine made by
 *               kmp_contract_engine or kmp_subgraphs_engine
 *   clustering  after a successful kmp_lp_cluster
 *   partition   with a bound k (all labels < k), after a successful
 *               kmp_lp_refine, kmp_lp_jet or kmp_lp_rebalance (the call's k,
 *               host and resident form alike), kmp_lp_set_labels,
 *               kmp_lp_project, kmp_lp_restrict (on the coarse engine) or
 *               kmp_lp_labels_from_communities
 *               (the host form of kmp_lp_refine takes its caller's word that
 *               the labels are below k, as it always has; all others check)
 * Each of these calls records "nothing" on entry and the new state only on
 * success. Every other entry point that writes the label array records
 * "nothing" as well, conservatively, whatever it leaves there: kmp_lp_balance,
 * kmp_lp_underload, kmp_lp_refine_begin / _end, kmp_lp_commit, the
 * kmp_lp_shard_* calls, kmp_lp_refine_dist, kmp_lp_run_sweeps, kmp_lp_reset
 * and kmp_lp_rearrange_degree_buckets.
 *
 * Resident form of kmp_lp_refine / kmp_lp_jet / kmp_lp_rebalance
 * (partition == NULL): starts from the resident partition and leaves the
 * result resident; no upload, no download, no validation pass. It fails with
 * -1 and a message iff the engine holds no partition or its bound exceeds the
 * call's k; this is decided on the host before anything is launched. Return
 * value and stats are those of the host form on the same labels.
 * kmp_lp_balance, kmp_lp_underload, kmp_contract and kmp_lp_extract_subgraphs
 * have no resident form. */

/* Checks on the host that every value is below k, then uploads the partition
 * (n entries); the engine then holds partition(k). Returns -1 on a label >= k,
 * before anything is uploaded. */
int kmp_lp_set_labels(kmp_lp_t *e, uint32_t k, const uint32_t *partition);

/* Downloads the resident partition or clustering (n entries). -1 if the engine
 * holds nothing. */
int kmp_lp_get_labels(const kmp_lp_t *e, uint32_t *out);

/* fine.labels[u] = coarse.labels[mapping[u]], on the device, where mapping is
 * the fine-to-coarse map of the kmp_contract_engine call that made coarse.
 * coarse must hold a partition and fine must be the engine coarse was
 * contracted from (coarse remembers that engine's address and n, to compare
 * only); -1 otherwise. fine then holds a partition with the same bound k. The
 * call is ordered after everything issued to either engine's stream and
 * before everything issued later; it does not wait on the host.
 * kmp_lp_rearrange_degree_buckets on the fine engine after the contraction
 * invalidates the mapping: contract again. */
int kmp_lp_project(kmp_lp_t *coarse, kmp_lp_t *fine);

/* ------------------------------------------------------ V-cycle pieces
 * What a V-cycle (kmp_vcycle_ex below) needs beyond the calls above: the
 * engine's partition as the clusterer's communities, its restriction to the
 * coarse level, and the way back after clustering overwrote the labels. The
 * communities are an array of their own next to the labels; they carry a
 * bound like a partition does: max + 1 of the array kmp_lp_set_communities
 * uploaded, the partition's k after kmp_lp_set_communities_resident. */

/* communities := the resident partition, copied on the device; the labels stay
 * as they are. -1 unless the engine holds a partition. The clusterer's host
 * chain over the isolated vertices gets their communities through a gather of
 * that many entries; nothing n-sized crosses PCIe, and
 * kmp_lp_label_traffic_bytes does not move. kmp_lp_set_communities(e, NULL)
 * clears these communities as it clears uploaded ones. */
int kmp_lp_set_communities_resident(kmp_lp_t *e);

/* The counterpart of kmp_lp_project: coarse.labels[mapping[u]] =
 * fine.communities[u] for every fine vertex u, on the device, where mapping is
 * the fine-to-coarse map coarse keeps from its kmp_contract_engine call. A
 * second pass counts the u whose coarse slot holds another value than their
 * community: a clustering that respects the communities gives 0; anything else
 * fails the call (-1, the count on stderr) and coarse then holds nothing. That
 * count is the only host read. On success coarse holds a partition with the
 * communities' bound (the label array only: the next refiner call rebuilds
 * its narrow copies, as after kmp_lp_project). Fails on the host, before any
 * launch, if fine has no communities, their bound exceeds KMP_LP_MAX_K, or
 * coarse was not contracted from fine. Ordered on both engines' streams as
 * kmp_lp_project is, but waits for the count. */
int kmp_lp_restrict(kmp_lp_t *fine, kmp_lp_t *coarse);

/* labels := communities on the device, narrow copies included; the engine then
 * holds a partition with the communities' bound. This is how a partition comes
 * back after kmp_lp_cluster overwrote it. -1 without communities or with a
 * bound above KMP_LP_MAX_K. */
int kmp_lp_labels_from_communities(kmp_lp_t *e);

/* Edge cut of the resident partition (the value kmp_lp_refine would return
 * for it) and, in *feasible (may be NULL), whether every block b < k weighs at
 * most max_block_weights[b] (k entries). The labels are not touched; the host
 * reads the cut and, where feasible is given, k block weights.
 * max_block_weights may be NULL iff feasible is. -1 iff the engine holds no
 * partition, its bound exceeds k, or feasible comes without caps; decided
 * before any launch. Any k up to KMP_LP_MAX_K. */
int64_t kmp_lp_resident_cut(
    kmp_lp_t *e, uint32_t k, const int64_t *max_block_weights, int32_t *feasible
);

/* Bytes of partitions, clusterings and mappings copied between host and
 * device so far in this process, by kmp_lp_cluster, kmp_contract,
 * kmp_contract_engine (its downloads of the coarse xadj / vwgt included),
 * kmp_lp_refine, kmp_lp_jet, kmp_lp_rebalance, kmp_lp_set_labels,
 * kmp_lp_get_labels and kmp_lp_project. Counts nothing else (no graph
 * transfers, no k-sized arrays, no isolated-vertex lists); never decreases. */
uint64_t kmp_lp_label_traffic_bytes(void);

/* Download an engine's device-resident CSR into a new host graph handle. */
kmp_graph_t *kmp_lp_download_graph(const kmp_lp_t *e);

uint32_t kmp_lp_n(const kmp_lp_t *e);
uint64_t kmp_lp_m(const kmp_lp_t *e);

/* ------------------------------------------- engines from edge lists
 * An engine built on the device from an unsorted, possibly duplicated,
 * possibly one-directional list of pairs, in host memory or already in HBM.
 * The fine graph never exists on the host (kernels: csrc/edges_hip.hip).
 *
 * Input: num_pairs pairs (src[i], dst[i]) of uint32_t ids (int64_t with
 * KMP_EDGES_IDS64, int32_t with KMP_EDGES_IDS_I32), optional int32_t
 * weights[num_pairs], optional int32_t vwgt[n], and n; n = 0 infers n as the
 * largest id + 1.
 *
 * Output: the canonical CSR of the undirected simple graph.
 *   1. Pairs with src == dst are dropped and counted.
 *   2. Every remaining pair contributes the arcs (u, v, w) and (v, u, w);
 *      whether the input lists one direction or both makes no difference.
 *   3. All arcs with the same (row, col) collapse into one. Without weights
 *      the graph is unweighted (the engine has no adjwgt and the unit-weight
 *      kernels run). With weights the arc weight is the MAXIMUM over the
 *      collapsed arcs, which is idempotent for an input that carries both
 *      directions; with KMP_EDGES_SUM it is the sum (multigraph semantics, as
 *      in contraction), every addition carried out in 64 bits.
 *   4. Rows are sorted by neighbour id, ascending. xadj is 64-bit on the
 *      device as in every engine; vertices without arcs keep empty rows.
 * The result is a pure function of the multiset of input pairs: input order,
 * thread scheduling and the order of atomics cannot show.
 *
 * Errors (NULL, a message on stderr, nothing left allocated): an id >= n
 * where n was given; a negative id or one >= 2^32; a weight <= 0; a sum above
 * 2^31 - 1; n = 0 with no pairs; n = 0 together with vwgt (whose length would
 * have to be the inferred n); 2 * num_pairs >= 2^32 (so that m < 2^32 and
 * every engine feature works on the result); unknown flags. Ids are validated
 * by the kernel that packs the sort keys, which indexes no array by a vertex
 * id, and the host reads the error counters before any kernel that does: a
 * bad id ends the call as an error return, never as an out-of-range access.
 * The input arrays are never modified.
 *
 * Host reads: the error counters, the number of collapsed arcs, the isolated
 * scan; one more, first, when n is inferred (the key width depends on n).
 * Nothing arc-sized is read back. Temporaries: 32 bytes per pair unweighted,
 * 48 weighted (two key and two value buffers of 2 * num_pairs entries), plus
 * rocprim's scratch; a staged host input is freed before the second buffers
 * are allocated, and every temporary before the engine's own buffers.
 *
 * The engine holds no labels afterwards, like one from kmp_lp_create; with
 * vwgt == NULL it has unit node weights. */
#define KMP_EDGES_DEVICE 1u /* src, dst, weights, vwgt are device pointers */
#define KMP_EDGES_IDS64  2u /* src, dst are int64_t; default uint32_t */
#define KMP_EDGES_SUM    4u /* parallel edges add; default: maximum */
#define KMP_EDGES_SORT64 8u /* measurement only: sort all 64 key bits instead
                             * of the 2 * bit_width(n) that carry information;
                             * same result */
#define KMP_EDGES_IDS_I32 16u /* src, dst are int32_t: a negative id is an
                               * error even where n is inferred */
typedef struct kmp_edges_stats_t {
  uint64_t pairs, self_loops, arcs;  /* arcs = m of the engine */
  uint64_t merged_arcs;              /* 2 * (pairs - self_loops) - arcs */
  uint32_t n, isolated, max_degree;
  uint64_t pack_ns, sort_ns, build_ns; /* HIP events; build = collapse + CSR */
  uint64_t total_ns;                 /* wall, device-synced, engine allocation included */
  uint64_t peak_bytes;               /* largest sum of live temporaries */
} kmp_edges_stats_t;
kmp_lp_t *kmp_lp_create_from_edges(uint32_t n, uint64_t num_pairs,
    const void *src, const void *dst, const int32_t *weights,
    const int32_t *vwgt, uint32_t flags, kmp_edges_stats_t *stats);

/* Device-to-device copy of the resident labels (n entries) into dst_device,
 * on the engine's stream, complete on return. -1 if the engine holds none.
 * Does not count towards kmp_lp_label_traffic_bytes. */
int kmp_lp_get_labels_device(const kmp_lp_t *e, uint32_t *dst_device);

/* ------------------------------------------- block subgraph extraction
 * All block-induced subgraphs of a partition, packed into one device memory
 * with per-block start positions: the counterpart of graph::extract_subgraphs
 * (kaminpar-shm/graphutils/subgraph_extractor.cc:335-480). Given labels L (n
 * entries, values < k, 1 <= k <= 2048) on the engine's device CSR:
 *   nodes    all vertex ids ordered by (L[u], u); node_off[b] (k + 1 entries)
 *            is the start of block b in nodes;
 *            mapping[u] = (position of u in nodes) - node_off[L[u]], the rank
 *            of u among its block's vertices in ascending id. The reference
 *            hands this rank out with a racing fetch_add (:395-401); this is
 *            the order a serial run of it produces, and it is deterministic
 *   sub-row  of the vertex at position i, u = nodes[i]: the arcs (u, v) of
 *            u's row with L[v] == L[u], in their original adjacency order,
 *            stored as mapping[v] and the arc's weight. Self-arcs and
 *            parallel arcs are kept as they are
 *   packed   sub_xadj (n + 1, u64) = exclusive prefix sum of the internal
 *            degrees in nodes order; arc_off[b] = sub_xadj[node_off[b]]
 *            (k + 1 entries); sub_adj, sub_adjwgt and sub_vwgt are packed in
 *            the same order. Block b's CSR is the slice
 *            [node_off[b], node_off[b + 1]] of sub_xadj, rebased by
 *            arc_off[b]. Weights are carried only when the engine has them.
 * All arithmetic is integer. Bit-identical to the numpy twin
 * tests/extract_twin.py.
 *
 * The partition is uploaded into scratch owned by the call: the engine's own
 * label state is not touched, and the engine must be idle. */
typedef struct kmp_subgraphs_t kmp_subgraphs_t; /* device-resident packed result */

typedef struct kmp_extract_stats_t {
  uint64_t arcs_scanned; /* arcs read by count + fill (2 * m) */
  uint64_t count_ns;     /* HIP-event time of the count pass */
  uint64_t fill_ns;      /* HIP-event time of the fill pass */
  uint64_t total_ns;     /* wall time of the whole call (device-synced) */
} kmp_extract_stats_t;

/* partition: n entries, values < k. mapping_out: n entries, may be NULL.
 * Returns NULL on error (k not in 1..2048, an engine with m >= 2^32 arcs or a
 * label >= k, reported on stderr); the engine stays usable. */
kmp_subgraphs_t *kmp_lp_extract_subgraphs(
    kmp_lp_t *e,
    uint32_t k,
    const uint32_t *partition,
    uint32_t *mapping_out,
    kmp_extract_stats_t *stats
);
uint32_t kmp_subgraphs_k(const kmp_subgraphs_t *s);
/* nodes_out n, node_off_out k + 1, arc_off_out k + 1 entries; any may be NULL */
int kmp_subgraphs_layout(
    const kmp_subgraphs_t *s,
    uint32_t *nodes_out,
    uint32_t *node_off_out,
    uint64_t *arc_off_out
);
/* Host copy of block b's subgraph; an empty block gives a 0-vertex graph. */
kmp_graph_t *kmp_subgraphs_download(const kmp_subgraphs_t *s, uint32_t b);
/* New engine holding block b's subgraph, copied device-to-device; it outlives
 * the handle and the parent engine. NULL for an empty block. Engines are made
 * one at a time, on demand (each owns a stream). */
kmp_lp_t *kmp_subgraphs_engine(const kmp_subgraphs_t *s, uint32_t b);
void kmp_subgraphs_free(kmp_subgraphs_t *s);

/* ------------------------------------------------- multilevel pipeline */

/* Recursive-bisection initial partitioning on a (small) host graph: greedy
 * graph growing from `reps` distinct high-degree seeds per bisection, each
 * polished by two-way FM with best-prefix rollback, then a gain-aware
 * overload balancer. Restates the reference's initial-partitioning recipe
 * in simplified form (kaminpar-shm/initial_partitioning/). CPU-only. */
int kmp_initial_partition(
    const kmp_graph_t *g,
    uint32_t k,
    int64_t max_block_weight,
    int reps,
    uint32_t *part_out
);

/* Full multilevel partition on the GPU (BASELINE config 3; the shape of
 * KaMinPar::compute_partition, kaminpar.h:970-1025): GPU LP clustering +
 * device-resident contraction per level, CPU initial partitioning on the
 * coarsest graph, GPU LP refinement at every level. Deterministic;
 * bit-identical to the Python driver kaminpar_amd.partition.partition.
 * Returns the final edge cut, or -1 on error. This is kmp_partition_ex (below)
 * with kmp_pipeline_opts_default() and the arguments given here: no Jet, the
 * size rule for the CPU FM, host labels. */
int64_t kmp_partition(
    const kmp_graph_t *g,
    uint32_t k,
    double eps,
    uint64_t seed,
    int iters,
    uint32_t contraction_limit, /* 0 -> default 2000 */
    uint32_t stop_n,            /* 0 -> default 512 */
    int ip_reps,                /* 0 -> default 8 */
    uint32_t *part_out
);

/* Progressive-k extension helper (C twin of partition.py
 * _extend_partition): split block groups in half via FM-polished subset
 * bisections while every block keeps >= split_c vertices (or force != 0).
 * group_lo/group_w are k-sized arrays holding *num_groups entries. */
int kmp_extend_partition(
    const kmp_graph_t *g, uint32_t *part, uint32_t k, int64_t mbw_val,
    uint32_t split_c, int reps, int force, uint32_t *group_lo,
    uint32_t *group_w, uint32_t *num_groups
);

/* Overload balancer (uniform cap) on a host graph, in place. */
int kmp_balance_partition(
    const kmp_graph_t *g, uint32_t k, int64_t cap, uint32_t *part
);

/* Deterministic k-way boundary FM with pass-level best-prefix rollback
 * (serial-deterministic restatement of the reference's k-way FM refiner
 * shape, kaminpar-shm/refinement/fm/fm_refiner.cc). caps[k] are hard
 * per-block weight caps (0 closes a block). 0 -> defaults: max_passes 3,
 * max_fruitless 300. CPU-only; the multilevel drivers run it per level on
 * graphs <= ~2M fine vertices. */
int kmp_kway_fm(
    const kmp_graph_t *g, uint32_t k, const int64_t *caps, uint32_t *part,
    int max_passes, int max_fruitless
);

/* Flat / multilevel FM bisection of a vertex subset (see partition_host.cpp). */
int kmp_bisect_subset(
    const kmp_graph_t *g, const uint32_t *nodes, uint32_t n_sub,
    int64_t target1, int64_t cap1, int64_t cap2, int reps, uint8_t *side_out
);
int kmp_bisect_subset_ml(
    const kmp_graph_t *g, const uint32_t *nodes, uint32_t n_sub,
    int64_t target1, int64_t cap1, int64_t cap2, int reps, uint8_t *side_out
);

/* Progressive-k (deep) multilevel partition: grows k by block bisections
 * during uncoarsening (the shape of the reference's deep multilevel mode,
 * kaminpar-shm/partitioning/deep/deep_multilevel.cc). Bit-identical to the
 * Python driver kaminpar_amd.partition.partition_deep. Better cuts than
 * kmp_partition on every golden case. 0 defaults:
 * contraction_limit 2000, stop_n 512, split_c auto (262144 up to 2M
 * vertices, 2000 beyond), ip_reps 8. split_c >= n selects the full
 * late-split quality mode on heavy-tailed graphs: every split at the
 * finest level (measured at R-MAT scale 23: cut 0.44x the reference's
 * best seed, at minutes of host-side bisection cost -- see DESIGN.md).
 * This is kmp_partition_deep_ex (below) with kmp_pipeline_opts_default() and
 * the arguments given here. */
int64_t kmp_partition_deep(
    const kmp_graph_t *g,
    uint32_t k,
    double eps,
    uint64_t seed,
    int iters,
    uint32_t contraction_limit,
    uint32_t stop_n,
    uint32_t split_c,
    int ip_reps,
    uint32_t *part_out
);

/* ------------------------------------------- pipeline options (the _ex forms)
 * Everything the Python drivers partition() / partition_deep() can switch on,
 * for a caller that binds the C ABI only. Always start from
 * kmp_pipeline_opts_default() and override fields: both structs grow at their
 * end only (as kmp_jet_params_t does). */
typedef struct kmp_pipeline_opts_t {
  int iters;                   /* LP sweeps per level; default 5 */
  uint32_t contraction_limit;  /* 0 -> 2000 */
  uint32_t stop_n;             /* 0 -> 512 */
  uint32_t split_c;            /* deep only; 0 -> auto (see kmp_partition_deep) */
  int ip_reps;                 /* 0 -> 8 */
  int jet;                     /* 0 (default) | 1: kmp_lp_jet after LP, before FM, every level */
  kmp_jet_params_t jet_fine;   /* level 0; default kmp_jet_params_default(0) */
  kmp_jet_params_t jet_coarse; /* levels > 0; default kmp_jet_params_default(1) */
  int fm;                      /* -1 (default): CPU FM on up to 2^21 fine vertices | 0 | 1 */
  int resident;                /* 0 (default) | 1: labels stay on the device between stages */
  kmp_lp_t *engine;            /* NULL (default), or an engine of g for level 0; not freed */
  int vcycles;                 /* 0 (default) .. KMP_PIPELINE_MAX_VCYCLES: V-cycles on the result */
  int sparsify;                /* 0 (default) | 1: sparsify every coarse graph of the bottom-up pass */
  kmp_sparsify_params_t sparsify_params; /* default kmp_sparsify_params_default() */
} kmp_pipeline_opts_t;
kmp_pipeline_opts_t kmp_pipeline_opts_default(void);

/* A chain with more levels than this is cut off with an error (-1, one line on
 * stderr, everything freed). A level is kept only if it shrinks its graph to
 * at most 0.95 of the one before; LP clustering shrinks by a factor of two or
 * more per level in practice, which puts 2^32 vertices above a stop size of
 * 512 at 23 levels. Only a chain that keeps shrinking by a few percent per
 * level (0.95^64 is about 1/27) can reach the bound, and coarsening that slow
 * is better reported than carried on. */
#define KMP_PIPELINE_MAX_LEVELS 64
/* Bound of opts.vcycles and of stats.vcycle_cuts. The gain of a cycle falls
 * off fast; nobody has a use for more. */
#define KMP_PIPELINE_MAX_VCYCLES 16
typedef struct kmp_pipeline_stats_t {
  uint32_t num_levels;
  uint32_t level_sizes[KMP_PIPELINE_MAX_LEVELS]; /* [0] = n; the Python drivers' level list */
  uint64_t jet_iterations, jet_moves, jet_balancer_calls; /* summed over levels */
  uint64_t label_traffic_bytes; /* kmp_lp_label_traffic_bytes() after - before */
  /* host wall time: clustering, contraction, the deep driver's extension step
   * (its graph download included), LP refinement, Jet, CPU FM (its graph
   * download and label copies included), the whole call */
  uint64_t cluster_ns, contract_ns, extend_ns, refine_ns, jet_ns, fm_ns, total_ns;
  /* V-cycles: how many ran, how many were accepted, the cut after each
   * (a rejected cycle repeats the cut before it), and their host wall time,
   * which the phase counters above include phase by phase */
  uint32_t vcycles_run, vcycles_accepted;
  int64_t vcycle_cuts[KMP_PIPELINE_MAX_VCYCLES];
  uint64_t vcycle_ns;
  /* arcs of every level's engine in the bottom-up pass of kmp_partition_ex /
   * kmp_partition_deep_ex ([0] = m, num_levels entries; after sparsification
   * where it ran; kmp_vcycle_ex leaves them 0), how many of the kept levels
   * were sparsified, the arcs that dropped and the HIP-event time of the
   * passes, which contract_ns includes */
  uint64_t level_arcs[KMP_PIPELINE_MAX_LEVELS];
  uint32_t sparsified_levels;
  uint64_t sparsify_arcs_dropped;
  uint64_t sparsify_ns;
} kmp_pipeline_stats_t;

/* sizeof of the two structs as the library was built, and the byte offset of
 * every field in declaration order (offsets_out: cap entries; returns the
 * number of fields). For bindings that mirror the structs by hand. */
uint32_t kmp_pipeline_opts_size(void);
uint32_t kmp_pipeline_stats_size(void);
uint32_t kmp_pipeline_opts_layout(uint32_t *offsets_out, uint32_t cap);
uint32_t kmp_pipeline_stats_layout(uint32_t *offsets_out, uint32_t cap);

/* C twins of kaminpar_amd.partition.partition() / partition_deep() with the
 * same options: same call order, seeds and caps, so partition, cut and level
 * sizes are bit-identical to the Python drivers. opts == NULL means the
 * defaults; stats may be NULL (it is filled on success only).
 *   jet       kmp_lp_jet after the level's LP refinement and before its CPU
 *             FM, with the level's caps (the group caps in the deep driver) and
 *             seed `seed`; jet_fine on level 0, jet_coarse on every other
 *             level. Needs k <= KMP_JET_MAX_K.
 *   fm        overrides the size rule for the per-level CPU FM.
 *   resident  clusterings and mappings never reach the host
 *             (kmp_lp_cluster / kmp_contract_engine with NULL arrays), the
 *             partition is uploaded once on the coarsest engine
 *             (kmp_lp_set_labels), refined in place (NULL-partition
 *             kmp_lp_refine / kmp_lp_jet), projected level to level on the
 *             device (kmp_lp_project) and downloaded once at the end; the CPU
 *             FM and the deep driver's extension step bracket themselves with
 *             kmp_lp_get_labels / kmp_lp_set_labels. Same result as 0, where
 *             the projection is a serial host loop.
 *   engine    used as the level-0 engine instead of a new one (creating it is
 *             the largest fixed cost of a call on a large graph); the caller
 *             keeps ownership, and its label state is overwritten.
 *   vcycles   that many V-cycles (kmp_vcycle_ex below) on the result, with
 *             this call's jet / fm / resident and the level-0 engine reused:
 *             cycle c runs with seed + c on the output of cycle c - 1; with
 *             resident the partition stays on the device between them. The
 *             returned cut and partition are the last cycle's; num_levels and
 *             level_sizes stay those of the bottom-up pass.
 *   sparsify  every contraction of the bottom-up pass is
 *             kmp_contract_engine_sparsified with sparsify_params and seed
 *             seed + level (level 0 contracts g); the sparsified graph is what
 *             the deeper levels are built from. Coarse-level cuts (LP's,
 *             Jet's) then refer to the sparsified graphs; the level-0 cut that
 *             is returned is exact as before. The chains of the V-cycles
 *             (vcycles, kmp_vcycle_ex) and the block bisections of the deep
 *             driver coarsen without it, as the reference's coarsener refuses
 *             communities; a cycle compares true level-0 cuts, so vcycles
 *             together with sparsify is allowed. Multi-GPU and kmp_contract
 *             (the form that downloads a host graph) have no such option.
 * Returns the final edge cut, or -1 on error. Bad options are reported with
 * one line on stderr before any engine is created or any GPU call is made:
 * vcycles outside 0 .. KMP_PIPELINE_MAX_VCYCLES,
 * fm outside {-1, 0, 1}, jet, resident or sparsify outside {0, 1}, sparsify = 1
 * with parameters kmp_sparsify_params_valid refuses, jet = 1 with
 * parameters kmp_lp_jet would refuse or with k > KMP_JET_MAX_K, an engine
 * whose n or m differs from g's. On a later error every engine the driver
 * created is freed, and a caller's engine stays usable. */
int64_t kmp_partition_ex(
    const kmp_graph_t *g,
    uint32_t k,
    double eps,
    uint64_t seed,
    const kmp_pipeline_opts_t *opts,
    uint32_t *part_out,
    kmp_pipeline_stats_t *stats
);
int64_t kmp_partition_deep_ex(
    const kmp_graph_t *g,
    uint32_t k,
    double eps,
    uint64_t seed,
    const kmp_pipeline_opts_t *opts,
    uint32_t *part_out,
    kmp_pipeline_stats_t *stats
);

/* One V-cycle: multilevel refinement of an existing k-way partition of g; the
 * C twin of kaminpar_amd.partition.vcycle(), bit-identical to it.
 *   coarsen    as kmp_partition_ex does (same cluster-weight rule, seeds
 *              seed + level, stop rule), with the level's partition as the
 *              clusterer's communities: no cluster crosses a block boundary,
 *              and the partition is restricted to every coarse level exactly
 *              (same cut, same block weights). There is no initial
 *              partitioning.
 *   uncoarsen  as kmp_partition_ex does, under the caps
 *              kmp_max_block_weight(g, k, eps) for every block: LP refinement,
 *              Jet (opts.jet), CPU FM (opts.fm), projection.
 *   accept     iff the result is feasible and the input was not, or both are
 *              alike in that and the result's cut is not above the input's;
 *              otherwise the input comes back unchanged.
 * part_inout holds the input (n labels < k, checked on the host) and receives
 * the result. part_inout == NULL needs opts->resident = 1 and opts->engine:
 * the input is that engine's resident partition, and the result is left there.
 * With resident = 1 nothing n-sized crosses PCIe but one upload of a host
 * input, one download of an accepted result and the FM's copies
 * (kmp_lp_set_communities_resident, kmp_lp_restrict, kmp_lp_project,
 * kmp_lp_labels_from_communities); with 0 every step takes its host form.
 * The communities of the level-0 engine are cleared on the way out.
 * opts.vcycles, split_c and ip_reps are not used. Options are refused as by
 * kmp_partition_ex. stats (may be NULL): num_levels / level_sizes of the
 * cycle's chain, vcycles_run = 1, vcycles_accepted, vcycle_cuts[0], traffic
 * and phase times. Returns the cut of the returned partition, or -1. */
int64_t kmp_vcycle_ex(
    const kmp_graph_t *g,
    uint32_t k,
    double eps,
    uint64_t seed,
    const kmp_pipeline_opts_t *opts,
    uint32_t *part_inout,
    kmp_pipeline_stats_t *stats
);

/* --------------------------------------------- ckaminpar-shaped C shim
 * Mirrors the reference's public C interface (include/kaminpar-shm/
 * ckaminpar.h:61-132: kaminpar_create / kaminpar_copy_graph /
 * kaminpar_set_k / kaminpar_set_uniform_max_block_weights /
 * kaminpar_compute_partition / kaminpar_free) with the same call order,
 * argument meaning and default types (NodeID/EdgeID u32, weights i32).
 * num_threads is accepted for signature parity; the implementation runs on
 * the GPU. */
typedef struct kaminpar_amd_t kaminpar_amd_t;

kaminpar_amd_t *kaminpar_amd_create(int num_threads);
void kaminpar_amd_free(kaminpar_amd_t *shm);
void kaminpar_amd_reseed(kaminpar_amd_t *shm, int seed);
void kaminpar_amd_copy_graph(
    kaminpar_amd_t *shm,
    uint32_t n,
    const uint32_t *xadj,
    const uint32_t *adjncy,
    const int32_t *vwgt,   /* NULL for unit weights */
    const int32_t *adjwgt  /* NULL for unit weights */
);
void kaminpar_amd_set_k(kaminpar_amd_t *shm, uint32_t k);
void kaminpar_amd_set_uniform_max_block_weights(kaminpar_amd_t *shm, double epsilon);
/* Returns the final edge cut, or -1 on error (missing GPU, no graph). */
void kaminpar_amd_set_absolute_max_block_weights(
    kaminpar_amd_t *shm, const int64_t *weights, uint32_t count); /* kaminpar.h:961 */
void kaminpar_amd_set_uniform_min_block_weights(
    kaminpar_amd_t *shm, double min_epsilon); /* kaminpar.h:965; context.cc:72-80 */
void kaminpar_amd_set_absolute_min_block_weights(
    kaminpar_amd_t *shm, const int64_t *weights, uint32_t count); /* kaminpar.h:966 */
void kaminpar_amd_clear_min_block_weights(kaminpar_amd_t *shm); /* kaminpar.h:968 */

/* Counterpart of kaminpar_create_context_by_preset_name (ckaminpar.h:61),
 * as a setter because the shim has no context object; call it anywhere before
 * kaminpar_amd_compute_partition.
 *   "default"  kmp_partition_deep with its defaults (LP refinement, CPU FM by
 *              the size rule); what a new handle does
 *   "jet"      the reference's Jet preset (Jet rebalanced by its
 *              OverloadBalancer): kmp_partition_deep_ex with jet = 1,
 *              balancer = KMP_JET_BALANCER_SELECT in jet_fine and jet_coarse,
 *              fm = -1 and resident = 1. Needs k <= KMP_JET_MAX_K:
 *              kaminpar_amd_compute_partition returns -1 above, it does not
 *              fall back.
 * Returns 0, or -1 for an unknown or NULL name, which leaves the current
 * preset in force. */
int kaminpar_amd_set_preset(kaminpar_amd_t *shm, const char *name);

/* V-cycles after the preset's pipeline (kmp_pipeline_opts_t.vcycles; 0, the
 * default of every preset, runs none). An n the driver refuses makes
 * kaminpar_amd_compute_partition return -1. */
void kaminpar_amd_set_vcycles(kaminpar_amd_t *shm, int n);

/* Threshold edge sparsification of the coarse graphs
 * (kmp_pipeline_opts_t.sparsify / sparsify_params; off in every preset).
 * on: 0 | 1; params == NULL means kmp_sparsify_params_default(). Values the
 * driver refuses make kaminpar_amd_compute_partition return -1. */
void kaminpar_amd_set_sparsification(
    kaminpar_amd_t *shm, int on, const kmp_sparsify_params_t *params);

/* Runs the preset's pipeline, then the absolute-max and min-weight post-steps
 * where such weights are set. Returns the final edge cut, or -1 on error. */
int64_t kaminpar_amd_compute_partition(kaminpar_amd_t *shm, uint32_t *partition);

#ifdef __cplusplus
}
#endif
