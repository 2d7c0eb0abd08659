"""kaminpar_amd: MI355X-native KaMinPar label-propagation hot path.

ctypes bindings over libkaminpar_lp.so (C ABI: include/kaminpar_lp.h).
Host-side graph handling works everywhere; the LP engine requires a GPU and
fails loudly if the HIP device or the native library is missing -- there is
no CPU fallback on the product path (the CPU oracle under oracle/ is test
infrastructure only).

Interop note: PyTorch wheels bundle their own HIP runtime; this module
preloads it (when torch is installed) before loading the native library so
the whole process shares one runtime regardless of import/initialization
order.
"""

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libkaminpar_lp.so")


class JetParams(ctypes.Structure):
    """kmp_jet_params_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("num_rounds", ctypes.c_int),
        ("max_iterations", ctypes.c_int),
        ("max_fruitless", ctypes.c_int),
        ("fruitless_threshold", ctypes.c_double),
        ("initial_gain_temp", ctypes.c_double),
        ("final_gain_temp", ctypes.c_double),
        ("balance_iters", ctypes.c_int),
        ("balancer", ctypes.c_int),
        ("balance_passes", ctypes.c_int),
    ]


KMP_LP_MAX_K = 1 << 24  # largest k of LpEngine.refine / balance (kaminpar_lp.h)

# kmp_jet_params_t.balancer: Jet's rebalance step
JET_BALANCER_LP = 0      # balance_iters sweeps of the LP balancer mode
JET_BALANCER_SELECT = 1  # balance_passes passes of LpEngine.rebalance


class RebalanceStats(ctypes.Structure):
    """kmp_rebalance_stats_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("passes", ctypes.c_uint64),
        ("selected", ctypes.c_uint64),
        ("moves", ctypes.c_uint64),
        ("arcs_scanned", ctypes.c_uint64),
        ("score_ns", ctypes.c_uint64),
        ("total_ns", ctypes.c_uint64),
        ("edge_cut", ctypes.c_int64),
        ("feasible", ctypes.c_int32),
    ]


class ExtractStats(ctypes.Structure):
    """kmp_extract_stats_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("arcs_scanned", ctypes.c_uint64),
        ("count_ns", ctypes.c_uint64),
        ("fill_ns", ctypes.c_uint64),
        ("total_ns", ctypes.c_uint64),
    ]


class JetStats(ctypes.Structure):
    """kmp_jet_stats_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("iterations", ctypes.c_uint64),
        ("balancer_calls", ctypes.c_uint64),
        ("jet_moves", ctypes.c_uint64),
        ("balancer_moves", ctypes.c_uint64),
        ("arcs_scanned", ctypes.c_uint64),
        ("find_filter_ns", ctypes.c_uint64),
        ("total_ns", ctypes.c_uint64),
        ("edge_cut", ctypes.c_int64),
        ("balancer_ns", ctypes.c_uint64),
        ("balancer_passes", ctypes.c_uint64),
        ("feasible_iterations", ctypes.c_uint64),
    ]


class SparsifyParams(ctypes.Structure):
    """kmp_sparsify_params_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("density_target_factor", ctypes.c_double),
        ("edge_target_factor", ctypes.c_double),
        ("laziness_factor", ctypes.c_double),
    ]


class SparsifyStats(ctypes.Structure):
    """kmp_sparsify_stats_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("applied", ctypes.c_uint64),
        ("m_before", ctypes.c_uint64),
        ("m_after", ctypes.c_uint64),
        ("target", ctypes.c_uint64),
        ("threshold", ctypes.c_uint64),
        ("larger", ctypes.c_uint64),
        ("equal", ctypes.c_uint64),
        ("include", ctypes.c_uint64),
        ("pass_ns", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


KMP_PIPELINE_MAX_LEVELS = 64
KMP_PIPELINE_MAX_VCYCLES = 16


class EdgesStats(ctypes.Structure):
    """Mirror of kmp_edges_stats_t (LpEngine.from_edges)."""

    _fields_ = [
        ("pairs", ctypes.c_uint64),
        ("self_loops", ctypes.c_uint64),
        ("arcs", ctypes.c_uint64),
        ("merged_arcs", ctypes.c_uint64),
        ("n", ctypes.c_uint32),
        ("isolated", ctypes.c_uint32),
        ("max_degree", ctypes.c_uint32),
        ("pack_ns", ctypes.c_uint64),
        ("sort_ns", ctypes.c_uint64),
        ("build_ns", ctypes.c_uint64),
        ("total_ns", ctypes.c_uint64),
        ("peak_bytes", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


# flags of kmp_lp_create_from_edges (include/kaminpar_lp.h)
EDGES_DEVICE = 1
EDGES_IDS64 = 2
EDGES_SUM = 4
EDGES_SORT64 = 8
EDGES_IDS_I32 = 16


class PipelineOpts(ctypes.Structure):
    """kmp_pipeline_opts_t (include/kaminpar_lp.h). Start from
    kmp_pipeline_opts_default(); `engine` is a kmp_lp_t * (LpEngine._h)."""

    _fields_ = [
        ("iters", ctypes.c_int),
        ("contraction_limit", ctypes.c_uint32),
        ("stop_n", ctypes.c_uint32),
        ("split_c", ctypes.c_uint32),
        ("ip_reps", ctypes.c_int),
        ("jet", ctypes.c_int),
        ("jet_fine", JetParams),
        ("jet_coarse", JetParams),
        ("fm", ctypes.c_int),
        ("resident", ctypes.c_int),
        ("engine", ctypes.c_void_p),
        ("vcycles", ctypes.c_int),
        ("sparsify", ctypes.c_int),
        ("sparsify_params", SparsifyParams),
    ]


class PipelineStats(ctypes.Structure):
    """kmp_pipeline_stats_t (include/kaminpar_lp.h)."""

    _fields_ = [
        ("num_levels", ctypes.c_uint32),
        ("level_sizes", ctypes.c_uint32 * KMP_PIPELINE_MAX_LEVELS),
        ("jet_iterations", ctypes.c_uint64),
        ("jet_moves", ctypes.c_uint64),
        ("jet_balancer_calls", ctypes.c_uint64),
        ("label_traffic_bytes", ctypes.c_uint64),
        ("cluster_ns", ctypes.c_uint64),
        ("contract_ns", ctypes.c_uint64),
        ("extend_ns", ctypes.c_uint64),
        ("refine_ns", ctypes.c_uint64),
        ("jet_ns", ctypes.c_uint64),
        ("fm_ns", ctypes.c_uint64),
        ("total_ns", ctypes.c_uint64),
        ("vcycles_run", ctypes.c_uint32),
        ("vcycles_accepted", ctypes.c_uint32),
        ("vcycle_cuts", ctypes.c_int64 * KMP_PIPELINE_MAX_VCYCLES),
        ("vcycle_ns", ctypes.c_uint64),
        ("level_arcs", ctypes.c_uint64 * KMP_PIPELINE_MAX_LEVELS),
        ("sparsified_levels", ctypes.c_uint32),
        ("sparsify_arcs_dropped", ctypes.c_uint64),
        ("sparsify_ns", ctypes.c_uint64),
    ]

    @property
    def levels(self):
        """Level sizes as a list, [0] = n (the Python drivers' third value)."""
        return [int(s) for s in self.level_sizes[:self.num_levels]]

    @property
    def arcs(self):
        """Arcs of every level's engine as a list, [0] = m."""
        return [int(a) for a in self.level_arcs[:self.num_levels]]

    @property
    def cycle_cuts(self):
        """The cut after every V-cycle that ran, as a list."""
        return [int(c) for c in self.vcycle_cuts[:self.vcycles_run]]


def sparsify_on(sparsify):
    """The one reading of the drivers' `sparsify` keyword: None and False
    switch the pass off; True, a dict of overrides (an empty one included:
    the defaults) or a SparsifyParams switch it on."""
    return sparsify is not None and sparsify is not False


def sparsify_params(overrides=None):
    """kmp_sparsify_params_default() with a dict of overrides applied; True,
    None or an empty dict gives the defaults (0.5 / 0.5 / 4). An existing
    SparsifyParams is passed through."""
    if isinstance(overrides, SparsifyParams):
        return overrides
    params = _lib.kmp_sparsify_params_default()
    if isinstance(overrides, dict):
        for name, value in overrides.items():
            if name not in ("density_target_factor", "edge_target_factor",
                            "laziness_factor"):
                raise ValueError(f"sparsify: unknown parameter {name!r}")
            setattr(params, name, float(value))
    elif overrides not in (None, True):
        raise ValueError("sparsify: expected True or a dict of overrides")
    return params


def sparsify_params_valid(params):
    """kmp_sparsify_params_valid: every factor finite and > 0, laziness >= 1."""
    return bool(_lib.kmp_sparsify_params_valid(ctypes.byref(sparsify_params(params))))


def _preload_torch_hip_runtime():
    """Bind everything to ONE HIP runtime.

    PyTorch wheels bundle their own libamdhip64 and load it via absolute
    RPATH paths, ignoring an already-loaded system copy -- two HSA clients in
    one process leave whichever initializes second unable to see the GPU.
    Preloading torch's copy under its SONAME makes this library resolve to
    it, and torch's later absolute-path load maps the same file. Without
    torch installed this is a no-op and the system runtime is used.
    """
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass  # fall back to the system runtime


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"kaminpar_amd: native library not found at {_LIB_PATH}; "
            "build it with __graft_entry__.build() or kaminpar_amd/csrc/build.sh"
        )
    _preload_torch_hip_runtime()
    lib = ctypes.CDLL(_LIB_PATH)

    u32, u64, i32, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64
    p = ctypes.POINTER
    vp = ctypes.c_void_p

    lib.kmp_graph_from_csr.restype = vp
    lib.kmp_graph_from_csr.argtypes = [u32, u64, p(u32), p(u32), p(i32), p(i32)]
    lib.kmp_graph_from_csr64.restype = vp
    lib.kmp_graph_from_csr64.argtypes = [u32, u64, p(u64), p(u32), p(i32), p(i32)]
    lib.kmp_gen_rmat.restype = vp
    lib.kmp_gen_rmat.argtypes = [ctypes.c_int, ctypes.c_int, u64]
    lib.kmp_gen_rgg2d.restype = vp
    lib.kmp_gen_rgg2d.argtypes = [u32, ctypes.c_double, u64]
    lib.kmp_read_metis.restype = vp
    lib.kmp_read_metis.argtypes = [ctypes.c_char_p]
    lib.kmp_write_metis.restype = ctypes.c_int
    lib.kmp_write_metis.argtypes = [vp, ctypes.c_char_p]
    lib.kmp_read_parhip.restype = vp
    lib.kmp_read_parhip.argtypes = [ctypes.c_char_p]
    lib.kmp_write_parhip.restype = ctypes.c_int
    lib.kmp_write_parhip.argtypes = [vp, ctypes.c_char_p]
    lib.kmp_graph_n.restype = u32
    lib.kmp_graph_n.argtypes = [vp]
    lib.kmp_graph_m.restype = u64
    lib.kmp_graph_m.argtypes = [vp]
    lib.kmp_graph_xadj.restype = p(u32)
    lib.kmp_graph_xadj.argtypes = [vp]
    lib.kmp_graph_xadj64.restype = p(u64)
    lib.kmp_graph_xadj64.argtypes = [vp]
    lib.kmp_graph_adjncy.restype = p(u32)
    lib.kmp_graph_adjncy.argtypes = [vp]
    lib.kmp_graph_vwgt.restype = p(i32)
    lib.kmp_graph_vwgt.argtypes = [vp]
    lib.kmp_graph_adjwgt.restype = p(i32)
    lib.kmp_graph_adjwgt.argtypes = [vp]
    lib.kmp_graph_total_node_weight.restype = i64
    lib.kmp_graph_total_node_weight.argtypes = [vp]
    lib.kmp_graph_free.argtypes = [vp]
    lib.kmp_edge_cut_host.restype = i64
    lib.kmp_edge_cut_host.argtypes = [vp, p(u32)]
    lib.kmp_max_block_weight.restype = i64
    lib.kmp_max_block_weight.argtypes = [vp, u32, ctypes.c_double]
    lib.kmp_rearrange_degree_buckets.restype = vp
    lib.kmp_rearrange_degree_buckets.argtypes = [vp, p(u32)]
    lib.kmp_initial_partition.restype = ctypes.c_int
    lib.kmp_initial_partition.argtypes = [vp, u32, i64, ctypes.c_int, p(u32)]
    lib.kmp_balance_partition.restype = ctypes.c_int
    lib.kmp_balance_partition.argtypes = [vp, u32, i64, p(u32)]
    lib.kmp_kway_fm.restype = ctypes.c_int
    lib.kmp_kway_fm.argtypes = [vp, u32, p(i64), p(u32),
                                ctypes.c_int, ctypes.c_int]
    lib.kmp_bisect_subset.restype = ctypes.c_int
    lib.kmp_bisect_subset.argtypes = [vp, p(u32), u32, i64, i64, i64,
                                      ctypes.c_int, p(ctypes.c_uint8)]
    lib.kmp_bisect_subset_ml.restype = ctypes.c_int
    lib.kmp_bisect_subset_ml.argtypes = [vp, p(u32), u32, i64, i64, i64,
                                         ctypes.c_int, p(ctypes.c_uint8)]
    lib.kmp_bisect_subset_fast.restype = ctypes.c_int
    lib.kmp_bisect_subset_fast.argtypes = [vp, p(u32), u32, i64, i64, i64,
                                           ctypes.c_int, p(ctypes.c_uint8)]
    lib.kmp_partition.restype = i64
    lib.kmp_partition.argtypes = [vp, u32, ctypes.c_double, u64, ctypes.c_int,
                                  u32, u32, ctypes.c_int, p(u32)]
    lib.kmp_partition_deep.restype = i64
    lib.kmp_partition_deep.argtypes = [vp, u32, ctypes.c_double, u64,
                                       ctypes.c_int, u32, u32, u32,
                                       ctypes.c_int, p(u32)]
    lib.kmp_pipeline_opts_default.restype = PipelineOpts
    lib.kmp_pipeline_opts_default.argtypes = []
    for fn in (lib.kmp_pipeline_opts_size, lib.kmp_pipeline_stats_size):
        fn.restype = u32
        fn.argtypes = []
    for fn in (lib.kmp_pipeline_opts_layout, lib.kmp_pipeline_stats_layout):
        fn.restype = u32
        fn.argtypes = [p(u32), u32]
    for fn in (lib.kmp_partition_ex, lib.kmp_partition_deep_ex, lib.kmp_vcycle_ex):
        fn.restype = i64
        fn.argtypes = [vp, u32, ctypes.c_double, u64, p(PipelineOpts), p(u32),
                       p(PipelineStats)]
    lib.kmp_jet_params_valid.restype = ctypes.c_int
    lib.kmp_jet_params_valid.argtypes = [p(JetParams)]

    # ckaminpar-shaped shim
    lib.kaminpar_amd_create.restype = vp
    lib.kaminpar_amd_create.argtypes = [ctypes.c_int]
    lib.kaminpar_amd_free.restype = None
    lib.kaminpar_amd_free.argtypes = [vp]
    lib.kaminpar_amd_reseed.restype = None
    lib.kaminpar_amd_reseed.argtypes = [vp, ctypes.c_int]
    lib.kaminpar_amd_copy_graph.restype = None
    lib.kaminpar_amd_copy_graph.argtypes = [vp, u32, p(u32), p(u32), p(i32), p(i32)]
    lib.kaminpar_amd_set_k.restype = None
    lib.kaminpar_amd_set_k.argtypes = [vp, u32]
    lib.kaminpar_amd_set_uniform_max_block_weights.restype = None
    lib.kaminpar_amd_set_uniform_max_block_weights.argtypes = [vp, ctypes.c_double]
    lib.kaminpar_amd_set_preset.restype = ctypes.c_int
    lib.kaminpar_amd_set_preset.argtypes = [vp, ctypes.c_char_p]
    lib.kaminpar_amd_set_vcycles.restype = None
    lib.kaminpar_amd_set_vcycles.argtypes = [vp, ctypes.c_int]
    lib.kaminpar_amd_set_sparsification.restype = None
    lib.kaminpar_amd_set_sparsification.argtypes = [
        vp, ctypes.c_int, ctypes.POINTER(SparsifyParams)]
    lib.kaminpar_amd_compute_partition.restype = i64
    lib.kaminpar_amd_compute_partition.argtypes = [vp, p(u32)]

    lib.kmp_lp_create.restype = vp
    lib.kmp_lp_create.argtypes = [vp]
    lib.kmp_lp_free.argtypes = [vp]
    lib.kmp_lp_refine.restype = i64
    lib.kmp_lp_refine.argtypes = [vp, u32, p(i64), p(u32), u64, ctypes.c_int, vp]
    lib.kmp_lp_balance.restype = i64
    lib.kmp_lp_balance.argtypes = [vp, u32, p(i64), p(u32), u64, ctypes.c_int, vp]
    lib.kmp_lp_balance_host_ns.restype = None
    lib.kmp_lp_balance_host_ns.argtypes = [vp, p(ctypes.c_uint64)]
    lib.kmp_jet_params_default.restype = JetParams
    lib.kmp_jet_params_default.argtypes = [ctypes.c_int]
    lib.kmp_lp_jet.restype = i64
    lib.kmp_lp_jet.argtypes = [vp, u32, p(i64), p(u32), u64, vp, vp]
    lib.kmp_lp_rebalance.restype = i64
    lib.kmp_lp_rebalance.argtypes = [vp, u32, p(i64), p(u32), ctypes.c_int, vp]
    lib.kmp_lp_set_communities.restype = ctypes.c_int
    lib.kmp_lp_set_communities.argtypes = [vp, p(u32)]
    lib.kmp_lp_rearrange_degree_buckets.restype = ctypes.c_int
    lib.kmp_lp_rearrange_degree_buckets.argtypes = [vp, p(u32)]
    lib.kmp_lp_underload.restype = i64
    lib.kmp_lp_underload.argtypes = [vp, u32, p(i64), p(i64), p(u32), u64,
                                     ctypes.c_int, vp]
    lib.kmp_lp_cluster.restype = i64
    lib.kmp_lp_cluster.argtypes = [vp, i64, u32, p(u32), u64, ctypes.c_int, vp]
    lib.kmp_lp_num_chunks.restype = u32
    lib.kmp_lp_num_chunks.argtypes = [vp]
    lib.kmp_lp_refine_begin.restype = ctypes.c_int
    lib.kmp_lp_refine_begin.argtypes = [vp, u32, p(i64), p(u32), u64]
    lib.kmp_lp_phase_a.restype = i64
    lib.kmp_lp_phase_a.argtypes = [vp, ctypes.c_int, u32, u32, u32, vp, u32]
    lib.kmp_lp_commit.restype = i64
    lib.kmp_lp_commit.argtypes = [vp, ctypes.c_int, u32, vp, u32]
    lib.kmp_nccl_unique_id.restype = ctypes.c_int
    lib.kmp_nccl_unique_id.argtypes = [vp]
    lib.kmp_nccl_comm_init.restype = vp
    lib.kmp_nccl_comm_init.argtypes = [ctypes.c_int, ctypes.c_int, vp]
    lib.kmp_nccl_comm_destroy.restype = None
    lib.kmp_nccl_comm_destroy.argtypes = [vp]
    lib.kmp_lp_refine_dist.restype = i64
    lib.kmp_lp_refine_dist.argtypes = [vp, u32, p(i64), p(u32), u64,
                                       ctypes.c_int, vp, ctypes.c_int,
                                       ctypes.c_int, vp]
    lib.kmp_lp_set_stream.restype = ctypes.c_int
    lib.kmp_lp_set_stream.argtypes = [vp, vp]
    lib.kmp_lp_shard_begin.restype = ctypes.c_int
    lib.kmp_lp_shard_begin.argtypes = [vp, u32, u32, vp, u32, vp]
    lib.kmp_lp_shard_round.restype = ctypes.c_int
    lib.kmp_lp_shard_round.argtypes = [vp, u32, u32, vp, vp]
    lib.kmp_lp_shard_finish_meta.restype = ctypes.c_int
    lib.kmp_lp_shard_finish_meta.argtypes = [vp, u32, u32, vp, vp]
    lib.kmp_lp_shard_apply.restype = i64
    lib.kmp_lp_shard_apply.argtypes = [vp, ctypes.c_int, u32, vp, u32, vp, vp, vp]
    lib.kmp_lp_refine_end.restype = i64
    lib.kmp_lp_refine_end.argtypes = [vp, p(u32), vp]
    lib.kmp_lp_reset.restype = ctypes.c_int
    lib.kmp_lp_reset.argtypes = [vp]
    lib.kmp_lp_run_sweeps.restype = i64
    lib.kmp_lp_run_sweeps.argtypes = [vp, ctypes.c_int]
    lib.kmp_lp_get_stats.restype = ctypes.c_int
    lib.kmp_lp_get_stats.argtypes = [vp, vp]
    lib.kmp_contract.restype = i64
    lib.kmp_contract.argtypes = [vp, p(u32), p(u32), ctypes.POINTER(vp)]
    lib.kmp_contract_engine.restype = i64
    lib.kmp_contract_engine.argtypes = [vp, p(u32), p(u32), ctypes.POINTER(vp)]
    lib.kmp_sparsify_params_default.restype = SparsifyParams
    lib.kmp_sparsify_params_default.argtypes = []
    lib.kmp_sparsify_params_valid.restype = ctypes.c_int
    lib.kmp_sparsify_params_valid.argtypes = [ctypes.POINTER(SparsifyParams)]
    lib.kmp_contract_engine_sparsified.restype = i64
    lib.kmp_contract_engine_sparsified.argtypes = [
        vp, p(u32), p(u32), ctypes.POINTER(SparsifyParams), ctypes.c_uint64,
        ctypes.POINTER(vp), ctypes.POINTER(SparsifyStats)]
    lib.kmp_lp_set_labels.restype = ctypes.c_int
    lib.kmp_lp_set_labels.argtypes = [vp, u32, p(u32)]
    lib.kmp_lp_get_labels.restype = ctypes.c_int
    lib.kmp_lp_get_labels.argtypes = [vp, p(u32)]
    lib.kmp_lp_project.restype = ctypes.c_int
    lib.kmp_lp_project.argtypes = [vp, vp]
    lib.kmp_lp_set_communities_resident.restype = ctypes.c_int
    lib.kmp_lp_set_communities_resident.argtypes = [vp]
    lib.kmp_lp_restrict.restype = ctypes.c_int
    lib.kmp_lp_restrict.argtypes = [vp, vp]
    lib.kmp_lp_labels_from_communities.restype = ctypes.c_int
    lib.kmp_lp_labels_from_communities.argtypes = [vp]
    lib.kmp_lp_resident_cut.restype = i64
    lib.kmp_lp_resident_cut.argtypes = [vp, u32, p(i64), p(ctypes.c_int32)]
    lib.kmp_lp_label_traffic_bytes.restype = ctypes.c_uint64
    lib.kmp_lp_label_traffic_bytes.argtypes = []
    lib.kmp_lp_download_graph.restype = vp
    lib.kmp_lp_download_graph.argtypes = [vp]
    lib.kmp_lp_extract_subgraphs.restype = vp
    lib.kmp_lp_extract_subgraphs.argtypes = [vp, u32, p(u32), p(u32), vp]
    lib.kmp_subgraphs_k.restype = u32
    lib.kmp_subgraphs_k.argtypes = [vp]
    lib.kmp_subgraphs_layout.restype = ctypes.c_int
    lib.kmp_subgraphs_layout.argtypes = [vp, p(u32), p(u32), p(u64)]
    lib.kmp_subgraphs_download.restype = vp
    lib.kmp_subgraphs_download.argtypes = [vp, u32]
    lib.kmp_subgraphs_engine.restype = vp
    lib.kmp_subgraphs_engine.argtypes = [vp, u32]
    lib.kmp_subgraphs_free.restype = None
    lib.kmp_subgraphs_free.argtypes = [vp]
    lib.kmp_lp_n.restype = u32
    lib.kmp_lp_n.argtypes = [vp]
    lib.kmp_lp_m.restype = ctypes.c_uint64
    lib.kmp_lp_m.argtypes = [vp]
    lib.kmp_lp_create_from_edges.restype = vp
    lib.kmp_lp_create_from_edges.argtypes = [
        u32, u64, vp, vp, vp, vp, u32, ctypes.POINTER(EdgesStats)]
    lib.kmp_lp_get_labels_device.restype = ctypes.c_int
    lib.kmp_lp_get_labels_device.argtypes = [vp, vp]
    return lib


_lib = _load()


class Stats(ctypes.Structure):
    _fields_ = [
        ("arcs_scanned", ctypes.c_uint64),
        ("moves", ctypes.c_uint64),
        ("phase_a_ns", ctypes.c_uint64),
        ("total_ns", ctypes.c_uint64),
        ("num_clusters", ctypes.c_uint64),
        ("edge_cut", ctypes.c_int64),
    ]


def _u32p(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _i64p(a):
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def label_traffic_bytes():
    """Bytes of partitions, clusterings and mappings copied between host and
    device so far in this process (kmp_lp_label_traffic_bytes)."""
    return int(_lib.kmp_lp_label_traffic_bytes())


def pipeline_opts(iters=5, jet=False, fm=None, resident=False, engine=None,
                  contraction_limit=0, stop_n=0, split_c=0, vcycles=0,
                  sparsify=False):
    """kmp_pipeline_opts_default() with the keywords of
    kaminpar_amd.partition.partition() / partition_deep() applied: `jet` is
    False, True or a dict of kmp_jet_params_t overrides applied to jet_fine
    and jet_coarse alike (an unknown key raises TypeError, as LpEngine.jet
    does); `fm` None keeps the size rule; `engine` is an LpEngine, which the
    caller keeps alive over the call; `sparsify` is False, True or a dict of
    kmp_sparsify_params_t overrides (sparsify_params())."""
    opts = _lib.kmp_pipeline_opts_default()
    opts.iters = int(iters)
    opts.contraction_limit = int(contraction_limit)
    opts.stop_n = int(stop_n)
    opts.split_c = int(split_c)
    opts.jet = 1 if jet else 0
    if isinstance(jet, dict):
        names = {f[0] for f in JetParams._fields_}
        for key, val in jet.items():
            if key not in names:
                raise TypeError(f"jet got an unknown parameter {key!r}")
            setattr(opts.jet_fine, key, val)
            setattr(opts.jet_coarse, key, val)
    opts.fm = -1 if fm is None else int(bool(fm))
    opts.resident = 1 if resident else 0
    opts.engine = None if engine is None else engine._h
    opts.vcycles = int(vcycles)
    opts.sparsify = 1 if sparsify_on(sparsify) else 0
    if sparsify_on(sparsify):
        opts.sparsify_params = sparsify_params(sparsify)
    return opts


class Graph:
    """Host CSR graph in the reference layout (csr_graph.h:27-33)."""

    def __init__(self, handle):
        if not handle:
            raise ValueError("graph construction failed")
        self._h = handle

    @classmethod
    def from_csr(cls, xadj, adjncy, vwgt=None, adjwgt=None):
        adjncy = np.ascontiguousarray(adjncy, dtype=np.uint32)
        n = len(xadj) - 1
        m = len(adjncy)
        vp = None
        ap = None
        if vwgt is not None:
            vwgt = np.ascontiguousarray(vwgt, dtype=np.int32)
            vp = vwgt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if adjwgt is not None:
            adjwgt = np.ascontiguousarray(adjwgt, dtype=np.int32)
            ap = adjwgt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if m >= (1 << 32):
            # EdgeID-64 path (device offsets are 64-bit either way)
            xadj = np.ascontiguousarray(xadj, dtype=np.uint64)
            xp = xadj.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            return cls(_lib.kmp_graph_from_csr64(n, m, xp, _u32p(adjncy), vp, ap))
        xadj = np.ascontiguousarray(xadj, dtype=np.uint32)
        return cls(_lib.kmp_graph_from_csr(n, m, _u32p(xadj), _u32p(adjncy), vp, ap))

    @classmethod
    def rmat(cls, scale, edgefactor=8, seed=42):
        return cls(_lib.kmp_gen_rmat(scale, edgefactor, seed))

    @classmethod
    def rgg2d(cls, n, avg_deg=16.0, seed=42):
        return cls(_lib.kmp_gen_rgg2d(n, avg_deg, seed))

    @classmethod
    def read_metis(cls, path):
        return cls(_lib.kmp_read_metis(os.fsencode(path)))

    @classmethod
    def read_parhip(cls, path):
        return cls(_lib.kmp_read_parhip(os.fsencode(path)))

    def write_metis(self, path):
        if _lib.kmp_write_metis(self._h, os.fsencode(path)) != 0:
            raise IOError(f"cannot write {path}")

    def write_parhip(self, path):
        if _lib.kmp_write_parhip(self._h, os.fsencode(path)) != 0:
            raise IOError(f"cannot write {path}")

    @property
    def n(self):
        return _lib.kmp_graph_n(self._h)

    @property
    def m(self):
        return _lib.kmp_graph_m(self._h)

    @property
    def xadj(self):
        p = _lib.kmp_graph_xadj(self._h)
        if not p:
            # 64-bit-offset graph (m >= 2^32): expose the wide offsets
            p64 = _lib.kmp_graph_xadj64(self._h)
            return np.ctypeslib.as_array(p64, shape=(self.n + 1,))
        return np.ctypeslib.as_array(p, shape=(self.n + 1,))

    @property
    def adjncy(self):
        if self.m == 0:
            return np.zeros(0, dtype=np.uint32)  # null data ptr on empty CSR
        return np.ctypeslib.as_array(_lib.kmp_graph_adjncy(self._h), shape=(self.m,))

    @property
    def vwgt(self):
        """Node weights (int32 view), or None on a unit-weight graph."""
        p = _lib.kmp_graph_vwgt(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(self.n,))

    @property
    def adjwgt(self):
        """Arc weights (int32 view), or None on a unit-weight graph."""
        p = _lib.kmp_graph_adjwgt(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(self.m,))

    @property
    def total_node_weight(self):
        return _lib.kmp_graph_total_node_weight(self._h)

    def edge_cut(self, labels):
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        return _lib.kmp_edge_cut_host(self._h, _u32p(labels))

    def max_block_weight(self, k, eps=0.03):
        return _lib.kmp_max_block_weight(self._h, k, eps)

    def _partition_ex(self, fn, name, k, eps, seed, iters, jet, fm, resident,
                      engine, contraction_limit, stop_n, split_c, return_stats,
                      vcycles=0, sparsify=False):
        """Shared body of partition_native / partition_deep_native: fill a
        kmp_pipeline_opts_t from the keywords and call the _ex driver."""
        opts = pipeline_opts(iters=iters, jet=jet, fm=fm, resident=resident,
                             engine=engine, contraction_limit=contraction_limit,
                             stop_n=stop_n, split_c=split_c, vcycles=vcycles,
                             sparsify=sparsify)
        part = np.zeros(self.n, dtype=np.uint32)
        stats = PipelineStats()
        cut = fn(self._h, k, eps, seed, ctypes.byref(opts), _u32p(part),
                 ctypes.byref(stats))
        if cut < 0:
            raise RuntimeError(f"{name} failed")
        return (cut, part, stats) if return_stats else (cut, part)

    def partition_native(self, k, eps=0.03, seed=1, iters=5, jet=False,
                         fm=None, resident=False, engine=None,
                         contraction_limit=0, stop_n=0, return_stats=False,
                         vcycles=0, sparsify=False):
        """Full multilevel partition driven entirely from the C ABI
        (kmp_partition_ex; the shape of KaMinPar::compute_partition).
        Bit-identical to kaminpar_amd.partition.partition with the same
        keywords: `jet` (True, or a dict of kmp_jet_params_t overrides applied
        to the fine and the coarse parameter set), `fm`, `resident`, `engine`
        (an LpEngine of this graph, reused as the level-0 engine),
        `contraction_limit` and `stop_n` (0 = default), `sparsify` (False,
        True or a dict of kmp_sparsify_params_t overrides). Requires a GPU.

        Returns (cut, partition); with return_stats also a PipelineStats."""
        return self._partition_ex(
            _lib.kmp_partition_ex, "kmp_partition_ex", k, eps, seed, iters,
            jet, fm, resident, engine, contraction_limit, stop_n, 0,
            return_stats, vcycles, sparsify)

    def balance_partition(self, k, cap, part):
        """Gain-aware overload balancer (uniform cap), in place."""
        part = np.ascontiguousarray(part, dtype=np.uint32)
        _lib.kmp_balance_partition(self._h, k, int(cap), _u32p(part))
        return part

    def kway_fm(self, k, caps, part, max_passes=0, max_fruitless=0):
        """Deterministic k-way boundary FM (best-prefix rollback), in
        place; caps is a k-length per-block hard cap array (0 closes a
        block)."""
        caps = np.ascontiguousarray(caps, dtype=np.int64)
        part = np.ascontiguousarray(part, dtype=np.uint32)
        _lib.kmp_kway_fm(self._h, k,
                         caps.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                         _u32p(part), max_passes, max_fruitless)
        return part

    def bisect_subset(self, nodes, target1, cap1, cap2, reps=8):
        """Bisect an arbitrary vertex subset (greedy grow + FM, best of
        reps). Returns a boolean side array aligned with `nodes`."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        side = np.zeros(len(nodes), dtype=np.uint8)
        rc = _lib.kmp_bisect_subset(
            self._h, _u32p(nodes), len(nodes), int(target1), int(cap1),
            int(cap2), reps, side.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        if rc != 0:
            raise RuntimeError("kmp_bisect_subset failed")
        return side.astype(bool)

    def bisect_subset_fast(self, nodes, target1, cap1, cap2, reps=8):
        """O(m log n) bisection (lazy-PQ greedy grow + FM); for subgraphs
        beyond a few thousand vertices."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        side = np.zeros(len(nodes), dtype=np.uint8)
        rc = _lib.kmp_bisect_subset_fast(
            self._h, _u32p(nodes), len(nodes), int(target1), int(cap1),
            int(cap2), reps, side.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        if rc != 0:
            raise RuntimeError("kmp_bisect_subset_fast failed")
        return side.astype(bool)

    def bisect_subset_ml(self, nodes, target1, cap1, cap2, reps=8):
        """Multilevel bisection of a vertex subset (heavy-edge matching
        + FM at every level; best of reps)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        side = np.zeros(len(nodes), dtype=np.uint8)
        rc = _lib.kmp_bisect_subset_ml(
            self._h, _u32p(nodes), len(nodes), int(target1), int(cap1),
            int(cap2), reps, side.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        if rc != 0:
            raise RuntimeError("kmp_bisect_subset_ml failed")
        return side.astype(bool)

    def partition_deep_native(self, k, eps=0.03, seed=1, iters=5, jet=False,
                              fm=None, resident=False, engine=None,
                              contraction_limit=0, stop_n=0, split_c=0,
                              return_stats=False, vcycles=0, sparsify=False):
        """Progressive-k multilevel partition driven entirely from the C
        ABI (kmp_partition_deep_ex). Bit-identical to
        kaminpar_amd.partition.partition_deep with the same keywords (see
        partition_native; `split_c` 0 = auto). Requires a GPU.

        Returns (cut, partition); with return_stats also a PipelineStats."""
        return self._partition_ex(
            _lib.kmp_partition_deep_ex, "kmp_partition_deep_ex", k, eps, seed,
            iters, jet, fm, resident, engine, contraction_limit, stop_n,
            split_c, return_stats, vcycles, sparsify)

    def vcycle_native(self, k, partition, eps=0.03, seed=1, iters=5, jet=False,
                      fm=None, resident=False, engine=None,
                      contraction_limit=0, stop_n=0):
        """One V-cycle driven entirely from the C ABI (kmp_vcycle_ex).
        Bit-identical to kaminpar_amd.partition.vcycle with the same keywords.
        partition=None (needs resident and engine) runs on the engine's
        resident partition, leaves the result there and returns None in its
        place. Requires a GPU.

        Returns (cut, partition, PipelineStats)."""
        opts = pipeline_opts(iters=iters, jet=jet, fm=fm, resident=resident,
                             engine=engine, contraction_limit=contraction_limit,
                             stop_n=stop_n)
        part = None
        if partition is not None:
            part = np.ascontiguousarray(partition, dtype=np.uint32).copy()
            if len(part) != self.n:
                raise ValueError("vcycle_native(): need n labels")
        stats = PipelineStats()
        cut = _lib.kmp_vcycle_ex(self._h, k, eps, seed, ctypes.byref(opts),
                                 None if part is None else _u32p(part),
                                 ctypes.byref(stats))
        if cut < 0:
            raise RuntimeError("kmp_vcycle_ex failed")
        return cut, part, stats

    def initial_partition_native(self, k, max_block_weight, reps=8):
        """C++ recursive-bisection initial partitioning (equivalent to
        kaminpar_amd.partition.initial_partition; host-only, no GPU)."""
        part = np.zeros(self.n, dtype=np.uint32)
        rc = _lib.kmp_initial_partition(self._h, k, max_block_weight, reps,
                                        _u32p(part))
        if rc != 0:
            raise RuntimeError("kmp_initial_partition failed")
        return part

    def rearrange_degree_buckets(self):
        """Degree-bucket rearrangement (the reference's default
        NodeOrdering::DEGREE_BUCKETS preprocessing).

        Returns (permuted_graph, perm) with perm[u_old] = u_new; a labelling
        l_new on the permuted graph maps back as l_old = l_new[perm]."""
        perm = np.zeros(self.n, dtype=np.uint32)
        h = _lib.kmp_rearrange_degree_buckets(self._h, _u32p(perm))
        return Graph(h), perm

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.kmp_graph_free(h)
            self._h = None


def random_partition(n, k, seed=42):
    """Deterministic pseudo-random balanced-in-expectation partition."""
    with np.errstate(over="ignore"):
        u = np.arange(n, dtype=np.uint64)
        x = u + np.uint64((0x9E3779B97F4A7C15 * (seed + 1)) & 0xFFFFFFFFFFFFFFFF)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x % np.uint64(k)).astype(np.uint32)


class LpEngine:
    """Device-resident LP engine (requires a GPU; fails loudly otherwise)."""

    def __init__(self, graph=None, _handle=None):
        self._graph = graph  # keep alive (None for device-resident engines)
        if _handle is not None:
            self._h = _handle
        else:
            self._h = _lib.kmp_lp_create(graph._h)
        if not self._h:
            raise RuntimeError(
                "kaminpar_amd: LP engine creation failed (no HIP GPU available?)"
            )
        self.n = int(_lib.kmp_lp_n(self._h))
        self.m = int(_lib.kmp_lp_m(self._h))
        self.sparsify_stats = None  # set by contract_engine(sparsify=...)

    @staticmethod
    def _is_tensor(a):
        return type(a).__module__.split(".")[0] == "torch"

    @classmethod
    def from_edges(cls, src, dst, n=None, weights=None, vwgt=None,
                   combine="max", return_stats=False, _flags=0):
        """An engine built on the device from an edge list
        (kmp_lp_create_from_edges; rule in include/kaminpar_lp.h): the pairs
        (src[i], dst[i]) may be unsorted, repeated and one-directional; the
        engine holds the canonical CSR of the undirected simple graph, which
        never exists on the host. `n=None` infers n as the largest id + 1.
        `weights` (int32, > 0) makes the graph weighted; parallel edges then
        keep the maximum weight, or with combine="sum" their sum. `vwgt`
        (int32, n entries) needs n.

        The arrays are either all numpy (ids uint32 or int64; int32 is widened
        to int64, so that a negative id is caught) or all contiguous torch
        tensors on torch's current GPU, which is where the engine is created
        (ids int64 or int32), whose memory the build reads
        in place after synchronising torch's current stream; the build itself
        runs on the engine's own stream. Mixing the two, a non-contiguous
        tensor or ids of another type raise ValueError; an invalid list (an id
        out of range, a weight <= 0, an overflowing sum, no n and no pairs,
        2^31 pairs or more) raises RuntimeError. The inputs are not modified.

        Returns the engine, with return_stats (engine, EdgesStats)."""
        if combine not in ("max", "sum"):
            raise ValueError("combine must be 'max' or 'sum'")
        given = [a for a in (src, dst, weights, vwgt) if a is not None]
        on_dev = [cls._is_tensor(a) for a in given]
        if any(on_dev) and not all(on_dev):
            raise ValueError("from_edges(): host arrays and GPU tensors cannot be mixed")
        if vwgt is not None and not n:
            raise ValueError("from_edges(): vwgt needs n")
        n = int(n) if n else 0
        if not 0 <= n < (1 << 32):
            raise ValueError("from_edges(): n must be in [1, 2^32)")
        flags = int(_flags) | (EDGES_SUM if combine == "sum" else 0)
        if all(on_dev):
            import torch

            for a in given:
                if not a.is_cuda:
                    raise ValueError("from_edges(): tensors must be on the GPU")
                if a.device.index != torch.cuda.current_device():
                    raise ValueError("from_edges(): tensors must be on the current "
                                     "device, where the engine is created")
                if not a.is_contiguous():
                    raise ValueError("from_edges(): tensors must be contiguous")
                if a.dim() != 1:
                    raise ValueError("from_edges(): tensors must be one-dimensional")
            if src.dtype != dst.dtype or src.dtype not in (torch.int64, torch.int32):
                raise ValueError("from_edges(): id tensors must both be int64 or int32")
            for a in (weights, vwgt):
                if a is not None and a.dtype != torch.int32:
                    raise ValueError("from_edges(): weights and vwgt must be int32")
            flags |= EDGES_DEVICE
            flags |= EDGES_IDS64 if src.dtype == torch.int64 else EDGES_IDS_I32
            num_pairs = src.numel()
            sizes = (dst.numel(), None if weights is None else weights.numel(),
                     None if vwgt is None else vwgt.numel())
            torch.cuda.current_stream(src.device).synchronize()

            def ptr(a):
                return None if a is None or a.numel() == 0 else a.data_ptr()
        else:
            src, dst = np.asarray(src), np.asarray(dst)
            if src.dtype == np.int32 and dst.dtype == np.int32:
                src, dst = src.astype(np.int64), dst.astype(np.int64)
            if src.dtype != dst.dtype or src.dtype not in (np.uint32, np.int64):
                raise ValueError("from_edges(): id arrays must both be uint32, int64 or int32")
            if src.ndim != 1 or dst.ndim != 1:
                raise ValueError("from_edges(): arrays must be one-dimensional")
            src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
            if weights is not None:
                weights = np.ascontiguousarray(weights, dtype=np.int32)
            if vwgt is not None:
                vwgt = np.ascontiguousarray(vwgt, dtype=np.int32)
            if src.dtype == np.int64:
                flags |= EDGES_IDS64
            num_pairs = src.size
            sizes = (dst.size, None if weights is None else weights.size,
                     None if vwgt is None else vwgt.size)

            def ptr(a):
                return None if a is None or a.size == 0 else a.ctypes.data
        if sizes[0] != num_pairs or sizes[1] not in (None, num_pairs):
            raise ValueError("from_edges(): src, dst and weights differ in length")
        if sizes[2] not in (None, n):
            raise ValueError("from_edges(): vwgt needs n entries")
        stats = EdgesStats()
        h = _lib.kmp_lp_create_from_edges(
            n, num_pairs, ptr(src), ptr(dst), ptr(weights), ptr(vwgt), flags,
            ctypes.byref(stats))
        if not h:
            raise RuntimeError("kmp_lp_create_from_edges failed")
        eng = cls(_handle=h)
        eng.edges_stats = stats
        return (eng, stats) if return_stats else eng

    @classmethod
    def from_edge_index(cls, edge_index, **kw):
        """from_edges() for a contiguous [2, E] array or GPU tensor: row 0
        holds the sources, row 1 the targets. Keywords as in from_edges()."""
        if not cls._is_tensor(edge_index):
            edge_index = np.asarray(edge_index)
            contiguous = edge_index.flags["C_CONTIGUOUS"]
            dims = edge_index.ndim
        else:
            contiguous = edge_index.is_contiguous()
            dims = edge_index.dim()
        if dims != 2 or edge_index.shape[0] != 2:
            raise ValueError("from_edge_index(): need a [2, E] array or tensor")
        if not contiguous:
            raise ValueError("from_edge_index(): edge_index must be contiguous")
        return cls.from_edges(edge_index[0], edge_index[1], **kw)

    @staticmethod
    def _host_part(partition):
        if partition is None:
            return None
        return np.ascontiguousarray(partition, dtype=np.uint32).copy()

    @staticmethod
    def _part_ptr(part):
        return None if part is None else _u32p(part)

    def refine(self, k, max_block_weights, partition, seed=1, iters=5):
        """Deterministic LP refinement; returns (cut, partition, Stats).
        partition=None refines the engine's resident partition in place and
        returns (cut, None, Stats). k may be up to KMP_LP_MAX_K = 2**24:
        above 2048 the gain tables are hashes sized by degree instead of
        dense tables sized by k (same result as the oracle either way), and
        a label >= k raises."""
        part = self._host_part(partition)
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        stats = Stats()
        cut = _lib.kmp_lp_refine(
            self._h, k, _i64p(mbw), self._part_ptr(part), seed, iters,
            ctypes.byref(stats)
        )
        if cut < 0:
            raise RuntimeError("kmp_lp_refine failed")
        return cut, part, stats

    def balance(self, k, max_block_weights, partition, seed=1, iters=5):
        """Overload-balancer mode: repair an infeasible partition (blocks
        over their caps shed boundary vertices at best admissible gain).
        Returns (cut, partition, Stats). k up to KMP_LP_MAX_K as in refine();
        the host parts are the isolated vertices of over-cap blocks (an
        ordered set of blocks) and an O(k) scan per chunk for the lightest
        block with room (balance_host_ns() reports their time)."""
        part = np.ascontiguousarray(partition, dtype=np.uint32).copy()
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        stats = Stats()
        cut = _lib.kmp_lp_balance(
            self._h, k, _i64p(mbw), _u32p(part), seed, iters, ctypes.byref(stats)
        )
        if cut < 0:
            raise RuntimeError("kmp_lp_balance failed")
        return cut, part, stats

    def balance_host_ns(self):
        """(pre-pass ns, per-chunk fallback scan ns) of the last balance()."""
        out = (ctypes.c_uint64 * 2)()
        _lib.kmp_lp_balance_host_ns(self._h, out)
        return int(out[0]), int(out[1])

    def jet(self, k, max_block_weights, partition, seed=1, coarse_level=0,
            **params):
        """Jet refinement (kmp_lp_jet): synchronous find / afterburner /
        execute iterations with deterministic rebalancing, returning the best
        partition seen. `params` override fields of the reference defaults
        (kmp_jet_params_default(coarse_level)): num_rounds, max_iterations,
        max_fruitless, fruitless_threshold, initial_gain_temp,
        final_gain_temp, balance_iters, balancer (JET_BALANCER_LP or
        JET_BALANCER_SELECT), balance_passes. Returns (cut, partition,
        JetStats). partition=None runs on the engine's resident partition and
        returns (cut, None, JetStats)."""
        jp = _lib.kmp_jet_params_default(int(coarse_level))
        names = {f[0] for f in JetParams._fields_}
        for key, val in params.items():
            if key not in names:
                raise TypeError(f"jet() got an unknown parameter {key!r}")
            setattr(jp, key, val)
        part = self._host_part(partition)
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        if len(mbw) != k or (part is not None and len(part) != self.n):
            raise ValueError("jet(): need k caps and n labels")
        stats = JetStats()
        cut = _lib.kmp_lp_jet(
            self._h, k, _i64p(mbw), self._part_ptr(part), seed, ctypes.byref(jp),
            ctypes.byref(stats)
        )
        if cut < 0:
            raise RuntimeError("kmp_lp_jet failed")
        return cut, part, stats

    def rebalance(self, k, max_block_weights, partition, max_passes=16):
        """Selection rebalancer (kmp_lp_rebalance): every over-cap block gives
        up its best relative gains until the overload is covered, in up to
        `max_passes` deterministic passes. A feasible input comes back
        unchanged; a call that stalls returns what it reached with
        stats.feasible == 0. Returns (cut, partition, RebalanceStats).
        partition=None runs on the engine's resident partition and returns
        (cut, None, RebalanceStats)."""
        part = self._host_part(partition)
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        if len(mbw) != k or (part is not None and len(part) != self.n):
            raise ValueError("rebalance(): need k caps and n labels")
        stats = RebalanceStats()
        cut = _lib.kmp_lp_rebalance(
            self._h, k, _i64p(mbw), self._part_ptr(part), int(max_passes),
            ctypes.byref(stats)
        )
        if cut < 0:
            raise RuntimeError("kmp_lp_rebalance failed")
        return cut, part, stats

    def underload(self, k, max_block_weights, min_block_weights, partition,
                  seed=1, iters=5):
        """Underload-balancer mode: fill blocks below their minimum weight
        (presets.cc:332-338 UNDERLOAD_BALANCER role; semantics restated from
        refinement/balancer/underload_balancer.cc). Returns
        (cut, partition, Stats)."""
        part = np.ascontiguousarray(partition, dtype=np.uint32).copy()
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        mnw = np.ascontiguousarray(min_block_weights, dtype=np.int64)
        stats = Stats()
        cut = _lib.kmp_lp_underload(
            self._h, k, _i64p(mbw), _i64p(mnw), _u32p(part), seed, iters,
            ctypes.byref(stats)
        )
        if cut < 0:
            raise RuntimeError("kmp_lp_underload failed")
        return cut, part, stats

    def rearrange_degree_buckets(self):
        """On-GPU degree-bucket rearrangement of the engine's CSR (the
        reference's default preprocessing, permutator.cc:36-110).
        Returns perm with perm[u_old] = u_new."""
        perm = np.zeros(self.n, dtype=np.uint32)
        rc = _lib.kmp_lp_rearrange_degree_buckets(self._h, _u32p(perm))
        if rc != 0:
            raise RuntimeError("kmp_lp_rearrange_degree_buckets failed")
        return perm

    def set_communities(self, communities):
        """Restrict clustering merges to stay within communities
        (coarsening/clusterer.h:35, lp_clusterer.cc:193-194). None clears."""
        if communities is None:
            _lib.kmp_lp_set_communities(self._h, None)
            self._comm_keepalive = None
            return
        comm = np.ascontiguousarray(communities, dtype=np.uint32)
        _lib.kmp_lp_set_communities(self._h, _u32p(comm))
        self._comm_keepalive = comm

    def cluster(self, max_cluster_weight, clustering=None, desired=0, seed=1, iters=5,
                download=True):
        """Deterministic LP clustering; returns (n_clusters, clustering, Stats).
        download=False leaves the clustering on the device only (for
        contract_engine(None)) and returns None in its place."""
        clus = np.zeros(self.n, dtype=np.uint32) if download else None
        stats = Stats()
        nc = _lib.kmp_lp_cluster(
            self._h, max_cluster_weight, desired, self._part_ptr(clus), seed, iters,
            ctypes.byref(stats),
        )
        if nc < 0:
            raise RuntimeError("kmp_lp_cluster failed")
        return nc, clus, stats

    # sharded API (multi-GPU orchestration; see kaminpar_amd/multi.py)
    def num_chunks(self):
        return _lib.kmp_lp_num_chunks(self._h)

    def refine_begin(self, k, max_block_weights, partition, seed=1):
        part = np.ascontiguousarray(partition, dtype=np.uint32)
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        rc = _lib.kmp_lp_refine_begin(self._h, k, _i64p(mbw), _u32p(part), seed)
        if rc != 0:
            raise RuntimeError("kmp_lp_refine_begin failed")

    def phase_a(self, it, chunk, pos_lo, pos_hi, d_out_ptr, cap):
        cnt = _lib.kmp_lp_phase_a(self._h, it, chunk, pos_lo, pos_hi, d_out_ptr, cap)
        if cnt < 0:
            raise RuntimeError("kmp_lp_phase_a failed")
        return int(cnt)

    def commit(self, it, chunk, d_props_ptr, count):
        mv = _lib.kmp_lp_commit(self._h, it, chunk, d_props_ptr, count)
        if mv < 0:
            raise RuntimeError("kmp_lp_commit failed")
        return int(mv)

    def refine_dist_cpp(self, k, max_block_weights, partition, seed, iters,
                        nccl_comm, rank, world):
        """C++ RCCL-driven sharded refinement (see kmp_lp_refine_dist)."""
        part = np.ascontiguousarray(partition, dtype=np.uint32).copy()
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        stats = Stats()
        cut = _lib.kmp_lp_refine_dist(
            self._h, k, _i64p(mbw), _u32p(part), seed, iters,
            nccl_comm, rank, world, ctypes.byref(stats))
        if cut < 0:
            raise RuntimeError("kmp_lp_refine_dist failed")
        return cut, part, stats

    def set_stream(self, stream_ptr):
        """Adopt an external HIP stream (torch: cuda.current_stream().cuda_stream);
        None restores the engine's own stream."""
        rc = _lib.kmp_lp_set_stream(self._h, stream_ptr)
        if rc != 0:
            raise RuntimeError("kmp_lp_set_stream failed")

    def shard_begin(self, c_lo, c_hi, d_props_ptr, count, d_dep_out_ptr):
        """Sharded commit step 1: sort own targets from the all-gathered
        list + full-admission departure contributions (device ptrs)."""
        rc = _lib.kmp_lp_shard_begin(self._h, c_lo, c_hi, d_props_ptr, count,
                                     d_dep_out_ptr)
        if rc != 0:
            raise RuntimeError("kmp_lp_shard_begin failed")

    def shard_round(self, c_lo, c_hi, d_dep_global_ptr, d_delta_out_ptr):
        rc = _lib.kmp_lp_shard_round(self._h, c_lo, c_hi, d_dep_global_ptr,
                                     d_delta_out_ptr)
        if rc != 0:
            raise RuntimeError("kmp_lp_shard_round failed")

    def shard_finish_meta(self, c_lo, c_hi, d_cutoff_ptr, d_arr_ptr):
        rc = _lib.kmp_lp_shard_finish_meta(self._h, c_lo, c_hi, d_cutoff_ptr,
                                           d_arr_ptr)
        if rc != 0:
            raise RuntimeError("kmp_lp_shard_finish_meta failed")

    def shard_apply(self, it, chunk, d_props_ptr, count, d_cutoff_ptr,
                    d_arr_ptr, d_dep_ptr):
        mv = _lib.kmp_lp_shard_apply(self._h, it, chunk, d_props_ptr, count,
                                     d_cutoff_ptr, d_arr_ptr, d_dep_ptr)
        if mv < 0:
            raise RuntimeError("kmp_lp_shard_apply failed")
        return int(mv)

    def reset(self):
        if _lib.kmp_lp_reset(self._h) != 0:
            raise RuntimeError("kmp_lp_reset failed")

    def run_sweeps(self, iters=5):
        mv = _lib.kmp_lp_run_sweeps(self._h, iters)
        if mv < 0:
            raise RuntimeError("kmp_lp_run_sweeps failed")
        return int(mv)

    def get_stats(self):
        stats = Stats()
        _lib.kmp_lp_get_stats(self._h, ctypes.byref(stats))
        return stats

    def contract(self, clustering):
        """Contract a clustering into the coarse graph (GPU).

        Returns (coarse_graph: Graph, mapping: np.ndarray[u32])."""
        clus = np.ascontiguousarray(clustering, dtype=np.uint32)
        mapping = np.zeros(self.n, dtype=np.uint32)
        out = ctypes.c_void_p()
        c_n = _lib.kmp_contract(self._h, _u32p(clus), _u32p(mapping), ctypes.byref(out))
        if c_n < 0:
            raise RuntimeError("kmp_contract failed")
        return Graph(out.value), mapping

    def contract_engine(self, clustering=None, download_mapping=True,
                        sparsify=None, seed=0):
        """Contract a clustering and hand the coarse graph directly to a NEW
        engine without a host round-trip (the coarse CSR stays in HBM).
        clustering=None contracts the clustering the last cluster() left on
        the device. The coarse engine keeps the mapping on the device for
        project_from(); download_mapping=False skips its host copy.

        sparsify=True, or a dict of overrides of sparsify_params(), runs the
        threshold edge sparsification of the coarse graph on the device with
        dice seed `seed` before the new engine adopts it
        (kmp_contract_engine_sparsified; rule in include/kaminpar_lp.h). The
        returned engine then carries `sparsify_stats` (a SparsifyStats; None
        otherwise). None or False leaves the pass out.

        Returns (coarse_engine: LpEngine, mapping: np.ndarray[u32] or None).
        Results are identical to contract() + LpEngine(coarse_graph)."""
        clus = None if clustering is None else np.ascontiguousarray(
            clustering, dtype=np.uint32)
        mapping = np.zeros(self.n, dtype=np.uint32) if download_mapping else None
        out = ctypes.c_void_p()
        stats = None
        if not sparsify_on(sparsify):
            c_n = _lib.kmp_contract_engine(self._h, self._part_ptr(clus),
                                           self._part_ptr(mapping), ctypes.byref(out))
        else:
            params = sparsify_params(sparsify)
            stats = SparsifyStats()
            c_n = _lib.kmp_contract_engine_sparsified(
                self._h, self._part_ptr(clus), self._part_ptr(mapping),
                ctypes.byref(params), int(seed) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(out),
                ctypes.byref(stats))
        if c_n < 0:
            raise RuntimeError("kmp_contract_engine failed")
        eng = LpEngine(_handle=out.value)
        eng.sparsify_stats = stats
        return eng, mapping

    def set_labels(self, k, partition):
        """Upload a partition (n labels < k, checked) as the engine's resident
        partition (kmp_lp_set_labels)."""
        part = np.ascontiguousarray(partition, dtype=np.uint32)
        if len(part) != self.n:
            raise ValueError("set_labels(): need n labels")
        if _lib.kmp_lp_set_labels(self._h, int(k), _u32p(part)) != 0:
            raise RuntimeError("kmp_lp_set_labels failed")

    def get_labels(self, out=None):
        """Download the resident partition or clustering (kmp_lp_get_labels).
        With `out`, a contiguous GPU tensor of n 4-byte integers, the labels
        are copied on the device instead (kmp_lp_get_labels_device) and `out`
        is returned."""
        if out is not None:
            import torch

            if (not self._is_tensor(out) or not out.is_cuda or not out.is_contiguous()
                    or out.numel() != self.n or out.element_size() != 4
                    or out.dtype.is_floating_point):
                raise ValueError("get_labels(out=): need a contiguous GPU tensor of n "
                                 "4-byte integers")
            if out.device.index != torch.cuda.current_device():
                raise ValueError("get_labels(out=): the tensor must be on the current "
                                 "device, where the engine lives")
            torch.cuda.current_stream(out.device).synchronize()
            if _lib.kmp_lp_get_labels_device(self._h, out.data_ptr()) != 0:
                raise RuntimeError("kmp_lp_get_labels_device failed")
            return out
        out = np.zeros(self.n, dtype=np.uint32)
        if _lib.kmp_lp_get_labels(self._h, _u32p(out)) != 0:
            raise RuntimeError("kmp_lp_get_labels failed")
        return out

    def project_from(self, coarse):
        """Project the resident partition of `coarse`, an engine made by this
        engine's contract_engine(), onto this engine, on the device
        (kmp_lp_project)."""
        if _lib.kmp_lp_project(coarse._h, self._h) != 0:
            raise RuntimeError("kmp_lp_project failed")

    def set_communities_resident(self):
        """communities := the engine's resident partition, on the device
        (kmp_lp_set_communities_resident); the labels stay. set_communities(None)
        clears them."""
        if _lib.kmp_lp_set_communities_resident(self._h) != 0:
            raise RuntimeError("kmp_lp_set_communities_resident failed")
        self._comm_keepalive = None

    def restrict_to(self, coarse):
        """The inverse of project_from: `coarse`, an engine made by this
        engine's contract_engine(), gets this engine's communities as its
        resident partition, coarse.labels[mapping[u]] = communities[u], on the
        device (kmp_lp_restrict). Raises if the clustering that was contracted
        merged vertices of different communities."""
        if _lib.kmp_lp_restrict(self._h, coarse._h) != 0:
            raise RuntimeError("kmp_lp_restrict failed")

    def labels_from_communities(self):
        """labels := communities on the device: the partition that
        set_communities_resident() saved comes back after cluster() overwrote
        it (kmp_lp_labels_from_communities)."""
        if _lib.kmp_lp_labels_from_communities(self._h) != 0:
            raise RuntimeError("kmp_lp_labels_from_communities failed")

    def resident_cut(self, k, max_block_weights):
        """(edge cut, feasible) of the resident partition under k caps, without
        a download (kmp_lp_resident_cut)."""
        mbw = np.ascontiguousarray(max_block_weights, dtype=np.int64)
        if len(mbw) != k:
            raise ValueError("resident_cut(): need k caps")
        feas = ctypes.c_int32(0)
        cut = _lib.kmp_lp_resident_cut(self._h, int(k), _i64p(mbw),
                                       ctypes.byref(feas))
        if cut < 0:
            raise RuntimeError("kmp_lp_resident_cut failed")
        return int(cut), bool(feas.value)

    def extract_subgraphs(self, k, partition):
        """All block-induced subgraphs of `partition` (n labels < k <= 2048),
        packed on the device (kmp_lp_extract_subgraphs). The engine's own
        label state is not touched. Returns a Subgraphs object."""
        part = np.ascontiguousarray(partition, dtype=np.uint32)
        if len(part) != self.n:
            raise ValueError("extract_subgraphs(): need n labels")
        mapping = np.zeros(self.n, dtype=np.uint32)
        stats = ExtractStats()
        h = _lib.kmp_lp_extract_subgraphs(
            self._h, int(k), _u32p(part), _u32p(mapping), ctypes.byref(stats))
        if not h:
            raise RuntimeError("kmp_lp_extract_subgraphs failed")
        return Subgraphs(h, self.n, mapping, stats)

    def download_graph(self):
        """Download the engine's device-resident CSR into a host Graph."""
        h = _lib.kmp_lp_download_graph(self._h)
        return Graph(h)

    def refine_end(self):
        part = np.zeros(self.n, dtype=np.uint32)
        stats = Stats()
        cut = _lib.kmp_lp_refine_end(self._h, _u32p(part), ctypes.byref(stats))
        return cut, part, stats

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.kmp_lp_free(h)
            self._h = None


class Subgraphs:
    """Device-resident packed block subgraphs (kmp_subgraphs_t; layout rule
    in include/kaminpar_lp.h). `mapping[u]` is the rank of u inside its block,
    `nodes` the vertex ids by (block, id), `node_offsets` / `arc_offsets` the
    k + 1 block starts in `nodes` and in the packed arcs."""

    def __init__(self, handle, n, mapping, stats):
        self._h = handle
        self.k = int(_lib.kmp_subgraphs_k(handle))
        self.mapping = mapping
        self.stats = stats
        self.nodes = np.zeros(n, dtype=np.uint32)
        self.node_offsets = np.zeros(self.k + 1, dtype=np.uint32)
        self.arc_offsets = np.zeros(self.k + 1, dtype=np.uint64)
        _lib.kmp_subgraphs_layout(
            handle, _u32p(self.nodes), _u32p(self.node_offsets),
            self.arc_offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))

    def graph(self, b):
        """Host copy of block b's subgraph (0 vertices for an empty block)."""
        return Graph(_lib.kmp_subgraphs_download(self._h, int(b)))

    def engine(self, b):
        """New LpEngine holding block b's subgraph, copied device-to-device;
        it outlives this object and the parent engine. None for an empty
        block."""
        if not 0 <= int(b) < self.k:
            raise ValueError(f"block {b} is not below k = {self.k}")
        h = _lib.kmp_subgraphs_engine(self._h, int(b))
        return LpEngine(_handle=h) if h else None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.kmp_subgraphs_free(h)
            self._h = None
