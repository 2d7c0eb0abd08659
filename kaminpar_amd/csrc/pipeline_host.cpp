// Multilevel pipeline drivers and the ckaminpar-shaped shim, on top of the
// C ABI in include/kaminpar_lp.h: kmp_partition(_ex), kmp_partition_deep(_ex)
// and kaminpar_amd_*. Host code only -- every device-side step is an entry
// point of the engine (lp_hip.hip); nothing here launches a kernel.
//
// The two drivers are the C twins of kaminpar_amd/partition.py partition()
// and partition_deep(): same call order, seeds and caps, so the results are
// bit-identical (keep the schedule in sync; pinned by
// tests/test_gpu_parity.py, tests/test_cpipeline_gpu.py and the pipeline
// goldens under tests/golden/).

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/kaminpar_lp.h"

using u32 = uint32_t;
using u64 = uint64_t;
using i32 = int32_t;
using i64 = int64_t;

namespace {

i64 level_cluster_weight(i64 total_w, u32 n, u32 k, double eps, u32 C) {
  u64 shrink = n / C;
  if (shrink < 2) {
    shrink = 2;
  }
  if (shrink > k) {
    shrink = k;
  }
  const i64 eps_rule = static_cast<i64>(eps * static_cast<double>(total_w) /
                                        static_cast<double>(shrink));
  const i64 block_rule = total_w / (12ll * k);
  i64 mcw = block_rule > 0 ? std::min(eps_rule, block_rule) : eps_rule;
  return mcw < 1 ? 1 : mcw;
}

// Adds the host wall time of a scope to one of the stats' phase counters.
struct PhaseTimer {
  u64 &acc;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit PhaseTimer(u64 &a) : acc(a) {}
  ~PhaseTimer() {
    acc += static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                std::chrono::steady_clock::now() - t0)
                                .count());
  }
};

// One line on stderr and -1 for options the drivers refuse; decided on the
// host before any engine exists.
int check_opts(const kmp_graph_t *g, u32 k, const kmp_pipeline_opts_t &o, const char *who) {
  if (o.fm < -1 || o.fm > 1) {
    fprintf(stderr, "kaminpar_amd: %s: fm = %d is not -1, 0 or 1\n", who, o.fm);
    return -1;
  }
  if (o.jet != 0 && o.jet != 1) {
    fprintf(stderr, "kaminpar_amd: %s: jet = %d is not 0 or 1\n", who, o.jet);
    return -1;
  }
  if (o.resident != 0 && o.resident != 1) {
    fprintf(stderr, "kaminpar_amd: %s: resident = %d is not 0 or 1\n", who, o.resident);
    return -1;
  }
  if (o.vcycles < 0 || o.vcycles > KMP_PIPELINE_MAX_VCYCLES) {
    fprintf(stderr, "kaminpar_amd: %s: vcycles = %d is not in 0 .. %d\n", who, o.vcycles,
            KMP_PIPELINE_MAX_VCYCLES);
    return -1;
  }
  if (o.sparsify != 0 && o.sparsify != 1) {
    fprintf(stderr, "kaminpar_amd: %s: sparsify = %d is not 0 or 1\n", who, o.sparsify);
    return -1;
  }
  if (o.sparsify == 1 && !kmp_sparsify_params_valid(&o.sparsify_params)) {
    fprintf(stderr, "kaminpar_amd: %s: kmp_contract_engine_sparsified would refuse "
                    "sparsify_params\n", who);
    return -1;
  }
  if (o.jet == 1 && k > KMP_JET_MAX_K) {
    fprintf(stderr, "kaminpar_amd: %s: jet supports k <= %u (got %u)\n", who, KMP_JET_MAX_K, k);
    return -1;
  }
  if (o.jet == 1 && (!kmp_jet_params_valid(&o.jet_fine) || !kmp_jet_params_valid(&o.jet_coarse))) {
    fprintf(stderr, "kaminpar_amd: %s: kmp_lp_jet would refuse jet_%s\n", who,
            kmp_jet_params_valid(&o.jet_fine) ? "coarse" : "fine");
    return -1;
  }
  if (o.engine != nullptr &&
      (kmp_lp_n(o.engine) != kmp_graph_n(g) || kmp_lp_m(o.engine) != kmp_graph_m(g))) {
    fprintf(stderr,
            "kaminpar_amd: %s: engine holds n = %u, m = %llu, the graph n = %u, m = %llu\n", who,
            kmp_lp_n(o.engine), static_cast<unsigned long long>(kmp_lp_m(o.engine)),
            kmp_graph_n(g), static_cast<unsigned long long>(kmp_graph_m(g)));
    return -1;
  }
  return 0;
}

// The multilevel chain of one call: engines, level sizes, the host mappings
// (resident = 0 only) and the partition of the current level, which lives
// either in `part` or in the current engine's resident labels.
struct Chain {
  const kmp_graph_t *g;
  u32 k;
  u64 seed;
  kmp_pipeline_opts_t o;
  bool fm_on;
  std::vector<kmp_lp_t *> engines;
  std::vector<u32> sizes;
  std::vector<u64> arcs; // m of every level's engine (the bottom-up pass)
  std::vector<std::vector<u32>> mappings;
  std::vector<u32> part;
  bool on_host = true; // where the current level's partition is
  kmp_pipeline_stats_t st{};

  ~Chain() {
    for (size_t i = 0; i < engines.size(); ++i) {
      if (i > 0 || engines[i] != o.engine) {
        kmp_lp_free(engines[i]);
      }
    }
  }

  // partition.py: the coarsening loop shared by both drivers. cycle: the
  // V-cycle's form of it (vcycle()): the level's partition is the clusterer's
  // communities and is restricted to every coarse level that is kept; on
  // entry it is engines[0]'s resident partition, already its communities
  // (resident = 1), or `part`.
  int coarsen(double eps, bool cycle = false) {
    kmp_lp_t *fine = o.engine != nullptr ? o.engine : kmp_lp_create(g);
    if (fine == nullptr) {
      return -1;
    }
    engines.push_back(fine);
    sizes.push_back(kmp_graph_n(g));
    arcs.push_back(kmp_lp_m(fine));
    const i64 total_w = kmp_graph_total_node_weight(g);
    const u32 stop = std::max(o.stop_n, 2 * k);
    std::vector<u32> clus;
    kmp_lp_stats_t lst;
    while (sizes.back() > stop) {
      const u32 cur_n = sizes.back();
      const i64 mcw = level_cluster_weight(total_w, cur_n, k, eps, o.contraction_limit);
      if (!o.resident) {
        clus.resize(cur_n);
      }
      if (cycle && o.resident && engines.size() > 1 &&
          kmp_lp_set_communities_resident(engines.back()) != 0) {
        return -1;
      }
      if (cycle && !o.resident && kmp_lp_set_communities(engines.back(), part.data()) != 0) {
        return -1;
      }
      {
        PhaseTimer t(st.cluster_ns);
        if (kmp_lp_cluster(engines.back(), mcw, 0, o.resident ? nullptr : clus.data(),
                           seed + mappings.size(), o.iters, &lst) < 0) {
          return -1;
        }
      }
      std::vector<u32> mapping(o.resident ? 0 : cur_n);
      kmp_lp_t *coarse_eng = nullptr;
      kmp_sparsify_stats_t sst{};
      {
        PhaseTimer t(st.contract_ns);
        // the V-cycle's chains coarsen without sparsification
        const i64 rc =
            (o.sparsify && !cycle)
                ? kmp_contract_engine_sparsified(
                      engines.back(), o.resident ? nullptr : clus.data(),
                      o.resident ? nullptr : mapping.data(), &o.sparsify_params,
                      seed + mappings.size(), &coarse_eng, &sst)
                : kmp_contract_engine(engines.back(), o.resident ? nullptr : clus.data(),
                                      o.resident ? nullptr : mapping.data(), &coarse_eng);
        if (rc < 0) {
          return -1;
        }
      }
      const u32 c_n = kmp_lp_n(coarse_eng);
      if (static_cast<double>(c_n) > 0.95 * static_cast<double>(cur_n)) {
        kmp_lp_free(coarse_eng);
        // the clustering overwrote this level's resident partition
        if (cycle && o.resident && kmp_lp_labels_from_communities(engines.back()) != 0) {
          return -1;
        }
        break;
      }
      if (engines.size() >= static_cast<size_t>(KMP_PIPELINE_MAX_LEVELS)) {
        kmp_lp_free(coarse_eng);
        fprintf(stderr, "kaminpar_amd: coarsening produced more than %d levels\n",
                KMP_PIPELINE_MAX_LEVELS);
        return -1;
      }
      if (cycle && o.resident && kmp_lp_restrict(engines.back(), coarse_eng) != 0) {
        kmp_lp_free(coarse_eng);
        return -1;
      }
      if (cycle && !o.resident) {
        std::vector<u32> coarse_part(c_n, 0);
        for (u32 u = 0; u < cur_n; ++u) {
          coarse_part[mapping[u]] = part[u];
        }
        u64 bad = 0;
        for (u32 u = 0; u < cur_n; ++u) {
          bad += coarse_part[mapping[u]] != part[u] ? 1 : 0;
        }
        if (bad != 0) {
          kmp_lp_free(coarse_eng);
          fprintf(stderr, "kaminpar_amd: vcycle: %llu fine vertices share a coarse vertex with a "
                          "vertex of another block\n", static_cast<unsigned long long>(bad));
          return -1;
        }
        part = std::move(coarse_part);
      }
      engines.push_back(coarse_eng);
      mappings.push_back(std::move(mapping));
      sizes.push_back(c_n);
      arcs.push_back(kmp_lp_m(coarse_eng));
      if (sst.applied) {
        st.sparsified_levels += 1;
        st.sparsify_arcs_dropped += sst.m_before - sst.m_after;
        st.sparsify_ns += sst.pass_ns;
      }
    }
    return 0;
  }

  // the partition of engines[level] on the host, downloading it if it is resident
  int to_host(size_t level) {
    if (!on_host) {
      part.resize(sizes[level]);
      if (kmp_lp_get_labels(engines[level], part.data()) != 0) {
        return -1;
      }
      on_host = true;
    }
    return 0;
  }

  // resident = 1: the partition of engines[level] on the device
  int to_device(size_t level) {
    if (on_host) {
      if (kmp_lp_set_labels(engines[level], k, part.data()) != 0) {
        return -1;
      }
      on_host = false;
    }
    return 0;
  }

  // LP refinement, then Jet, on engines[level] with the given caps. Returns
  // the level's cut or -1.
  i64 refine_level(size_t level, const i64 *caps) {
    kmp_lp_stats_t lst;
    u32 *p = on_host ? part.data() : nullptr;
    i64 cut;
    {
      PhaseTimer t(st.refine_ns);
      cut = kmp_lp_refine(engines[level], k, caps, p, seed, o.iters, &lst);
    }
    if (cut >= 0 && o.jet) {
      PhaseTimer t(st.jet_ns);
      kmp_jet_stats_t jst;
      cut = kmp_lp_jet(engines[level], k, caps, p, seed, level == 0 ? &o.jet_fine : &o.jet_coarse,
                       &jst);
      if (cut >= 0) {
        st.jet_iterations += jst.iterations;
        st.jet_moves += jst.jet_moves;
        st.jet_balancer_calls += jst.balancer_calls;
      }
    }
    return cut;
  }

  // CPU k-way FM on the level's host graph (hg, or a download of the level's
  // engine if NULL). *cut is recomputed on level 0 only, as in partition.py.
  int fm_level(size_t level, const i64 *caps, const kmp_graph_t *hg, i64 *cut) {
    PhaseTimer t(st.fm_ns);
    kmp_graph_t *owned = nullptr;
    if (hg == nullptr) {
      owned = level == 0 ? nullptr : kmp_lp_download_graph(engines[level]);
      hg = level == 0 ? g : owned;
      if (hg == nullptr) {
        return -1;
      }
    }
    int rc = to_host(level);
    if (rc == 0) {
      kmp_kway_fm(hg, k, caps, part.data(), 0, 0);
      if (level == 0) {
        *cut = kmp_edge_cut_host(g, part.data());
      }
    }
    if (owned != nullptr) {
      kmp_graph_free(owned);
    }
    return rc;
  }

  // the partition of engines[level] carried to engines[level - 1]
  int project(size_t level) {
    if (o.resident) {
      if (to_device(level) != 0) {
        return -1;
      }
      return kmp_lp_project(engines[level], engines[level - 1]);
    }
    const std::vector<u32> &map = mappings[level - 1];
    std::vector<u32> fine(map.size());
    for (size_t u = 0; u < map.size(); ++u) {
      fine[u] = part[map[u]];
    }
    part = std::move(fine);
    return 0;
  }
};

bool host_feasible(const kmp_graph_t *g, const std::vector<u32> &part, const std::vector<i64> &caps) {
  const i32 *vw = kmp_graph_vwgt(g);
  std::vector<i64> w(caps.size(), 0);
  for (size_t u = 0; u < part.size(); ++u) {
    w[part[u]] += vw != nullptr ? vw[u] : 1;
  }
  for (size_t b = 0; b < caps.size(); ++b) {
    if (w[b] > caps[b]) {
      return false;
    }
  }
  return true;
}

// partition.py vcycle_accept()
bool vcycle_accept(bool feasible_in, i64 cut_in, bool feasible_out, i64 cut_out) {
  return feasible_in != feasible_out ? feasible_out : cut_out <= cut_in;
}

// Clears the level-0 engine's communities on every way out of a cycle.
struct CommunitiesGuard {
  kmp_lp_t *e;
  ~CommunitiesGuard() { kmp_lp_set_communities(e, nullptr); }
};

// One V-cycle on eng0, an engine of g: partition.py vcycle() (keep in sync).
// o has its defaults resolved. The input is `part` (on_host) or eng0's
// resident partition; the result is left in `part` (want_host) or resident on
// eng0 (resident = 1 only), and on_host says which. sizes receives the level
// sizes, the phase times are added to st. Returns the cut or -1.
i64 vcycle_core(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, kmp_pipeline_opts_t o, kmp_lp_t *eng0,
    std::vector<u32> &part, bool &on_host, bool want_host, kmp_pipeline_stats_t &st,
    std::vector<u32> &sizes, bool *accepted_out
) {
  const u32 n = kmp_graph_n(g);
  o.engine = eng0; // level 0 of the chain, not freed with it
  Chain c{g, k, seed, o, o.fm < 0 ? n <= (1u << 21) : o.fm == 1};
  CommunitiesGuard guard{eng0};
  const std::vector<i64> mbw(k, kmp_max_block_weight(g, k, eps));

  std::vector<u32> input; // a host input, for a rejected result
  i64 cut_in;
  bool feas_in;
  if (o.resident) {
    if (on_host) {
      if (kmp_lp_set_labels(eng0, k, part.data()) != 0) {
        return -1;
      }
      input = std::move(part);
    }
    int32_t f = 0;
    cut_in = kmp_lp_resident_cut(eng0, k, mbw.data(), &f);
    // kept for the whole cycle: a rejected result is replaced by it
    if (cut_in < 0 || kmp_lp_set_communities_resident(eng0) != 0) {
      return -1;
    }
    feas_in = f != 0;
    c.on_host = false;
  } else {
    cut_in = kmp_edge_cut_host(g, part.data());
    feas_in = host_feasible(g, part, mbw);
    input = part;
    c.part = std::move(part);
    c.on_host = true;
  }

  if (c.coarsen(eps, true) != 0) {
    return -1;
  }
  i64 cut = cut_in;
  for (size_t level = c.engines.size(); level-- > 0;) {
    cut = c.refine_level(level, mbw.data());
    if (cut < 0) {
      return -1;
    }
    if (c.fm_on && c.fm_level(level, mbw.data(), nullptr, &cut) != 0) {
      return -1;
    }
    if (level > 0 && c.project(level) != 0) {
      return -1;
    }
  }

  bool feas;
  if (!c.on_host) {
    int32_t f = 0;
    cut = kmp_lp_resident_cut(eng0, k, mbw.data(), &f);
    if (cut < 0) {
      return -1;
    }
    feas = f != 0;
  } else {
    cut = kmp_edge_cut_host(g, c.part.data());
    feas = host_feasible(g, c.part, mbw);
  }
  const bool accepted = vcycle_accept(feas_in, cut_in, feas, cut);
  if (!accepted) {
    cut = cut_in;
    if (o.resident) { // level 0 still has the input as its communities
      if (kmp_lp_labels_from_communities(eng0) != 0) {
        return -1;
      }
      c.on_host = false;
      if (want_host && !input.empty()) {
        c.part = std::move(input);
        c.on_host = true;
      }
    } else {
      c.part = std::move(input);
      c.on_host = true;
    }
  }
  if (want_host ? c.to_host(0) != 0 : c.to_device(0) != 0) {
    return -1;
  }
  on_host = c.on_host;
  if (on_host) {
    part = std::move(c.part);
  }
  sizes = c.sizes;
  st.jet_iterations += c.st.jet_iterations;
  st.jet_moves += c.st.jet_moves;
  st.jet_balancer_calls += c.st.jet_balancer_calls;
  st.cluster_ns += c.st.cluster_ns;
  st.contract_ns += c.st.contract_ns;
  st.refine_ns += c.st.refine_ns;
  st.jet_ns += c.st.jet_ns;
  st.fm_ns += c.st.fm_ns;
  *accepted_out = accepted;
  return cut;
}

void resolve_defaults(kmp_pipeline_opts_t &o, u32 n) {
  if (o.contraction_limit == 0) {
    o.contraction_limit = 2000;
  }
  if (o.stop_n == 0) {
    o.stop_n = 512;
  }
  if (o.split_c == 0) {
    // auto: fine-level splits up to ~2M vertices, reference-like block
    // sizes beyond (see kaminpar_amd/partition.py partition_deep)
    o.split_c = n <= (1u << 21) ? 262144 : 2000;
  }
  if (o.ip_reps == 0) {
    o.ip_reps = 8;
  }
}

i64 run_pipeline(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, const kmp_pipeline_opts_t *opts,
    u32 *part_out, kmp_pipeline_stats_t *stats, bool deep
) {
  const char *who = deep ? "kmp_partition_deep_ex" : "kmp_partition_ex";
  kmp_pipeline_opts_t o = opts != nullptr ? *opts : kmp_pipeline_opts_default();
  if (check_opts(g, k, o, who) != 0) {
    return -1;
  }
  const u32 n = kmp_graph_n(g);
  resolve_defaults(o, n);

  const auto wall0 = std::chrono::steady_clock::now();
  const u64 traffic0 = kmp_lp_label_traffic_bytes();
  Chain c{g, k, seed, o, o.fm < 0 ? n <= (1u << 21) : o.fm == 1};
  const i64 mbw_val = kmp_max_block_weight(g, k, eps);
  i64 cut = -1;

  // split-schedule dispatch by degree variance of the fine graph (keep in
  // sync with partition_deep): heavy-tailed graphs defer all splits to the
  // finest level (no eager coarsest split); CV^2 >= 1 as for the bisector
  // dispatch.
  bool late_splits = false;
  if (deep) {
    const u32 *fx = kmp_graph_xadj(g);
    unsigned __int128 sum = 0, sq = 0;
    for (u32 u = 0; u < n; ++u) {
      const u64 d = fx[u + 1] - fx[u];
      sum += d;
      sq += d * d;
    }
    const bool heavy = static_cast<unsigned __int128>(n) * sq >= 2 * sum * sum;
    late_splits = heavy && (n <= (1u << 21) || o.split_c >= n);
  }

  if (c.coarsen(eps) != 0) {
    return -1;
  }
  const size_t coarsest = c.engines.size() - 1;

  if (!deep) {
    // initial partition on the coarsest graph (CPU), refine at every level
    kmp_graph_t *cg = coarsest > 0 ? kmp_lp_download_graph(c.engines.back()) : nullptr;
    if (coarsest > 0 && cg == nullptr) {
      return -1;
    }
    c.part.resize(c.sizes.back());
    const int ip = kmp_initial_partition(cg ? cg : g, k, mbw_val, o.ip_reps, c.part.data());
    if (cg != nullptr) {
      kmp_graph_free(cg);
    }
    if (ip != 0) {
      return -1;
    }
    const std::vector<i64> mbw(k, mbw_val);
    if (o.resident && c.to_device(coarsest) != 0) {
      return -1;
    }
    for (size_t level = coarsest + 1; level-- > 0;) {
      cut = c.refine_level(level, mbw.data());
      if (cut < 0) {
        return -1;
      }
      if (c.fm_on && c.fm_level(level, mbw.data(), nullptr, &cut) != 0) {
        return -1;
      }
      if (level > 0 && c.project(level) != 0) {
        return -1;
      }
    }
  } else {
    // progressive k: block groups are bisected during uncoarsening, LP / Jet /
    // FM run under per-group caps (width x uniform cap; unopened ids get 0)
    std::vector<u32> group_lo(k, 0), group_w(k, 0);
    u32 num_groups = 1;
    group_w[0] = k;
    std::vector<i64> caps(k, 0);
    c.part.assign(c.sizes.back(), 0);
    for (size_t level = coarsest + 1; level-- > 0;) {
      // at the coarsest level split eagerly (down to ~32-vertex blocks);
      // afterwards extend only when every block keeps >= split_c vertices
      const u32 sc = (level == coarsest && !late_splits) ? std::min(o.split_c, 48u) : o.split_c;
      kmp_graph_t *hg_owned = nullptr;
      const kmp_graph_t *hg = nullptr;
      int rc = 0;
      if (num_groups < k &&
          (static_cast<u64>(c.sizes[level]) >= 2ull * sc * num_groups || level == 0)) {
        PhaseTimer t(c.st.extend_ns);
        rc = c.to_host(level);
        if (rc == 0) {
          hg_owned = level == 0 ? nullptr : kmp_lp_download_graph(c.engines[level]);
          hg = level == 0 ? g : hg_owned;
          rc = hg != nullptr ? 0 : -1;
        }
        if (rc == 0) {
          kmp_extend_partition(hg, c.part.data(), k, mbw_val, sc, o.ip_reps, level == 0 ? 1 : 0,
                               group_lo.data(), group_w.data(), &num_groups);
          if (num_groups == k) {
            kmp_balance_partition(hg, k, mbw_val, c.part.data());
          }
        }
      }
      if (rc == 0) {
        std::fill(caps.begin(), caps.end(), 0);
        for (u32 i = 0; i < num_groups; ++i) {
          caps[group_lo[i]] = static_cast<i64>(group_w[i]) * mbw_val;
        }
        if (o.resident) {
          rc = c.to_device(level);
        }
      }
      if (rc == 0) {
        cut = c.refine_level(level, caps.data());
        rc = cut < 0 ? -1 : 0;
      }
      if (rc == 0 && c.fm_on) {
        rc = c.fm_level(level, caps.data(), hg, &cut);
      }
      if (hg_owned != nullptr) {
        kmp_graph_free(hg_owned);
      }
      if (rc == 0 && level > 0) {
        rc = c.project(level);
      }
      if (rc != 0) {
        return -1;
      }
    }
  }

  // V-cycles on the result: cycle i with seed + i on the output of cycle
  // i - 1, on the level-0 engine; the coarse engines are freed first (every
  // cycle builds a chain of its own)
  if (o.vcycles > 0) {
    const auto cyc0 = std::chrono::steady_clock::now();
    for (size_t i = c.engines.size(); i-- > 1;) {
      kmp_lp_free(c.engines[i]);
      c.engines.pop_back();
    }
    std::vector<u32> cyc_sizes;
    for (int i = 0; i < o.vcycles; ++i) {
      const bool last = i == o.vcycles - 1;
      bool accepted = false;
      cut = vcycle_core(g, k, eps, seed + static_cast<u64>(i), o, c.engines[0], c.part, c.on_host,
                        last || !o.resident, c.st, cyc_sizes, &accepted);
      if (cut < 0) {
        return -1;
      }
      c.st.vcycles_run += 1;
      c.st.vcycles_accepted += accepted ? 1 : 0;
      c.st.vcycle_cuts[i] = cut;
    }
    c.st.vcycle_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                          std::chrono::steady_clock::now() - cyc0)
                                          .count());
  }

  if (c.to_host(0) != 0) {
    return -1;
  }
  std::memcpy(part_out, c.part.data(), sizeof(u32) * n);
  if (stats != nullptr) {
    c.st.num_levels = static_cast<u32>(c.sizes.size());
    std::copy(c.sizes.begin(), c.sizes.end(), c.st.level_sizes);
    std::copy(c.arcs.begin(), c.arcs.end(), c.st.level_arcs);
    c.st.label_traffic_bytes = kmp_lp_label_traffic_bytes() - traffic0;
    c.st.total_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                         std::chrono::steady_clock::now() - wall0)
                                         .count());
    *stats = c.st;
  }
  return cut;
}

} // namespace

extern "C" {

kmp_pipeline_opts_t kmp_pipeline_opts_default(void) {
  kmp_pipeline_opts_t o;
  std::memset(&o, 0, sizeof(o));
  o.iters = 5;
  o.jet_fine = kmp_jet_params_default(0);
  o.jet_coarse = kmp_jet_params_default(1);
  o.fm = -1;
  o.sparsify_params = kmp_sparsify_params_default();
  return o;
}

u32 kmp_pipeline_opts_size(void) { return sizeof(kmp_pipeline_opts_t); }
u32 kmp_pipeline_stats_size(void) { return sizeof(kmp_pipeline_stats_t); }

u32 kmp_pipeline_opts_layout(u32 *offsets_out, u32 cap) {
#define KMP_OFF(f) static_cast<u32>(offsetof(kmp_pipeline_opts_t, f))
  const u32 off[] = {KMP_OFF(iters),   KMP_OFF(contraction_limit), KMP_OFF(stop_n),
                     KMP_OFF(split_c), KMP_OFF(ip_reps),           KMP_OFF(jet),
                     KMP_OFF(jet_fine), KMP_OFF(jet_coarse),       KMP_OFF(fm),
                     KMP_OFF(resident), KMP_OFF(engine),           KMP_OFF(vcycles),
                     KMP_OFF(sparsify), KMP_OFF(sparsify_params)};
#undef KMP_OFF
  const u32 cnt = sizeof(off) / sizeof(off[0]);
  for (u32 i = 0; i < cnt && i < cap; ++i) {
    offsets_out[i] = off[i];
  }
  return cnt;
}

u32 kmp_pipeline_stats_layout(u32 *offsets_out, u32 cap) {
#define KMP_OFF(f) static_cast<u32>(offsetof(kmp_pipeline_stats_t, f))
  const u32 off[] = {KMP_OFF(num_levels),     KMP_OFF(level_sizes),
                     KMP_OFF(jet_iterations), KMP_OFF(jet_moves),
                     KMP_OFF(jet_balancer_calls), KMP_OFF(label_traffic_bytes),
                     KMP_OFF(cluster_ns),     KMP_OFF(contract_ns),
                     KMP_OFF(extend_ns),      KMP_OFF(refine_ns),
                     KMP_OFF(jet_ns),         KMP_OFF(fm_ns),
                     KMP_OFF(total_ns),       KMP_OFF(vcycles_run),
                     KMP_OFF(vcycles_accepted), KMP_OFF(vcycle_cuts),
                     KMP_OFF(vcycle_ns),      KMP_OFF(level_arcs),
                     KMP_OFF(sparsified_levels), KMP_OFF(sparsify_arcs_dropped),
                     KMP_OFF(sparsify_ns)};
#undef KMP_OFF
  const u32 cnt = sizeof(off) / sizeof(off[0]);
  for (u32 i = 0; i < cnt && i < cap; ++i) {
    offsets_out[i] = off[i];
  }
  return cnt;
}

i64 kmp_partition_ex(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, const kmp_pipeline_opts_t *opts,
    u32 *part_out, kmp_pipeline_stats_t *stats
) {
  return run_pipeline(g, k, eps, seed, opts, part_out, stats, false);
}

i64 kmp_partition_deep_ex(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, const kmp_pipeline_opts_t *opts,
    u32 *part_out, kmp_pipeline_stats_t *stats
) {
  return run_pipeline(g, k, eps, seed, opts, part_out, stats, true);
}

i64 kmp_vcycle_ex(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, const kmp_pipeline_opts_t *opts,
    u32 *part_inout, kmp_pipeline_stats_t *stats
) {
  const char *who = "kmp_vcycle_ex";
  kmp_pipeline_opts_t o = opts != nullptr ? *opts : kmp_pipeline_opts_default();
  if (check_opts(g, k, o, who) != 0) {
    return -1;
  }
  const u32 n = kmp_graph_n(g);
  if (part_inout == nullptr && (o.resident != 1 || o.engine == nullptr)) {
    fprintf(stderr, "kaminpar_amd: %s: part_inout == NULL needs resident = 1 and an engine\n",
            who);
    return -1;
  }
  for (u32 u = 0; part_inout != nullptr && u < n; ++u) {
    if (part_inout[u] >= k) {
      fprintf(stderr, "kaminpar_amd: %s: part_inout[%u] = %u is not below k = %u\n", who, u,
              part_inout[u], k);
      return -1;
    }
  }
  resolve_defaults(o, n);
  const auto wall0 = std::chrono::steady_clock::now();
  const u64 traffic0 = kmp_lp_label_traffic_bytes();
  kmp_lp_t *eng0 = o.engine != nullptr ? o.engine : kmp_lp_create(g);
  if (eng0 == nullptr) {
    return -1;
  }
  std::vector<u32> part;
  bool on_host = part_inout != nullptr;
  if (on_host) {
    part.assign(part_inout, part_inout + n);
  }
  kmp_pipeline_stats_t st{};
  std::vector<u32> sizes;
  bool accepted = false;
  const i64 cut =
      vcycle_core(g, k, eps, seed, o, eng0, part, on_host, part_inout != nullptr, st, sizes,
                  &accepted);
  if (eng0 != o.engine) {
    kmp_lp_free(eng0);
  }
  if (cut < 0) {
    return -1;
  }
  if (part_inout != nullptr) {
    std::memcpy(part_inout, part.data(), sizeof(u32) * n);
  }
  if (stats != nullptr) {
    st.num_levels = static_cast<u32>(sizes.size());
    std::copy(sizes.begin(), sizes.end(), st.level_sizes);
    st.label_traffic_bytes = kmp_lp_label_traffic_bytes() - traffic0;
    st.vcycles_run = 1;
    st.vcycles_accepted = accepted ? 1 : 0;
    st.vcycle_cuts[0] = cut;
    st.total_ns = static_cast<u64>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                       std::chrono::steady_clock::now() - wall0)
                                       .count());
    st.vcycle_ns = st.total_ns;
    *stats = st;
  }
  return cut;
}

i64 kmp_partition(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, int iters, u32 contraction_limit,
    u32 stop_n, int ip_reps, u32 *part_out
) {
  kmp_pipeline_opts_t o = kmp_pipeline_opts_default();
  o.iters = iters;
  o.contraction_limit = contraction_limit;
  o.stop_n = stop_n;
  o.ip_reps = ip_reps;
  return kmp_partition_ex(g, k, eps, seed, &o, part_out, nullptr);
}

i64 kmp_partition_deep(
    const kmp_graph_t *g, u32 k, double eps, u64 seed, int iters, u32 contraction_limit,
    u32 stop_n, u32 split_c, int ip_reps, u32 *part_out
) {
  kmp_pipeline_opts_t o = kmp_pipeline_opts_default();
  o.iters = iters;
  o.contraction_limit = contraction_limit;
  o.stop_n = stop_n;
  o.split_c = split_c;
  o.ip_reps = ip_reps;
  return kmp_partition_deep_ex(g, k, eps, seed, &o, part_out, nullptr);
}

// --------------------------- ckaminpar-shaped shim (see kaminpar_lp.h) ----

struct kaminpar_amd_t {
  kmp_graph_t *g = nullptr;
  u32 k = 2;
  double eps = 0.03;
  u64 seed = 1;
  bool jet_preset = false;   // kaminpar_amd_set_preset
  int vcycles = 0;           // kaminpar_amd_set_vcycles
  int sparsify = 0;          // kaminpar_amd_set_sparsification
  kmp_sparsify_params_t sparsify_params = kmp_sparsify_params_default();
  std::vector<i64> abs_maxw; // per-block max weights (kaminpar.h:961)
  std::vector<i64> minw;     // per-block min weights (kaminpar.h:965-968)
};

kaminpar_amd_t *kaminpar_amd_create(int /*num_threads*/) {
  return new kaminpar_amd_t();
}

void kaminpar_amd_free(kaminpar_amd_t *shm) {
  if (shm) {
    if (shm->g) {
      kmp_graph_free(shm->g);
    }
    delete shm;
  }
}

void kaminpar_amd_reseed(kaminpar_amd_t *shm, int seed) {
  shm->seed = static_cast<u64>(seed);
}

void kaminpar_amd_copy_graph(
    kaminpar_amd_t *shm, u32 n, const u32 *xadj, const u32 *adjncy,
    const i32 *vwgt, const i32 *adjwgt
) {
  if (shm->g) {
    kmp_graph_free(shm->g);
  }
  shm->g = kmp_graph_from_csr(n, xadj[n], xadj, adjncy, vwgt, adjwgt);
}

void kaminpar_amd_set_k(kaminpar_amd_t *shm, u32 k) { shm->k = k; }

void kaminpar_amd_set_uniform_max_block_weights(kaminpar_amd_t *shm, double epsilon) {
  shm->eps = epsilon;
  shm->abs_maxw.clear();
}

// kaminpar.h:961 set_absolute_max_block_weights: explicit per-block caps.
void kaminpar_amd_set_absolute_max_block_weights(
    kaminpar_amd_t *shm, const i64 *weights, u32 count
) {
  shm->abs_maxw.assign(weights, weights + count);
}

// kaminpar.h:965 set_uniform_min_block_weights: minimum block weights as a
// fraction of the perfectly balanced weight (context.cc:72-80); triggers the
// underload balancer after partitioning (the reference's refiner chain runs
// it only when minima are configured, presets.cc:332-338).
void kaminpar_amd_set_uniform_min_block_weights(kaminpar_amd_t *shm, double min_epsilon) {
  // marker encoding {-1, min_epsilon in ppb}; materialized at compute time
  // (the actual minima need k and the total node weight)
  shm->minw.assign(2, -1);
  shm->minw[1] = static_cast<i64>(min_epsilon * 1e9);
}

// kaminpar.h:966-967 absolute variant.
void kaminpar_amd_set_absolute_min_block_weights(
    kaminpar_amd_t *shm, const i64 *weights, u32 count
) {
  shm->minw.assign(weights, weights + count);
}

void kaminpar_amd_clear_min_block_weights(kaminpar_amd_t *shm) {
  shm->minw.clear();
}

int kaminpar_amd_set_preset(kaminpar_amd_t *shm, const char *name) {
  if (name != nullptr && std::strcmp(name, "default") == 0) {
    shm->jet_preset = false;
    return 0;
  }
  if (name != nullptr && std::strcmp(name, "jet") == 0) {
    shm->jet_preset = true;
    return 0;
  }
  return -1;
}

void kaminpar_amd_set_vcycles(kaminpar_amd_t *shm, int n) { shm->vcycles = n; }

void kaminpar_amd_set_sparsification(
    kaminpar_amd_t *shm, int on, const kmp_sparsify_params_t *params
) {
  shm->sparsify = on;
  shm->sparsify_params = params != nullptr ? *params : kmp_sparsify_params_default();
}

i64 kaminpar_amd_compute_partition(kaminpar_amd_t *shm, u32 *partition) {
  if (!shm->g) {
    fprintf(stderr, "kaminpar_amd: no graph set (call kaminpar_amd_copy_graph)\n");
    return -1;
  }
  const u32 k = shm->k;
  const i64 W = kmp_graph_total_node_weight(shm->g);
  double eps = shm->eps;
  std::vector<i64> caps;
  if (!shm->abs_maxw.empty()) {
    // pipeline under a uniform proxy derived from the average cap; exact
    // per-block enforcement happens below via balance + refine under the
    // true caps (both engine paths take per-block arrays)
    caps = shm->abs_maxw;
    caps.resize(k, caps.empty() ? 0 : caps.back());
    i64 cap_sum = 0;
    for (i64 c : caps) {
      cap_sum += c;
    }
    const double avg_cap = static_cast<double>(cap_sum) / k;
    eps = avg_cap * k / static_cast<double>(W) - 1.0;
    if (eps < 0.001) {
      eps = 0.001;
    }
  }
  // progressive-k (deep) pipeline: best measured cuts;
  // the "jet" preset adds Jet with the selection rebalancer at every level
  // (DESIGN.md sections 9 and 13)
  i64 cut;
  if (shm->jet_preset) {
    kmp_pipeline_opts_t o = kmp_pipeline_opts_default();
    o.jet = 1;
    o.jet_fine.balancer = KMP_JET_BALANCER_SELECT;
    o.jet_coarse.balancer = KMP_JET_BALANCER_SELECT;
    o.fm = -1;
    o.resident = 1;
    o.vcycles = shm->vcycles;
    o.sparsify = shm->sparsify;
    o.sparsify_params = shm->sparsify_params;
    cut = kmp_partition_deep_ex(shm->g, k, eps, shm->seed, &o, partition, nullptr);
  } else if (shm->vcycles != 0 || shm->sparsify != 0) {
    kmp_pipeline_opts_t o = kmp_pipeline_opts_default();
    o.vcycles = shm->vcycles;
    o.sparsify = shm->sparsify;
    o.sparsify_params = shm->sparsify_params;
    cut = kmp_partition_deep_ex(shm->g, k, eps, shm->seed, &o, partition, nullptr);
  } else {
    cut = kmp_partition_deep(shm->g, k, eps, shm->seed, 5, 0, 0, 0, 0, partition);
  }
  if (cut < 0) {
    return cut;
  }
  const bool want_min = !shm->minw.empty();
  if (!caps.empty() || want_min) {
    kmp_lp_t *e = kmp_lp_create(shm->g);
    if (!e) {
      return -1;
    }
    if (caps.empty()) {
      const i64 uni = kmp_max_block_weight(shm->g, k, shm->eps);
      caps.assign(k, uni);
    }
    if (!caps.empty() && !shm->abs_maxw.empty()) {
      // exact per-block caps: repair + refine under them
      cut = kmp_lp_balance(e, k, caps.data(), partition, shm->seed, 5, nullptr);
      if (cut >= 0) {
        cut = kmp_lp_refine(e, k, caps.data(), partition, shm->seed, 5, nullptr);
      }
    }
    if (cut >= 0 && want_min) {
      std::vector<i64> minw = shm->minw;
      if (minw.size() == 2 && minw[0] == -1) {
        // uniform min epsilon (ppb-encoded): ceil((1-eps_min) * W/k)
        const double me = static_cast<double>(minw[1]) / 1e9;
        const i64 v = static_cast<i64>(
            std::ceil((1.0 - me) * static_cast<double>(W) / k));
        minw.assign(k, v);
      } else {
        minw.resize(k, 0);
      }
      cut = kmp_lp_underload(e, k, caps.data(), minw.data(), partition, shm->seed, 5, nullptr);
    }
    kmp_lp_free(e);
  }
  return cut;
}

} // extern "C"
