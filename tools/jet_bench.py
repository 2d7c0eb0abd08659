"""Measurements for the GPU Jet refiner (kmp_lp_jet / LpEngine.jet).

Three modes, each printing JSON and optionally writing it to --out:

  kernels   R-MAT scale S, k blocks: 5 LP refine sweeps from a seeded random
            partition (their phase-A arcs/s is the yardstick find is compared
            with), then `--iterations` Jet iterations from that result, timed
            by the call's own HIP events (find + filter) and its device-synced
            wall clock. The per-kernel split (find / filter / cut / balance
            sweeps) comes from a separate rocprofv3 --kernel-trace run of
            `--load-start`, summarized with tools/rocpd_summarize.py.
  pipeline  cut and wall time of partition() and partition_deep() with
            jet=False, jet=True and jet=True without the CPU FM, for every
            golden pipeline case or one R-MAT scale, and balance_iters 1/2/5.
  rebalance LpEngine.rebalance (kmp_lp_rebalance) alone on R-MAT scale S from a
            skewed start: random, every third vertex forced into block 0.

`--balancer 0 1` on kernels and pipeline runs Jet with the LP balance sweeps
(one configuration per --balance-iters value) and with the selection
rebalancer; in kernels mode the configurations alternate within every
repetition, so they see the same machine state.

Usage (GPU box):
  python tools/jet_bench.py kernels --scale 20 --k 16 --out j.json
  python tools/jet_bench.py pipeline --goldens --out p.json
  python tools/jet_bench.py pipeline --scale 23 --k 16 --out p23.json
  python tools/jet_bench.py kernels --scale 23 --balancer 0 1 --balance-iters 1 2
  python tools/jet_bench.py rebalance --scale 23 --k 16 --out r23.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import kaminpar_amd as ka  # noqa: E402
from kaminpar_amd.partition import partition, partition_deep  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")


def jet_row(st, wall):
    it = max(1, int(st.iterations))
    ff = st.find_filter_ns / 1e6
    return {
        "iterations": int(st.iterations),
        "balancer_calls": int(st.balancer_calls),
        "jet_moves": int(st.jet_moves),
        "balancer_moves": int(st.balancer_moves),
        "arcs_scanned": int(st.arcs_scanned),
        "find_filter_ms": round(ff, 3),
        "find_filter_ms_per_iteration": round(ff / it, 3),
        "total_ms": round(st.total_ns / 1e6, 3),
        "total_ms_per_iteration": round(st.total_ns / 1e6 / it, 3),
        "host_wall_ms": round(wall * 1e3, 3),
        "find_filter_arcs_per_s": round(st.arcs_scanned / max(ff, 1e-9) * 1e3),
        "balancer_ms": round(st.balancer_ns / 1e6, 3),
        "balancer_ms_per_iteration": round(st.balancer_ns / 1e6 / it, 3),
        "balancer_ms_per_call": round(st.balancer_ns / 1e6 / max(1, int(st.balancer_calls)), 3),
        "balancer_passes": int(st.balancer_passes),
        "feasible_iterations": int(st.feasible_iterations),
        "cut": int(st.edge_cut),
    }


def jet_configs(a):
    """(name, jet parameters) per requested balancer configuration."""
    configs = []
    if 0 in a.balancer:
        configs += [(f"balance_iters_{bi}", dict(balancer=0, balance_iters=bi))
                    for bi in a.balance_iters]
    if 1 in a.balancer:
        configs.append((f"select_passes_{a.balance_passes}",
                        dict(balancer=1, balance_passes=a.balance_passes)))
    return configs


def run_kernels(a):
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    k = a.k
    mbw = np.full(k, g.max_block_weight(k, a.eps), dtype=np.int64)
    eng = ka.LpEngine(g)
    out = {"mode": "kernels", "graph": f"rmat{a.scale}_s42", "n": int(g.n), "m": int(g.m),
           "k": k, "eps": a.eps, "temp": a.temp, "max_iterations": a.iterations}
    if a.load_start:
        part0 = np.load(a.load_start)
    else:
        lp = None
        for _ in range(2):  # first call warms code objects and allocations
            lp_cut, part0, lp = eng.refine(k, mbw, ka.random_partition(g.n, k, seed=3),
                                           seed=1, iters=5)
        out["lp_refine"] = {
            "cut": int(lp_cut), "arcs_scanned": int(lp.arcs_scanned),
            "phase_a_ms": round(lp.phase_a_ns / 1e6, 3),
            "phase_a_arcs_per_s": round(lp.arcs_scanned / max(lp.phase_a_ns, 1) * 1e9),
        }
        if a.save_start:
            np.save(a.save_start, part0)
    out["jet"] = {}
    configs = jet_configs(a)
    rows = {name: [] for name, _ in configs}
    feasible = {}
    for _ in range(a.reps + 1):  # first repetition is the warm-up
        for name, kw in configs:  # alternate: every configuration sees the same state
            t0 = time.perf_counter()
            cut, part, st = eng.jet(
                k, mbw, part0, seed=1, num_rounds=1, max_iterations=a.iterations,
                max_fruitless=0, fruitless_threshold=0.999, initial_gain_temp=a.temp,
                final_gain_temp=a.temp, **kw)
            rows[name].append(jet_row(st, time.perf_counter() - t0))
            feasible[name] = bool((np.bincount(part, minlength=k) <= mbw).all())  # unit weights
    for name, _ in configs:
        assert all(r["cut"] == rows[name][0]["cut"] for r in rows[name])
        best = min(rows[name][1:], key=lambda r: r["total_ms"])
        best["feasible"] = feasible[name]
        best["total_ms_all_reps"] = [r["total_ms"] for r in rows[name][1:]]
        out["jet"][name] = best
    return out


def golden_cases():
    exp = json.load(open(os.path.join(GOLDEN, "pipeline_expected.json")))
    for name, case in exp.items():
        if name.startswith("walshaw"):
            d = json.load(open(os.path.join(GOLDEN, "walshaw_data.json")))
            g = ka.Graph.from_csr(np.array(d["xadj"], np.uint32),
                                  np.array(d["adjncy"], np.uint32))
        elif name.startswith("rgg2d"):
            g = ka.Graph.read_metis(os.path.join(GOLDEN, "rgg2d.metis"))
        else:
            g = ka.Graph.rmat(int(name.split("_")[0][4:]), 8, 42)
        yield name, g, case["k"]


def run_pipeline(a):
    cases = golden_cases() if a.goldens else [
        (f"rmat{a.scale}_s42_k{a.k}", ka.Graph.rmat(a.scale, 8, seed=42), a.k)]
    out = {"mode": "pipeline", "eps": 0.03, "cases": {}}
    drivers = [("partition_deep", partition_deep)]
    if not a.deep_only:
        drivers.append(("partition", partition))
    for name, g, k in cases:
        cap = g.max_block_weight(k, 0.03)
        row = {"n": int(g.n), "m": int(g.m), "k": k,
               "fm_default_on": bool(g.n <= (1 << 21))}
        for dname, fn in drivers:
            eng = ka.LpEngine(g)  # fine CSR stays resident across configurations
            fn(g, k, seed=1, engine=eng)  # warm-up
            configs = [("lp", dict(jet=False))]
            for jname, jkw in jet_configs(a):
                cname = jname.replace("balance_iters_", "jet_b").replace("select_passes_",
                                                                         "jet_select_p")
                configs.append((cname, dict(jet=jkw)))
                if row["fm_default_on"]:
                    configs.append((f"{cname}_nofm", dict(jet=jkw, fm=False)))
            if row["fm_default_on"]:
                configs.append(("lp_nofm", dict(jet=False, fm=False)))
            res = {}
            for cname, kw in configs:
                t0 = time.perf_counter()
                cut, part, _ = fn(g, k, seed=1, engine=eng, **kw)
                dt = time.perf_counter() - t0
                res[cname] = {"cut": int(cut), "seconds": round(dt, 3),
                              "feasible": bool(np.bincount(part, minlength=k).max() <= cap)
                              if g.total_node_weight == g.n else None}
                print(f"{name} {dname} {cname}: {res[cname]}", flush=True)
            row[dname] = res
        out["cases"][name] = row
    return out


def run_rebalance(a):
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    k = a.k
    mbw = np.full(k, g.max_block_weight(k, a.eps), dtype=np.int64)
    part0 = ka.random_partition(g.n, k, seed=3)
    part0[::3] = 0
    eng = ka.LpEngine(g)
    out = {"mode": "rebalance", "graph": f"rmat{a.scale}_s42", "n": int(g.n), "m": int(g.m),
           "k": k, "eps": a.eps, "max_passes": a.balance_passes,
           "start": "random, every third vertex in block 0",
           "start_overload": int(np.maximum(np.bincount(part0, minlength=k) - mbw, 0).sum())}
    rows = []
    for _ in range(a.reps + 1):  # first repetition is the warm-up
        t0 = time.perf_counter()
        cut, part, st = eng.rebalance(k, mbw, part0, max_passes=a.balance_passes)
        wall = time.perf_counter() - t0
        rows.append({
            "passes": int(st.passes), "selected": int(st.selected), "moves": int(st.moves),
            "arcs_scanned": int(st.arcs_scanned), "score_ms": round(st.score_ns / 1e6, 3),
            "score_ms_per_pass": round(st.score_ns / 1e6 / max(1, int(st.passes)), 3),
            "total_ms": round(st.total_ns / 1e6, 3), "host_wall_ms": round(wall * 1e3, 3),
            "feasible": bool(st.feasible), "cut": int(cut)})
    assert all(r["cut"] == rows[0]["cut"] and r["moves"] == rows[0]["moves"] for r in rows)
    best = min(rows[1:], key=lambda r: r["total_ms"])
    best["total_ms_all_reps"] = [r["total_ms"] for r in rows[1:]]
    out["rebalance"] = best
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["kernels", "pipeline", "rebalance"])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--eps", type=float, default=0.03)
    ap.add_argument("--temp", type=float, default=0.25)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--balance-iters", type=int, nargs="+", default=[1])
    ap.add_argument("--balancer", type=int, nargs="+", choices=[0, 1], default=[0])
    ap.add_argument("--balance-passes", type=int, default=16)
    ap.add_argument("--goldens", action="store_true")
    ap.add_argument("--deep-only", action="store_true")
    ap.add_argument("--save-start")
    ap.add_argument("--load-start")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"kernels": run_kernels, "pipeline": run_pipeline, "rebalance": run_rebalance}[a.mode](a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
