"""Measurements for the GPU block subgraph extraction
(kmp_lp_extract_subgraphs / LpEngine.extract_subgraphs) and the drivers on it.

Two modes, each printing JSON and optionally writing it to --out:

  kernels   R-MAT scale S, k blocks, seeded random partition: the count and
            the fill pass timed by the call's own HIP events, the whole call by
            its device-synced wall clock; best of `--reps` after a warm-up,
            all repetitions listed. G arcs/s per pass is m over the pass time
            (each pass reads every arc once; arcs_scanned == 2 m is checked),
            next to the recorded rate of Jet's find at the same scale
            (profiles/jet/kernel_stats_rmat*_k16.json):
            the count pass does the same work per arc, one adjncy read and
            one label gather. A yardstick, not a threshold.
  pipeline  cut and seconds of partition_deep on R-MAT scale S with gpu_split
            False / True, in the default split schedule and with
            split_c >= n (every split on the finest level), each with LP only
            and with jet=dict(balancer=1). Every configuration runs in a
            child process of its own after one warm-up run of the default
            path. A child that runs past --limit seconds is stopped and
            reported as such, and so is a child that fails; either ends the
            whole run, since nothing more may start on a GPU that has just
            hung or faulted (--configs selects what a later run covers). The
            host run with split_c >= n is not run: it
            is quoted from profiles/round1/quality_rmat23_k16_late_full.json
            (5502 s of host bisection for a cut of 15.80M at scale 23).

Usage (GPU box):
  python tools/extract_bench.py kernels --scale 20 --k 16 --out e20.json
  python tools/extract_bench.py pipeline --scale 23 --k 16 --out p23.json
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# find kernels per pass, R-MAT edge factor 8, seed 42, k = 16
JET_FIND_MS = {20: 0.21, 23: 1.40}
QUOTED_HOST_LATE_FULL = {
    "source": "profiles/round1/quality_rmat23_k16_late_full.json",
    "cut": 15.80e6, "host_bisection_seconds": 5502, "rerun": False}


def run_kernels(a):
    import kaminpar_amd as ka

    g = ka.Graph.rmat(a.scale, 8, seed=42)
    part = ka.random_partition(g.n, a.k, seed=3)
    eng = ka.LpEngine(g)
    rows = []
    for _ in range(a.reps + 1):  # first repetition is the warm-up
        t0 = time.perf_counter()
        subs = eng.extract_subgraphs(a.k, part)
        wall = time.perf_counter() - t0
        st = subs.stats
        assert st.arcs_scanned == 2 * g.m
        rows.append({
            "count_ms": round(st.count_ns / 1e6, 3), "fill_ms": round(st.fill_ns / 1e6, 3),
            "total_ms": round(st.total_ns / 1e6, 3), "host_wall_ms": round(wall * 1e3, 3),
            "count_arcs_per_s": round(g.m / max(st.count_ns, 1) * 1e9),
            "fill_arcs_per_s": round(g.m / max(st.fill_ns, 1) * 1e9),
            "internal_arcs": int(subs.arc_offsets[-1])})
        del subs
    best = min(rows[1:], key=lambda r: r["total_ms"])
    best["total_ms_all_reps"] = [r["total_ms"] for r in rows[1:]]
    best["count_ms_all_reps"] = [r["count_ms"] for r in rows[1:]]
    best["fill_ms_all_reps"] = [r["fill_ms"] for r in rows[1:]]
    out = {"mode": "kernels", "graph": f"rmat{a.scale}_s42", "n": int(g.n), "m": int(g.m),
           "k": a.k, "partition": "random_partition(seed=3)", "extract": best}
    if a.scale in JET_FIND_MS:
        ms = JET_FIND_MS[a.scale]
        out["jet_find_recorded"] = {"ms_per_pass": ms,
                                    "arcs_per_s": round(g.m / ms * 1e3)}
    return out


CONFIGS = {
    # name: (gpu_split, late_full, jet)
    "host_default_lp": (False, False, False),
    "gpu_default_lp": (True, False, False),
    "gpu_latefull_lp": (True, True, False),
    "host_default_jet": (False, False, True),
    "gpu_default_jet": (True, False, True),
    "gpu_latefull_jet": (True, True, True),
}


def run_one(a):
    import kaminpar_amd as ka
    from kaminpar_amd.partition import partition_deep

    gpu_split, late_full, jet = CONFIGS[a.config]
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)  # fine CSR stays resident
    partition_deep(g, a.k, seed=1, engine=eng)  # warm-up: the default path
    kw = dict(gpu_split=gpu_split, jet=dict(balancer=1) if jet else False)
    if late_full:
        kw["split_c"] = g.n
    t0 = time.perf_counter()
    cut, part, sizes = partition_deep(g, a.k, seed=1, engine=eng, **kw)
    dt = time.perf_counter() - t0
    cap = g.max_block_weight(a.k, 0.03)
    return {"cut": int(cut), "seconds": round(dt, 3), "levels": [int(s) for s in sizes],
            "feasible": bool(np.bincount(part, minlength=a.k).max() <= cap)}


def run_pipeline(a):
    out = {"mode": "pipeline", "graph": f"rmat{a.scale}_s42", "k": a.k, "eps": 0.03,
           "limit_seconds": a.limit, "host_latefull_lp": dict(QUOTED_HOST_LATE_FULL),
           "host_latefull_jet": {"rerun": False,
                                 "note": "same host bisection as host_latefull_lp"},
           "configs": {}}
    for name in a.configs or list(CONFIGS):
        cmd = [sys.executable, os.path.abspath(__file__), "one", "--config", name,
               "--scale", str(a.scale), "--k", str(a.k)]
        t0 = time.perf_counter()
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            # stopped at its limit: it may hang the GPU, so start nothing more
            out["configs"][name] = {"stopped_after_seconds": a.limit}
            print(f"{name}: stopped after {a.limit} s; ending the run", flush=True)
            break
        if res.returncode != 0:
            # a child that died may have faulted the GPU: start nothing more
            out["configs"][name] = {"failed": res.returncode, "stderr": res.stderr[-2000:]}
            print(f"{name}: failed ({res.returncode})\n{res.stderr[-2000:]}", flush=True)
            break
        row = json.loads(res.stdout.strip().splitlines()[-1])
        row["child_seconds"] = round(time.perf_counter() - t0, 1)
        out["configs"][name] = row
        print(f"{name}: {row}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["kernels", "pipeline", "one"])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=180)
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--configs", nargs="+", choices=sorted(CONFIGS))
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"kernels": run_kernels, "pipeline": run_pipeline, "one": run_one}[a.mode](a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
