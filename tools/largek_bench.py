"""Measurements for LP refinement / balancing above k = 2048 (the hash gain
tiers). R-MAT edge factor 8, seed 42; every mode prints JSON and writes it to
--out (by default under profiles/largek/).

  refine    5 sweeps from random_partition(seed=3) at eps 0.03, for every k
            of --ks in one process on one engine. k = 2048 runs the dense
            legacy path and is the yardstick (same commit machinery). Per k:
            one warm-up, then --reps timed repetitions of reset + run_sweeps;
            the device-synced wall clock per repetition (all listed, best and
            median reported), the call's own HIP-event times (phase A, commit
            region), ms per sweep, arcs/s, and the ratio to k = 2048.
            Per-kernel times come from a separate run of this mode under
            `rocprofv3 --kernel-trace --stats` with nothing else collected.
  balance   kmp_lp_balance from random_partition under caps of eps 0 (so
            that blocks are over their caps): wall time and the host time of
            the isolated-vertex pre-pass and of the per-chunk fallback scans.
  deep      cut, seconds and feasibility of partition_deep at every k of
            --ks, each in a child process of its own after a warm-up at
            k = 16. A child that runs past --limit seconds is stopped and
            reported as such, and so is one that fails; either ends the run.
  kstats    turn the `*_kernel_stats.csv` of a `rocprofv3 --kernel-trace
            --stats -f csv` run into a per-kernel JSON summary (--csv, --out).

Usage (GPU box):
  python tools/largek_bench.py refine --scale 20 --ks 2048 4096 65536 1048576
  python tools/largek_bench.py balance --scale 20 --ks 65536
  python tools/largek_bench.py deep --scale 20 --ks 4096 65536
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWEEPS = 5
EPS = 0.03


def run_refine(a):
    import kaminpar_amd as ka

    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)
    rows = {}
    for k in a.ks:
        part0 = ka.random_partition(g.n, k, seed=3)
        mbw = np.full(k, g.max_block_weight(k, EPS), dtype=np.int64)
        eng.refine_begin(k, mbw, part0, seed=1)
        reps = []
        for rep in range(a.reps + 1):  # the first repetition is the warm-up
            eng.reset()
            t0 = time.perf_counter()
            moves = eng.run_sweeps(SWEEPS)  # returns device-synced
            wall = time.perf_counter() - t0
            st = eng.get_stats()
            if rep:
                reps.append({"wall_ms": round(wall * 1e3, 3),
                             "phase_a_ms": round(st.phase_a_ns / 1e6, 3),
                             "commit_ms": round(st.total_ns / 1e6, 3)})
        walls = [r["wall_ms"] for r in reps]
        best = min(reps, key=lambda r: r["wall_ms"])
        rows[str(k)] = {
            "path": "dense" if k <= 2048 else "hash",
            "moves": moves, "arcs_scanned": int(st.arcs_scanned),
            "wall_ms_all_reps": walls,
            "wall_ms_best": best["wall_ms"],
            "wall_ms_median": round(statistics.median(walls), 3),
            "phase_a_ms_best_rep": best["phase_a_ms"],
            "commit_ms_best_rep": best["commit_ms"],
            # run_sweeps stops after a sweep without moves
            "sweeps_run": 1 if moves == 0 else SWEEPS,
            "ms_per_sweep": round(best["wall_ms"] / (1 if moves == 0 else SWEEPS), 3),
            "arcs_per_s": round(st.arcs_scanned / best["wall_ms"] * 1e3),
        }
        print(f"k={k}: {rows[str(k)]}", flush=True)
        eng.refine_end()
    base = rows.get("2048")
    if base:
        for r in rows.values():
            r["ratio_to_k2048"] = round(r["ms_per_sweep"] / base["ms_per_sweep"], 3)
    return {"mode": "refine", "graph": f"rmat{a.scale}_s42", "n": int(g.n), "m": int(g.m),
            "sweeps": SWEEPS, "eps": EPS, "partition": "random_partition(seed=3)",
            "reps": a.reps, "k": rows}


def run_balance(a):
    import kaminpar_amd as ka

    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)
    deg = np.diff(np.asarray(g.xadj, dtype=np.int64))
    rows = {}
    for k in a.ks:
        part0 = ka.random_partition(g.n, k, seed=3)
        mbw = np.full(k, g.max_block_weight(k, 0.0), dtype=np.int64)
        over0 = int((np.bincount(part0, minlength=k) > mbw).sum())
        reps = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            cut, part, st = eng.balance(k, mbw, part0, seed=1, iters=SWEEPS)
            wall = time.perf_counter() - t0
            pre_ns, scan_ns = eng.balance_host_ns()
            if rep:
                reps.append({"wall_ms": round(wall * 1e3, 3),
                             "host_prepass_ms": round(pre_ns / 1e6, 3),
                             "host_fallback_scans_ms": round(scan_ns / 1e6, 3)})
        best = min(reps, key=lambda r: r["wall_ms"])
        rows[str(k)] = dict(best, wall_ms_all_reps=[r["wall_ms"] for r in reps],
                            cut=int(cut), moves=int(st.moves),
                            blocks_over_cap_before=over0,
                            blocks_over_cap_after=int(
                                (np.bincount(part, minlength=k) > mbw).sum()))
        print(f"k={k}: {rows[str(k)]}", flush=True)
    return {"mode": "balance", "graph": f"rmat{a.scale}_s42", "n": int(g.n), "m": int(g.m),
            "isolated_vertices": int((deg == 0).sum()), "sweeps": SWEEPS,
            "caps": "max_block_weight(k, 0.0)", "partition": "random_partition(seed=3)",
            "k": rows}


def run_one(a):
    import kaminpar_amd as ka
    from kaminpar_amd.partition import partition_deep

    k = a.ks[0]
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)  # the fine CSR stays resident
    partition_deep(g, 16, seed=1, engine=eng)  # warm-up
    t0 = time.perf_counter()
    cut, part, sizes = partition_deep(g, k, seed=1, engine=eng)
    dt = time.perf_counter() - t0
    w = np.bincount(part, minlength=k)
    return {"cut": int(cut), "seconds": round(dt, 3), "levels": [int(s) for s in sizes],
            "feasible": bool(w.max() <= g.max_block_weight(k, EPS)),
            "heaviest_block": int(w.max()), "cap": int(g.max_block_weight(k, EPS)),
            "blocks_used": int((w > 0).sum())}


def run_deep(a):
    out = {"mode": "deep", "graph": f"rmat{a.scale}_s42", "eps": EPS,
           "limit_seconds": a.limit, "k": {}}
    for k in a.ks:
        cmd = [sys.executable, os.path.abspath(__file__), "one", "--scale", str(a.scale),
               "--ks", str(k)]
        t0 = time.perf_counter()
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            # stopped at its limit: it may hang the GPU, so start nothing more
            out["k"][str(k)] = {"stopped_after_seconds": a.limit}
            print(f"k={k}: stopped after {a.limit} s; ending the run", flush=True)
            break
        if res.returncode != 0:
            # a child that died may have faulted the GPU: start nothing more
            out["k"][str(k)] = {"failed": res.returncode, "stderr": res.stderr[-2000:]}
            print(f"k={k}: failed ({res.returncode})\n{res.stderr[-2000:]}", flush=True)
            break
        row = json.loads(res.stdout.strip().splitlines()[-1])
        row["child_seconds"] = round(time.perf_counter() - t0, 1)
        out["k"][str(k)] = row
        print(f"k={k}: {row}", flush=True)
    return out


def run_kstats(a):
    import csv
    import re

    rows = list(csv.DictReader(open(a.csv)))
    total = sum(int(r["TotalDurationNs"]) for r in rows)
    kernels = []
    for r in rows:
        name = r["Name"].replace("(anonymous namespace)::", "")
        m = re.search(r"wrapped_(\w+?)_config", name)
        if "rocprim" in name and m:
            short = "rocprim:" + m.group(1)
        else:
            short = re.sub(r"^void ", "", name).split("(")[0]
        kernels.append({"kernel": short, "calls": int(r["Calls"]),
                        "total_ms": round(int(r["TotalDurationNs"]) / 1e6, 3),
                        "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                        "percent": float(r["Percentage"])})
    return {"mode": "kstats", "source": "rocprofv3 --kernel-trace --stats -f csv",
            "note": a.note, "total_kernel_ms": round(total / 1e6, 3), "kernels": kernels}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["refine", "balance", "deep", "one", "kstats"])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ks", type=int, nargs="+", default=[2048, 4096, 65536, 1 << 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--csv", help="kstats: the *_kernel_stats.csv to summarize")
    ap.add_argument("--note", default="", help="kstats: what was traced")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"refine": run_refine, "balance": run_balance, "deep": run_deep,
           "one": run_one, "kstats": run_kstats}[a.mode](a)
    if a.mode == "kstats":
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        return
    print(json.dumps(out))
    if a.mode != "one":
        path = a.out or os.path.join(REPO, "profiles", "largek",
                                     f"{a.mode}_rmat{a.scale}.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
