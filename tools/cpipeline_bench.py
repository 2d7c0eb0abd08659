"""The C pipeline drivers against the Python drivers, configuration by
configuration (kmp_partition_deep_ex through Graph.partition_deep_native, and
kaminpar_amd.partition.partition_deep).

R-MAT scale S (edge factor 8, seed 42), k blocks, eps 0.03, seed 1. The
configurations are {LP, jet b2 (balancer=0, balance_iters=2), jet sel
(balancer=1)} x {Python driver, C driver} x {resident off, on}. Every one runs
in a child process of its own, under a time limit: the child generates the
graph, creates one engine for the fine graph (passed to the driver as
`engine`, so neither driver pays for it inside the timed call), runs the
configuration once as a warm-up and then --reps timed repetitions. A host
clock around the call (which ends synchronised) gives the time; the delta of
label_traffic_bytes() around the call gives the label bytes that crossed PCIe.
The first child that fails or runs out of time ends the run.

The parent asserts that the C and the Python driver of one configuration
report equal cuts, level sizes, partition checksums and label bytes, and
writes per configuration the times, their median and spread (max - min), and
per pair the C driver's median over the Python driver's. The yardstick for a C
time is the Python driver of the same configuration in the same run.

Usage (GPU box):
  python tools/cpipeline_bench.py --scale 23 --k 16 --out p23.json
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REFINERS = {
    "lp": False,
    "jet_b2": dict(balancer=0, balance_iters=2),
    "jet_sel": dict(balancer=1),
}
DRIVERS = ("py", "c")


def config_names():
    return [f"{ref}_{drv}_{'resident' if res else 'host'}"
            for ref in REFINERS for res in (False, True) for drv in DRIVERS]


def run_child(a):
    import numpy as np

    import kaminpar_amd as ka
    from kaminpar_amd.partition import partition_deep

    ref, drv, where = a.child.rsplit("_", 2)
    jet, resident = REFINERS[ref], where == "resident"
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)  # fine CSR stays resident

    def call():
        b0 = ka.label_traffic_bytes()
        t0 = time.perf_counter()
        if drv == "c":
            cut, part, st = g.partition_deep_native(
                a.k, seed=1, jet=jet, resident=resident, engine=eng, return_stats=True)
            sizes = st.levels
            phases = {q[0][:-3]: round(getattr(st, q[0]) / 1e9, 4)
                      for q in st._fields_ if q[0].endswith("_ns")}
        else:
            cut, part, sizes = partition_deep(
                g, a.k, seed=1, jet=jet, resident=resident, engine=eng)
            phases = None
        dt = time.perf_counter() - t0
        checksum = int(np.bitwise_xor.reduce(
            np.asarray(part, np.uint64) * np.arange(1, g.n + 1, dtype=np.uint64)))
        return dict(cut=int(cut), sizes=[int(s) for s in sizes], seconds=dt,
                    label_bytes=ka.label_traffic_bytes() - b0, checksum=checksum,
                    phases=phases)

    first = call()  # warm-up
    times = []
    for _ in range(a.reps):
        r = call()
        for q in ("cut", "sizes", "label_bytes", "checksum"):
            assert r[q] == first[q], q
        times.append(round(r["seconds"], 4))
    print(json.dumps({
        "n": int(g.n), "m": int(g.m), "cut": first["cut"], "levels": first["sizes"],
        "part_checksum": first["checksum"], "label_bytes_per_call": int(first["label_bytes"]),
        "seconds": times, "median_seconds": round(statistics.median(times), 4),
        "spread_seconds": round(max(times) - min(times), 4),
        "warmup_seconds": round(first["seconds"], 4), "phase_seconds_last": r["phases"]}))


def run_parent(a):
    out = {"graph": f"rmat{a.scale}_s42", "k": a.k, "eps": 0.03, "seed": 1, "reps": a.reps,
           "driver": "partition_deep / kmp_partition_deep_ex", "configs": {}}
    refiners = a.refiners.split(",")
    wheres = a.labels.split(",")
    names = [n for n in config_names()
             if n.rsplit("_", 2)[0] in refiners and n.rsplit("_", 2)[2] in wheres]
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--scale",
               str(a.scale), "--k", str(a.k), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {a.step_timeout} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{name}: exit status {r.returncode}; stopping")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        out["n"], out["m"] = row.pop("n"), row.pop("m")
        out["configs"][name] = row
        print(f"{name}: cut {row['cut']} median {row['median_seconds']} s "
              f"spread {row['spread_seconds']} s", flush=True)
    out["levels"] = out["configs"][names[0]]["levels"]
    out["c_over_py"] = {}
    for ref in refiners:
        for where in wheres:
            py = out["configs"][f"{ref}_py_{where}"]
            c = out["configs"][f"{ref}_c_{where}"]
            for q in ("cut", "levels", "part_checksum", "label_bytes_per_call"):
                assert py[q] == c[q], (ref, where, q, py[q], c[q])
            out["c_over_py"][f"{ref}_{where}"] = {
                "ratio": round(c["median_seconds"] / py["median_seconds"], 4),
                "c_minus_py_seconds": round(c["median_seconds"] - py["median_seconds"], 4),
                "larger_spread_seconds": max(c["spread_seconds"], py["spread_seconds"])}
    for row in out["configs"].values():
        del row["levels"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=240.0,
                    help="time limit of one configuration's child process, seconds")
    ap.add_argument("--refiners", default=",".join(REFINERS),
                    help="comma-separated subset of " + ",".join(REFINERS))
    ap.add_argument("--labels", default="host,resident",
                    help="comma-separated subset of host,resident")
    ap.add_argument("--child", choices=config_names(), help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("needs at least three timed repetitions")
    if a.child:
        run_child(a)
        return
    out = run_parent(a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
