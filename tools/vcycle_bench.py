"""What a V-cycle costs and gains on top of the multilevel drivers.

R-MAT scale S (edge factor 8, seed 42), k blocks, eps 0.03, seed 1, resident
labels. The configurations are {Python, C} x {partition, partition_deep} x
{LP, jet sel (balancer=1)}. Every one runs in a child process of its own, under
a time limit (protocol of tools/cpipeline_bench.py): the child generates the
graph, creates one engine for the fine graph and reuses it, runs the whole
sequence once as a warm-up and then --reps timed repetitions. The sequence is
the driver without cycles (the 0-cycle figure every other figure is compared
with), then --cycles stand-alone cycles, cycle c with seed 1 + c on the output
of cycle c - 1 -- what the drivers' `vcycles` option runs (tests/
test_vcycle_gpu.py pins the two to each other), taken apart so that every
cycle has a cut, a time, label bytes and, for the C driver, the phase times of
kmp_pipeline_stats_t of its own. Each cycle gets its input as a host array and
returns one, so its label bytes include one upload and one download. With
--with-option the sequence ends with the driver called once with
vcycles=CYCLES, which keeps the partition on the device between the cycles:
its time and label bytes are those of the option itself, and its result must
equal the stand-alone cycles'. Phase times are medians over the repetitions,
phase by phase.

The parent asserts that the C and the Python driver of one configuration
report equal cuts and partition checksums, and writes per configuration the
cut after every stage, the median and spread (max - min) of every stage's
seconds and the label bytes. The first child that fails or runs out of time
ends the run.

Usage (GPU box):
  python tools/vcycle_bench.py --scale 20 --k 16 --out v20.json
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

REFINERS = {"lp": False, "jet_sel": dict(balancer=1)}
PIPELINES = ("basic", "deep")
DRIVERS = ("py", "c")


def config_names():
    return [f"{pipe}_{ref}_{drv}" for pipe in PIPELINES for ref in REFINERS for drv in DRIVERS]


def split_name(name):
    pipe, rest = name.split("_", 1)
    ref, drv = rest.rsplit("_", 1)
    return pipe, ref, drv


def run_child(a):
    import numpy as np

    import kaminpar_amd as ka
    from kaminpar_amd.partition import partition, partition_deep, vcycle

    pipe, ref, drv = split_name(a.child)
    jet, deep = REFINERS[ref], pipe == "deep"
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)  # fine CSR stays resident

    def phases_of(st):
        return {q[0][:-3]: round(getattr(st, q[0]) / 1e9, 4)
                for q in st._fields_ if q[0].endswith("_ns")}

    def stage(fn):
        b0 = ka.label_traffic_bytes()
        t0 = time.perf_counter()
        cut, part, extra = fn()
        dt = time.perf_counter() - t0
        return dict(cut=int(cut), seconds=dt, label_bytes=ka.label_traffic_bytes() - b0,
                    **extra), part

    def driver(vcycles=0):
        if drv == "c":
            nat = g.partition_deep_native if deep else g.partition_native
            cut, part, st = nat(a.k, seed=1, jet=jet, resident=True, engine=eng,
                                return_stats=True, vcycles=vcycles)
            return cut, part, dict(levels=st.levels, phases=phases_of(st))
        cut, part, sizes = (partition_deep if deep else partition)(
            g, a.k, seed=1, jet=jet, resident=True, engine=eng, vcycles=vcycles)
        return cut, part, dict(levels=[int(s) for s in sizes], phases=None)

    def cycle(part, c):
        if drv == "c":
            cut, out, st = g.vcycle_native(a.k, part, seed=1 + c, jet=jet, resident=True,
                                           engine=eng)
            return cut, out, dict(levels=st.levels, phases=phases_of(st),
                                  accepted=bool(st.vcycles_accepted))
        cut, out, sizes, acc = vcycle(g, a.k, part, seed=1 + c, jet=jet, resident=True,
                                      engine=eng)
        return cut, out, dict(levels=[int(s) for s in sizes], phases=None, accepted=bool(acc))

    def sequence():
        rows = []
        row, part = stage(driver)
        rows.append(row)
        for c in range(a.cycles):
            row, part = stage(lambda: cycle(part, c))
            rows.append(row)
        checksum = checksum_of(part)
        if a.with_option:  # the drivers' own option: one call, cycles included
            row, part = stage(lambda: driver(a.cycles))
            assert row["cut"] == rows[-1]["cut"] and checksum_of(part) == checksum
            rows.append(row)
        return rows, checksum

    def checksum_of(part):
        return int(np.bitwise_xor.reduce(
            np.asarray(part, np.uint64) * np.arange(1, g.n + 1, dtype=np.uint64)))

    first, checksum = sequence()  # warm-up
    runs = []
    for _ in range(a.reps):
        rows, cs = sequence()
        assert cs == checksum
        for r, f in zip(rows, first):
            for q in ("cut", "levels", "label_bytes"):
                assert r[q] == f[q], q
        runs.append(rows)
    stages = []
    for i, f in enumerate(first):
        times = [round(run[i]["seconds"], 4) for run in runs]
        phases = None
        if f["phases"] is not None:  # median over the timed repetitions, phase by phase
            phases = {q: round(statistics.median(run[i]["phases"][q] for run in runs), 4)
                      for q in f["phases"]}
        name = "driver" if i == 0 else f"cycle{i}"
        if i > a.cycles:
            name = f"driver_vcycles{a.cycles}"
        stages.append({
            "stage": name, "cut": f["cut"],
            "levels": f["levels"], "accepted": f.get("accepted"),
            "label_bytes": int(f["label_bytes"]), "seconds": times,
            "median_seconds": round(statistics.median(times), 4),
            "spread_seconds": round(max(times) - min(times), 4),
            "phase_seconds_median": phases})
    print(json.dumps({"n": int(g.n), "m": int(g.m), "part_checksum": checksum,
                      "stages": stages}))


def run_parent(a):
    out = {"graph": f"rmat{a.scale}_s42", "k": a.k, "eps": 0.03, "seed": 1, "reps": a.reps,
           "cycles": a.cycles, "resident": True, "configs": {}}
    names = [n for n in config_names()
             if split_name(n)[0] in a.pipelines.split(",")
             and split_name(n)[1] in a.refiners.split(",")
             and split_name(n)[2] in a.drivers.split(",")]
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--scale",
               str(a.scale), "--k", str(a.k), "--reps", str(a.reps), "--cycles", str(a.cycles)]
        if a.with_option:
            cmd.append("--with-option")
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
        print(name + ": " + "  ".join(
            f"{s['stage']} cut {s['cut']} {s['median_seconds']} s" for s in row["stages"]),
            flush=True)
        if a.out:  # keep what is done if a later child runs out of time
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
                fh.write("\n")
    for name in names:
        pipe, ref, drv = split_name(name)
        other = f"{pipe}_{ref}_{'py' if drv == 'c' else 'c'}"
        if drv == "c" and other in out["configs"]:
            c, py = out["configs"][name], out["configs"][other]
            assert c["part_checksum"] == py["part_checksum"], name
            assert [s["cut"] for s in c["stages"]] == [s["cut"] for s in py["stages"]], name
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=240.0,
                    help="time limit of one configuration's child process, seconds")
    ap.add_argument("--pipelines", default=",".join(PIPELINES))
    ap.add_argument("--refiners", default=",".join(REFINERS))
    ap.add_argument("--drivers", default=",".join(DRIVERS))
    ap.add_argument("--with-option", action="store_true",
                    help="also time the driver with vcycles=CYCLES in one call")
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
            fh.write("\n")


if __name__ == "__main__":
    main()
