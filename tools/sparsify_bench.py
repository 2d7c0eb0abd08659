"""What the threshold edge sparsification of the coarse graphs costs and gains
in the multilevel drivers.

R-MAT scale S (edge factor 8, seed 42), k blocks, eps 0.03, seed 1, resident
labels, one engine for the fine graph reused by every run.

  pipeline  the settings {off, defaults, laziness 2, laziness 1} on the drivers
            {basic: partition(), deep: partition_deep(), cdeep:
            kmp_partition_deep_ex} with the refiners {lp, jet_sel: Jet with
            balancer=1}. Every (driver, refiner) pair runs in a child process
            of its own under a time limit. The child runs the four settings in
            turn as a warm-up, then --reps more rounds of the four in the same
            order, so the settings alternate in one process and the spread of
            each is visible next to the differences between them. A run is
            timed from call to return (the drivers return host arrays, so the
            device has finished). Per setting: cut, best and all seconds,
            level sizes, level arcs, the arcs before and after the pass per
            level, and for cdeep the phase times of kmp_pipeline_stats_t (of
            the best run). The baseline of every figure is `off` of the same
            child. The first child that fails or runs out of time ends the run.
  kernels   the workload for a separate `rocprofv3 --kernel-trace --stats` run
            with nothing else collected: level 0 is clustered once, then --reps
            times contracted with the pass at laziness 1 (the pass always
            triggers), and --reps times the block subgraphs of the unsparsified
            level-1 graph are extracted (k blocks, labels u mod k), so that the
            extraction's count and fill kernels are timed in the same run on
            the same graph. Prints the arcs the pass read and kept. With
            KMP_SPARSIFY_FLAGS set in the environment the pass stores a byte
            per arc in count and reads it in fill instead of evaluating the
            rule twice: trace both forms in runs of their own to compare them.

Usage (GPU box):
  python tools/sparsify_bench.py pipeline --scale 20 --out profiles/sparsify/pipeline_rmat20_k16.json
  rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/sparsify_bench.py kernels --scale 20
  python tools/largek_bench.py kstats --csv OUT/.../*_kernel_stats.csv --out profiles/sparsify/kernel_stats_rmat20_k16.json
"""

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SETTINGS = {"off": False, "defaults": True, "lazy2": dict(laziness_factor=2),
            "lazy1": dict(laziness_factor=1)}
REFINERS = {"lp": False, "jet_sel": dict(balancer=1)}
DRIVERS = ("basic", "deep", "cdeep")


def run_child(a):
    import numpy as np

    import kaminpar_amd as ka
    from kaminpar_amd.partition import partition, partition_deep

    drv, ref = a.child.split(":")
    jet = REFINERS[ref]
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)  # fine CSR stays resident

    def one(opt):
        t0 = time.perf_counter()
        if drv == "cdeep":
            cut, part, st = g.partition_deep_native(
                a.k, seed=1, jet=jet, resident=True, engine=eng, sparsify=opt,
                return_stats=True)
            dt = time.perf_counter() - t0
            row = dict(levels=st.levels, level_arcs=st.arcs,
                       sparsified_levels=int(st.sparsified_levels),
                       arcs_dropped=int(st.sparsify_arcs_dropped),
                       phases={q[0][:-3]: round(getattr(st, q[0]) / 1e9, 4)
                               for q in st._fields_ if q[0].endswith("_ns")})
        else:
            stats = {}
            cut, part, sizes = (partition_deep if drv == "deep" else partition)(
                g, a.k, seed=1, jet=jet, resident=True, engine=eng, sparsify=opt,
                stats=stats)
            dt = time.perf_counter() - t0
            per = [s for s in stats["sparsify"] if s is not None]
            row = dict(levels=[int(s) for s in sizes], level_arcs=stats["level_arcs"],
                       arcs_before=[s["m_before"] for s in per],
                       arcs_after=[s["m_after"] for s in per],
                       applied=[s["applied"] for s in per],
                       pass_seconds=round(sum(s["pass_ns"] for s in per) / 1e9, 5))
        assert cut == g.edge_cut(part)
        row.update(cut=int(cut), seconds=round(dt, 4), checksum=int(np.bitwise_xor.reduce(
            np.asarray(part, np.uint64) * np.arange(1, g.n + 1, dtype=np.uint64))))
        return row

    first = {name: one(opt) for name, opt in SETTINGS.items()}  # warm-up
    rounds = [{name: one(opt) for name, opt in SETTINGS.items()} for _ in range(a.reps)]
    out = {}
    for name in SETTINGS:
        runs = [r[name] for r in rounds]
        for r in runs:
            for q in ("cut", "levels", "level_arcs", "checksum"):
                assert r[q] == first[name][q], (name, q)
        best = min(runs, key=lambda r: r["seconds"])
        out[name] = dict(best, best_seconds=best["seconds"],
                         seconds=[r["seconds"] for r in runs])
    print(json.dumps({"n": int(g.n), "m": int(g.m), "settings": out}))


def run_pipeline(a):
    out = {"graph": f"rmat{a.scale}_s42", "k": a.k, "eps": 0.03, "seed": 1, "reps": a.reps,
           "resident": True, "order": list(SETTINGS), "configs": {}}
    names = [f"{d}:{r}" for d in a.drivers.split(",") for r in a.refiners.split(",")]
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "pipeline", "--child", name,
               "--scale", str(a.scale), "--k", str(a.k), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            # stopped at its limit: it may hang the GPU, so start nothing more
            print(f"{name}: no result within {a.step_timeout} s; stopping", flush=True)
            out["configs"][name] = {"stopped_after_seconds": a.step_timeout}
            break
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            out["configs"][name] = {"failed": r.returncode}
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        out["n"], out["m"] = row.pop("n"), row.pop("m")
        out["configs"][name] = row["settings"]
        base = row["settings"]["off"]
        print(name + ": " + "  ".join(
            f"{s} cut {v['cut']} ({v['cut'] / base['cut']:.3f}) {v['best_seconds']} s "
            f"({v['best_seconds'] / base['best_seconds']:.3f})"
            for s, v in row["settings"].items()), flush=True)
        if a.out:  # keep what is done if a later child runs out of time
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
                fh.write("\n")
    return out


def run_kernels(a):
    import numpy as np

    import kaminpar_amd as ka
    from kaminpar_amd.partition import level_cluster_weight

    g = ka.Graph.rmat(a.scale, 8, seed=42)
    eng = ka.LpEngine(g)
    mcw = level_cluster_weight(g.total_node_weight, g.n, a.k, 0.03)
    eng.cluster(mcw, seed=1, download=False)
    st = None
    for _ in range(a.reps):
        coarse, _ = eng.contract_engine(None, download_mapping=False,
                                        sparsify=dict(laziness_factor=1), seed=1)
        st = coarse.sparsify_stats.as_dict()
        del coarse
    plain, _ = eng.contract_engine(None, download_mapping=False)
    part = (np.arange(plain.n, dtype=np.uint64) % a.k).astype(np.uint32)
    for _ in range(a.reps):
        sub = plain.extract_subgraphs(a.k, part)
        ext = dict(count_ns=int(sub.stats.count_ns), fill_ns=int(sub.stats.fill_ns))
        del sub
    return {"graph": f"rmat{a.scale}_s42", "k": a.k, "reps": a.reps, "level1_n": int(plain.n),
            "level1_m": int(plain.m), "pass": st, "extract_events": ext}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["pipeline", "kernels"])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=240.0,
                    help="time limit of one (driver, refiner) child process, seconds")
    ap.add_argument("--drivers", default=",".join(DRIVERS))
    ap.add_argument("--refiners", default=",".join(REFINERS))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "pipeline" and a.child:
        run_child(a)
        return
    if a.mode == "pipeline" and a.reps < 3:
        ap.error("needs at least three timed repetitions")
    out = run_pipeline(a) if a.mode == "pipeline" else run_kernels(a)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
