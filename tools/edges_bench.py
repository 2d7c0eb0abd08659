"""What building the engine's CSR on the device from an edge list costs
(kmp_lp_create_from_edges, LpEngine.from_edges).

R-MAT scale S (edge factor 8, seed 42): the upper triangle of the generator's
CSR, one direction per edge, shuffled on the device with a fixed seed. The
list therefore holds no duplicates and no self-loops; what is measured is
validation, sort, collapse and CSR build of 2 * E arcs.

  build    variants {dev_i64, dev_i32: GPU tensors as a torch user holds them;
           host_u32: numpy arrays, staged through one upload} x {unweighted,
           weighted (1..7, max)}, plus dev_i32 with KMP_EDGES_SORT64 (all 64 key
           bits sorted instead of 2 * bit_width(n)) as the A/B of the restricted
           sort. One process: every variant once as a warm-up, then --reps
           rounds over all of them in the same order, so the variants alternate
           and the spread of each is visible next to the differences. Per
           variant: the HIP-event times of pack / sort / build (collapse + CSR),
           the synced wall time of the call (engine allocation and isolated scan
           included), peak temporaries, arcs per second of the best run, and the
           model bytes of each phase over its event time. The model assumes
           8-bit digits (ceil(bits / 8) passes, each reading and writing keys
           and values once, plus one histogram read); the phases stream, so the
           bound that applies is HBM bandwidth. For comparison only, not a pass
           criterion: LpEngine(g) from the READY host CSR of the same graph,
           the cheapest thing the library offered before; it excludes the CSR
           construction that path leaves to the caller.
  kernels  the workload for a separate `rocprofv3 --kernel-trace --stats` run
           with nothing else collected: dev_i32 unweighted and weighted, --reps
           builds each.

Usage (GPU box):
  python tools/edges_bench.py build --scale 23 --out profiles/edges/build_rmat23.json
  rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/edges_bench.py kernels --scale 23
  python tools/largek_bench.py kstats --csv OUT/.../*_kernel_stats.csv --out profiles/edges/kernel_stats_rmat23.json
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_list(scale, with_graph):
    """(graph or None, n, m, src, dst, weights): the shuffled upper triangle
    as int32 GPU tensors; the graph is kept only for the host-CSR comparison."""
    import numpy as np
    import torch

    import kaminpar_amd as ka

    g = ka.Graph.rmat(scale, 8, seed=42)
    n, m = int(g.n), int(g.m)
    xadj = np.asarray(g.xadj).astype(np.int64)
    adjncy = np.asarray(g.adjncy)
    rows = np.repeat(np.arange(n, dtype=np.uint32), np.diff(xadj))
    up = rows < adjncy
    src = torch.as_tensor(rows[up].astype(np.int32), device="cuda:0")
    dst = torch.as_tensor(adjncy[up].astype(np.int32), device="cuda:0")
    del rows, up
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(23)
    perm = torch.randperm(src.numel(), device="cuda:0", generator=gen)
    src, dst = src[perm].contiguous(), dst[perm].contiguous()
    w = (perm % 7 + 1).to(torch.int32).contiguous()
    del perm
    torch.cuda.synchronize()
    assert 2 * src.numel() == m
    return (g if with_graph else None), n, m, src, dst, w


def model_bytes(pairs, m, n, id_bytes, weighted, bits):
    arc = 8 + (4 if weighted else 0)
    passes = (bits + 7) // 8
    return {
        "pack": pairs * (2 * id_bytes + (4 if weighted else 0)) + 2 * pairs * arc,
        "sort": 2 * pairs * 8 + passes * 2 * (2 * pairs * arc),
        "build": 2 * pairs * arc + m * arc + m * arc + m * (arc - 4) + 16 * (n + 1),
        "sort_passes_assumed": passes,
    }


def run_build(a):
    import numpy as np
    import torch

    import kaminpar_amd as ka

    t0 = time.perf_counter()
    g, n, m, s32, d32, w = make_list(a.scale, True)
    prep = time.perf_counter() - t0
    pairs = s32.numel()
    s64, d64 = s32.to(torch.int64), d32.to(torch.int64)
    hs, hd = s32.cpu().numpy().astype(np.uint32), d32.cpu().numpy().astype(np.uint32)
    hw = w.cpu().numpy()
    inputs = {"dev_i64": (s64, d64, w, 8), "dev_i32": (s32, d32, w, 4),
              "host_u32": (hs, hd, hw, 4)}
    variants = [(src, weighted, 0) for src in inputs for weighted in (False, True)]
    variants += [("dev_i32", weighted, ka.EDGES_SORT64) for weighted in (False, True)]
    bits = 2 * int(n).bit_length()

    def name_of(v):
        return f"{v[0]}_{'weighted' if v[1] else 'unweighted'}" + ("_sort64" if v[2] else "")

    def one(v):
        src, dst, wgt, _ = inputs[v[0]]
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng, st = ka.LpEngine.from_edges(src, dst, n=n, weights=wgt if v[1] else None,
                                         return_stats=True, _flags=v[2])
        wall = time.perf_counter() - t
        row = st.as_dict()
        row["python_wall_ns"] = int(wall * 1e9)
        assert row["arcs"] == m and row["self_loops"] == 0 and row["merged_arcs"] == 0
        del eng
        return row

    def host_csr():
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng = ka.LpEngine(g)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        del eng
        return int(dt * 1e9)

    for v in variants:  # warm-up
        one(v)
    host_csr()
    rounds, host_rounds = [], []
    for _ in range(a.reps):
        rounds.append({name_of(v): one(v) for v in variants})
        host_rounds.append(host_csr())
    out = {"graph": f"rmat{a.scale}_s42_upper_triangle_shuffled", "n": n, "pairs": pairs,
           "arcs": m, "reps": a.reps, "key_bits_sorted": bits, "order": [name_of(v) for v in variants],
           "list_preparation_seconds_not_part_of_any_figure": round(prep, 2),
           "bound": "HBM bandwidth (streaming pack / radix passes / collapse / build)",
           "variants": {}}
    for v in variants:
        runs = [r[name_of(v)] for r in rounds]
        best = min(runs, key=lambda r: r["total_ns"])
        mb = model_bytes(pairs, m, n, inputs[v[0]][3], v[1], 64 if v[2] else bits)
        row = {"best": best, "arcs_per_second": round(m / (best["total_ns"] / 1e9)),
               "model_bytes": mb}
        for q in ("pack_ns", "sort_ns", "build_ns", "total_ns", "python_wall_ns"):
            row[q] = [r[q] for r in runs]
        for ph in ("pack", "sort", "build"):
            row[f"{ph}_model_GBps"] = round(mb[ph] / best[f"{ph}_ns"], 1)
        out["variants"][name_of(v)] = row
    out["ready_host_csr_LpEngine_ns"] = host_rounds
    out["ready_host_csr_note"] = ("LpEngine(g) from a finished host CSR: upload and engine "
                                  "allocation only; the CSR construction is the caller's and is "
                                  "not in this figure")
    return out


def run_kernels(a):
    import kaminpar_amd as ka

    _, n, m, src, dst, w = make_list(a.scale, False)
    for _ in range(a.reps):
        for wgt in (None, w):
            eng = ka.LpEngine.from_edges(src, dst, n=n, weights=wgt)
            assert eng.m == m
            del eng
    return {"graph": f"rmat{a.scale}_s42_upper_triangle_shuffled", "n": n, "arcs": m,
            "pairs": src.numel(), "reps": a.reps, "builds": 2 * a.reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["build", "kernels"])
    ap.add_argument("--scale", type=int, default=23)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "build" and a.reps < 3:
        ap.error("needs at least three timed repetitions")
    out = run_build(a) if a.mode == "build" else run_kernels(a)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
