"""Measurements for the resident label state (LpEngine.set_labels / get_labels /
project_from and resident=True of the pipelines).

Two modes, each printing JSON and optionally writing it to --out:

  pipeline  partition_deep on R-MAT scale S (edge factor 8, seed 42) with
            default arguments and with jet=dict(balancer=1), each with
            resident False and True. One process, one engine for the fine
            graph; every configuration is warmed up once, then the four
            alternate for --reps timed repetitions. A host clock around the
            call (which ends synchronised) gives the time; the delta of
            label_traffic_bytes() around the call gives the label bytes that
            crossed PCIe. Cut, partition and level sizes of the two modes are
            asserted equal. The yardstick is resident=False in the same
            process; "spread" is max - min over the repetitions of one
            configuration.
  project   project_from alone on the finest level: the fine graph is clustered
            and contracted once (resident forms), the coarse engine gets a
            partition, and the projection is timed with HIP events on a stream
            both engines adopt, --reps times after a warm-up: gathering from
            the u8 shadow (coarse state left by refine) and from the u32 labels
            (coarse state left by set_labels). Next to it, in the same run and
            on the same stream, a device-to-device hipMemcpyAsync of 8 n bytes
            (the yardstick) and one of 4 n bytes, which moves exactly the
            projection's compulsory traffic: one 4-byte read and one 4-byte
            write per vertex.

Usage (GPU box):
  python tools/resident_bench.py pipeline --scale 23 --k 16 --out p23.json
  python tools/resident_bench.py project --scale 23 --k 16 --out j23.json
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = {
    # name: (jet, resident)
    "lp_host": (False, False),
    "lp_resident": (False, True),
    "jet_host": (True, False),
    "jet_resident": (True, True),
}


def run_pipeline(a):
    import kaminpar_amd as ka
    from kaminpar_amd.partition import partition_deep

    t0 = time.perf_counter()
    g = ka.Graph.rmat(a.scale, 8, seed=42)
    gen_s = time.perf_counter() - t0
    eng = ka.LpEngine(g)  # fine CSR stays resident

    def call(name):
        jet, resident = CONFIGS[name]
        b0 = ka.label_traffic_bytes()
        t0 = time.perf_counter()
        cut, part, sizes = partition_deep(
            g, a.k, seed=1, engine=eng, jet=dict(balancer=1) if jet else False,
            resident=resident)
        dt = time.perf_counter() - t0
        return dict(cut=int(cut), part=part, sizes=[int(s) for s in sizes], seconds=dt,
                    label_bytes=ka.label_traffic_bytes() - b0)

    first = {name: call(name) for name in CONFIGS}  # warm-up of each
    for host, res in (("lp_host", "lp_resident"), ("jet_host", "jet_resident")):
        assert first[host]["cut"] == first[res]["cut"], (host, res)
        assert (first[host]["part"] == first[res]["part"]).all(), (host, res)
        assert first[host]["sizes"] == first[res]["sizes"], (host, res)
    times = {name: [] for name in CONFIGS}
    for _ in range(a.reps):
        for name in CONFIGS:
            r = call(name)
            assert r["cut"] == first[name]["cut"]
            assert r["label_bytes"] == first[name]["label_bytes"]
            times[name].append(round(r["seconds"], 4))
            print(f"{name}: {r['seconds']:.3f} s", flush=True)
    out = {"mode": "pipeline", "graph": f"rmat{a.scale}_s42", "n": int(g.n), "m": int(g.m),
           "k": a.k, "eps": 0.03, "reps": a.reps, "generation_seconds": round(gen_s, 1),
           "levels": first["lp_host"]["sizes"], "configs": {}}
    for name in CONFIGS:
        ts = times[name]
        out["configs"][name] = {
            "cut": first[name]["cut"], "seconds": ts,
            "median_seconds": round(statistics.median(ts), 4),
            "spread_seconds": round(max(ts) - min(ts), 4),
            "warmup_seconds": round(first[name]["seconds"], 4),
            "label_bytes_per_call": int(first[name]["label_bytes"])}
    for host, res in (("lp_host", "lp_resident"), ("jet_host", "jet_resident")):
        h, r = out["configs"][host], out["configs"][res]
        out[f"{res}_over_{host}"] = round(r["median_seconds"] / h["median_seconds"], 4)
    return out


def run_project(a):
    import torch

    torch.zeros(1, device="cuda:0")  # torch's runtime first (see kaminpar_amd._load)
    import kaminpar_amd as ka
    from kaminpar_amd.partition import level_cluster_weight

    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.c_int, ctypes.c_void_p]
    d2d = 3  # hipMemcpyDeviceToDevice

    g = ka.Graph.rmat(a.scale, 8, seed=42)
    fine = ka.LpEngine(g)
    mcw = level_cluster_weight(g.total_node_weight, g.n, a.k, 0.03)
    fine.cluster(mcw, seed=1, download=False)
    coarse, _ = fine.contract_engine(None, download_mapping=False)
    caps = np.full(a.k, g.max_block_weight(a.k, 0.03), dtype=np.int64)
    cpart = ka.random_partition(coarse.n, a.k, seed=3)

    coarse.set_labels(a.k, cpart)
    coarse.refine(a.k, caps, None, seed=1, iters=1)  # leaves the shadows valid

    stream = torch.cuda.Stream()
    src = torch.empty(8 * g.n, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(8 * g.n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    coarse.set_stream(stream.cuda_stream)
    fine.set_stream(stream.cuda_stream)

    def timed(fn):
        ms = []
        for i in range(a.reps + 1):  # first repetition is the warm-up
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i > 0:
                ms.append(round(e0.elapsed_time(e1), 4))
        return ms

    def copy(nbytes=8 * g.n):
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, d2d,
                                stream.cuda_stream)
        assert rc == 0, rc

    rows = {}
    rows["project_u8_shadow_ms"] = timed(lambda: fine.project_from(coarse))
    rows["copy_8n_bytes_ms"] = timed(copy)
    coarse.set_labels(a.k, cpart)  # d_labels only: the gather reads the u32 array
    rows["project_u32_labels_ms"] = timed(lambda: fine.project_from(coarse))
    rows["copy_8n_bytes_again_ms"] = timed(copy)
    rows["copy_4n_bytes_ms"] = timed(lambda: copy(4 * g.n))
    stream.synchronize()
    coarse.set_stream(None)
    fine.set_stream(None)
    out = {"mode": "project", "graph": f"rmat{a.scale}_s42", "n": int(g.n),
           "coarse_n": int(coarse.n), "k": a.k, "reps": a.reps, **rows}
    med = {q: statistics.median(v) for q, v in rows.items()}
    out["median_ms"] = {q: round(v, 4) for q, v in med.items()}
    copy_ms = min(med["copy_8n_bytes_ms"], med["copy_8n_bytes_again_ms"])
    out["project_u8_over_copy"] = round(med["project_u8_shadow_ms"] / copy_ms, 3)
    out["project_u32_over_copy"] = round(med["project_u32_labels_ms"] / copy_ms, 3)
    out["project_u8_bytes_per_s"] = round(8 * g.n / med["project_u8_shadow_ms"] * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["pipeline", "project"])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "pipeline" and a.reps < 3:
        ap.error("pipeline needs at least three timed repetitions")
    out = {"pipeline": run_pipeline, "project": run_project}[a.mode](a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
