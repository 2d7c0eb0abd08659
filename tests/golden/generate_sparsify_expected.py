"""Generate the expected results of the multilevel drivers with the `sparsify`
option by running the CPU mirror (tests/sparsify_mirror.py: the oracle
pipelines with their contraction wrapped by the numpy twin of the pass). Every
stage is bit-reproducible, so the GPU drivers must reproduce these exactly
(test_sparsify_gpu.py), and the mirror itself is pinned to them
(test_sparsify_cpu.py).

Run here (CPU):  PYTHONPATH=.:tests python tests/golden/generate_sparsify_expected.py
Writes tests/golden/sparsify_expected.json.
"""

import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import kaminpar_amd as ka
from sparsify_mirror import mirror_partition, mirror_partition_deep

DEEP_SPLIT_C = 2000  # the mid-split schedule: coarse levels are used for splits


def record(g, result):
    cut, part, levels, stats = result
    return {
        "cut": int(cut), "levels": [int(x) for x in levels],
        "level_arcs": stats["level_arcs"],
        "arcs_before": [st["m_before"] for st in stats["sparsify"]],
        "arcs_after": [st["m_after"] for st in stats["sparsify"]],
        "applied": [st["applied"] for st in stats["sparsify"]],
        "part_checksum": int(np.bitwise_xor.reduce(
            np.asarray(part, np.uint64) * np.arange(1, g.n + 1, dtype=np.uint64))),
    }


def main():
    oracle = ctypes.CDLL(os.path.join(REPO, "oracle", "liblp_oracle.so"))
    oracle.kmp_oracle_lp_refine.restype = ctypes.c_int64
    oracle.kmp_oracle_lp_cluster.restype = ctypes.c_int64
    out = {}
    for scale in (14, 16):
        g = ka.Graph.rmat(scale, 8, 42)
        for laziness in (1, 2):
            opt = dict(laziness_factor=laziness)
            name = f"rmat{scale}_s42_k16_lazy{laziness}"
            out[name] = {
                "k": 16, "seed": 1, "laziness_factor": laziness,
                "partition": record(g, mirror_partition(oracle, g, 16, opt, seed=1)),
                "partition_deep": record(g, mirror_partition_deep(
                    oracle, g, 16, opt, seed=1, split_c=DEEP_SPLIT_C)),
            }
            print(name, out[name])
    with open(os.path.join(HERE, "sparsify_expected.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
