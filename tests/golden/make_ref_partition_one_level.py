"""Records tests/golden/ref_partition_one_level.npz from the reference binary
(oracle/_ref/ge_ref): the one-level overloads partition(A, numParts, ...) and
partition(A, printing, ...) (src/partitioner.cpp:1272-1544, :970-1266).

    python tests/golden/make_ref_partition_one_level.py

Arrays only: per graph the input CSR (so the test can tell a changed generator
from a changed result) and, per num_parts and for the overload without one, the
P_T's indptr and indices.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import partition_trace as PT  # noqa: E402
import ref_lib as R  # noqa: E402

KW = dict(positive_merging=False, matching=1, stall=0.9)


def graphs():
    return {"rmat600": PT.graph("rmat600"), "er600w": PT.weights_from(PT.graph("er600"), PT.W3)}


def parts_of(A):
    return (1, 40, 200, len(A[0]) - 1)


def main():
    out = {}
    for name, A in graphs().items():
        for part, arr in zip(("ip", "ix", "dx"), A):
            out[f"{name}_A_{part}"] = np.asarray(arr)
        for p in parts_of(A):
            (lv,) = R.partition(A, num_parts=p, **KW)
            out[f"{name}_parts{p}_ip"], out[f"{name}_parts{p}_ix"] = lv[0], lv[1]
            print(name, "num_parts", p, "->", lv[2], "aggregates")
        (lv,) = R.partition(A, **KW)
        out[f"{name}_single_ip"], out[f"{name}_single_ix"] = lv[0], lv[1]
        print(name, "single ->", lv[2], "aggregates")
    path = os.path.join(HERE, "ref_partition_one_level.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
