"""Records tests/golden/ref_dims_*.npz and ref_dims_manifest.json -- the cases above
dimension 4 of tests/dims_cases.py -- from the reference binary (oracle/_ref/ge_ref:
the reference's own translation units, oracle/Makefile).

    python tests/golden/make_ref_dims.py

Same rules as make_ref_fixtures.py: each .npz holds only outputs of the reference;
the manifest keeps a sha256 of every input array, the compile flags and the sha256
of the reference files the binary was built from.  P^T A P (the As of the embed
case) comes from the oracle and is hashed as an input.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dims_cases as D  # noqa: E402
import oracle_lib as O  # noqa: E402
import ref_cases as C  # noqa: E402
import ref_lib as R  # noqa: E402

MAX_BYTES = 256 * 1024


def save(name, arrays):
    path = os.path.join(HERE, f"ref_dims_{name}.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes")


def main():
    assert R.available(), "no reference binary: build oracle/ with the reference tree present"
    man = {"build": R.build_info(), "cases": {}}
    for d in D.DIMS:
        arrays, entry = {}, {}
        for name in D.fa_names():
            case = D.fa_case(name, d)
            arrays[name] = C.run_fa(R.force_atlas, case)
            entry[name] = {"inputs": C.input_hashes(case)}
        save(f"fa_d{d}", arrays)
        man["cases"][f"fa_d{d}"] = entry
        arrays, entry = {}, {}
        for name in D.ml_names(d):
            case = D.ml_case(name, d)
            arrays[name] = C.run_ml(R.force_atlas_ml, case)
            entry[name] = {"inputs": C.input_hashes(case)}
        save(f"ml_d{d}", arrays)
        man["cases"][f"ml_d{d}"] = entry
    A = D.e_graph()
    hier = R.partition(A, cf=D.E_CF)
    As = O.hierarchy_As(A, hier)
    arrays = C.hier_arrays("h", hier)
    for d in D.E_DIMS:
        arrays[f"x_d{d}"] = R.embed(As, hier, d, seed=D.E_SEED)
    save("embed", arrays)
    man["cases"]["embed"] = {"inputs": C.input_hashes({"As": As}), "seed": D.E_SEED}
    with open(D.MANIFEST, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
