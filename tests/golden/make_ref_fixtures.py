"""Records tests/golden/ref_*.npz and ref_manifest.json from the reference binary
(oracle/_ref/ge_ref: the reference's own translation units, oracle/Makefile).

    python tests/golden/make_ref_fixtures.py [case ...]

Each .npz holds only outputs of the reference; the inputs are rebuilt from
tests/ref_cases.py, and the manifest keeps a sha256 of every input array, the
compile flags and the sha256 of the reference files the binary was built from.
P^T A P (the As of the embed case) is linalgcpp's operation, not the
reference's: it comes from the oracle and is hashed as an input.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib as O  # noqa: E402
import ref_cases as C  # noqa: E402
import ref_lib as R  # noqa: E402

MAX_BYTES = 256 * 1024


def derive(name):
    """(arrays, manifest entry) of one fixture, from the live reference binary."""
    if name in C.FA_CASES:
        case = C.fa_case(name)
        return {"x": C.run_fa(R.force_atlas, case)}, {"inputs": C.input_hashes(case)}
    if name in C.ML_CASES:
        case = C.ml_case(name)
        entry = {"inputs": C.input_hashes(case),
                 "local_global_edges": C.local_global_edges(case["A"], case["PT"])}
        if name in C.ML_QUIRK:
            assert entry["local_global_edges"] > 0, (name, "change the permutation seed")
        return {"x": C.run_ml(R.force_atlas_ml, case)}, entry
    if name.startswith("P_"):
        case = C.p_case(name[2:])
        arrays, q = {}, {}
        for cf in C.P_CFS:
            hier = R.partition(case["A"], cf=cf, **case["kw"])
            arrays.update(C.hier_arrays("cf" + C.cf_key(cf), hier))
            if name == "P_rmat":  # Q: modularity per level of one P case
                As = O.hierarchy_As(case["A"], hier)
                q[C.cf_key(cf)] = [R.modularity(Al, PT).hex() for Al, PT in zip(As, hier)]
        entry = {"inputs": C.input_hashes(case)}
        if q:
            entry["modularity"] = q
        return arrays, entry
    if name == "E":
        A = C.e_graph()
        hier = R.partition(A, cf=C.E_CF)
        As = O.hierarchy_As(A, hier)
        arrays = C.hier_arrays("h", hier)
        for d in C.E_DIMS:
            arrays[f"x_d{d}"] = R.embed(As, hier, d, seed=C.E_SEED)
        entry = {"inputs": C.input_hashes({"As": As}), "seed": C.E_SEED,
                 "modularity": [R.modularity(Al, PT).hex() for Al, PT in zip(As, hier)]}
        return arrays, entry
    raise KeyError(name)


def all_names():
    return list(C.FA_CASES) + list(C.ML_CASES) + ["P_" + p for p in C.P_NAMES] + ["E"]


def main(argv):
    assert R.available(), "no reference binary: build oracle/ with the reference tree present"
    names = argv or all_names()
    man = C.manifest() if os.path.exists(C.MANIFEST) else {"cases": {}}
    man["build"] = R.build_info()
    for name in names:
        arrays, entry = derive(name)
        path = os.path.join(HERE, f"ref_{name}.npz")
        np.savez(path, **arrays)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (name, size)
        man["cases"][name] = entry
        print(f"{name}: {size} bytes")
    with open(C.MANIFEST, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
