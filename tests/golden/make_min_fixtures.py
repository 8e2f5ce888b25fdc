"""Records tests/golden/ref_min_*.npz from the reference binary (oracle/_ref/ge_ref;
run where the reference tree is present):

  ref_min_small.npz, ref_min_full.npz -- the levels of tests/min_cases.py.  Per
      aggregate the reference's embedViaMinimization(sub, d, zeros, sweeps) on the
      sub-pattern, then anyToMultilevel's normalisation and placement in numpy in the
      reference's operation order (min_cases.place).  x_d<dim>: n x dim.
  ref_min_e2e.npz -- embedVia(As, P_Ts, 2, anyToMultilevel(embedViaMinimization)) of
      the reference itself on min_cases.E2E: nothing restated.

    python tests/golden/make_min_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import min_cases as M  # noqa: E402
import oracle_lib as O  # noqa: E402
import ref_cases as C  # noqa: E402
import ref_lib as R  # noqa: E402


def main():
    assert R.available(), "the reference binary is needed to record fixtures"
    for name in M.LEVELS:
        lv = M.level(name)
        out = {"sha": np.array(M.SHA[name])}
        for dim in M.DIMS[name]:
            out[f"x_d{dim}"] = M.compose(
                lv, dim, lv["iterations"],
                lambda A, d, X0, it: R.embed_via_minimization(A, d, coords=X0, iterations=it))
        np.savez_compressed(os.path.join(HERE, f"ref_min_{name}.npz"), **out)
        print(name, {k: getattr(v, "shape", v) for k, v in out.items()})
    e = M.E2E
    A = M.e2e_graph()
    hier = R.partition(A, cf=e["cf"])
    As = O.hierarchy_As(A, hier)
    coords = R.embed_via_minimization_ml(As, hier, e["dim"], seed=e["seed"])
    out = {"coords": coords, "A_ip_sha": np.array(C.sha(A[0])), "A_ix_sha": np.array(C.sha(A[1]))}
    out.update(C.hier_arrays("h", hier))
    np.savez_compressed(os.path.join(HERE, "ref_min_e2e.npz"), **out)
    print("e2e", coords.shape, [p[2] for p in hier], int(np.isnan(coords).sum()))


if __name__ == "__main__":
    main()
