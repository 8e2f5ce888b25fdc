"""ge_embed_via_minimization_ml on its host path (ctx=None): one level of
anyToMultilevel(embedViaMinimization) behind the C ABI, the CPU-testable twin of
the batched device call (tests/test_gpu_minimize_ml.py).  Pinned to fixtures
recorded from the reference binary (tests/golden/make_min_fixtures.py), to the
composition the drop-in header performs with one ge_embed_via_minimization call
per aggregate, and to the live reference where it is available."""
import os

import numpy as np
import pytest

import ge_amd as ge
import min_cases as M

CASES, build_driver, run_level = M.CASES, M.build_driver, M.run_level


@pytest.mark.parametrize("name,dim", CASES)
def test_host_equals_reference_fixture(golden, name, dim):
    lv = M.level(name)
    g = golden(f"ref_min_{name}")
    assert str(g["sha"]) == M.SHA[name]
    want = g[f"x_d{dim}"]
    got, info = run_level(lv, dim, info=True)
    assert info == {"packed": 0, "wave": 0, "host": lv["m"], "path": 0}
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert M.same(got, want)
    # the NaN cases are there: the one-member and the edgeless aggregate, all of them
    sizes = np.array(lv["sizes"])
    for a in (int(np.flatnonzero(sizes == 1)[0]), int(np.flatnonzero(sizes == 4)[0])):
        v = lv["PT"][1][lv["PT"][0][a]:lv["PT"][0][a + 1]]
        assert np.isnan(want[v]).all()
    assert np.isfinite(want).any()


@pytest.mark.parametrize("name,dim", CASES)
def test_host_equals_header_composition(name, dim):
    lv = M.level(name)
    want = M.compose(lv, dim, lv["iterations"],
                     lambda A, d, X0, it: ge.embed_via_minimization(A, d, coords=X0,
                                                                    iterations=it))
    assert M.same(run_level(lv, dim), want)


def test_unsorted_member_lists_take_the_sorted_sub_pattern():
    """Member lists that are not ascending: the sub-matrix rows are sorted by local
    index (CooMatrix::ToSparse), which is no longer the stored order."""
    lv = dict(M.level("full"))
    pip, pix = lv["PT"][0], lv["PT"][1].copy()
    for a in range(lv["m"]):
        pix[pip[a]:pip[a + 1]] = pix[pip[a]:pip[a + 1]][::-1]
    lv["PT"] = (pip, pix)
    want = M.compose(lv, 2, 3, lambda A, d, X0, it: ge.embed_via_minimization(
        A, d, coords=X0, iterations=it))
    assert M.same(run_level(lv, 2, iterations=3), want)


def test_live_reference_composition():
    import ref_lib as R
    if not R.available():
        pytest.skip("neither the reference tree nor a built oracle/_ref/ge_ref is here")
    lv = M.level("full")
    want = M.compose(lv, 3, 4, lambda A, d, X0, it: R.embed_via_minimization(
        A, d, coords=X0, iterations=it))
    assert M.same(run_level(lv, 3, iterations=4), want)


def test_zero_iterations_and_empty_level():
    lv = M.level("small")
    X = run_level(lv, 2, iterations=0)
    assert np.isnan(X).all()  # a zero embedding has no largest norm: 0 / 0 everywhere
    e = np.zeros(0, np.int32)
    X = ge.embed_via_minimization_ml((np.zeros(1, np.int32), e), (np.zeros(1, np.int32), e), e,
                                     np.zeros((0, 2)), np.zeros(0), 2)
    assert X.shape == (0, 2)


def test_argument_errors():
    lv = M.level("small")
    A, PT, vA, cA, rA = lv["A"], lv["PT"], lv["vA"], lv["cA"][2], lv["rA"]
    call = ge.embed_via_minimization_ml
    with pytest.raises(ge.GeError):
        call(A, PT, vA, cA, rA, 0, iterations=1)  # dim
    with pytest.raises(ge.GeError):
        call(A, PT, vA, cA, rA, 2, iterations=-1)
    with pytest.raises(ge.GeError):
        call(A, PT, vA, cA[:-1], rA, 2, iterations=1)  # sizes
    bad = vA.copy()
    bad[PT[1][0]] = (bad[PT[1][0]] + 1) % lv["m"]
    with pytest.raises(ge.GeError, match="vertex_A"):
        call(A, PT, bad, cA, rA, 2, iterations=1)
    twice = PT[1].copy()
    twice[1] = twice[0]
    with pytest.raises(ge.GeError):
        call(A, (PT[0], twice), vA, cA, rA, 2, iterations=1)
    short = PT[0].copy()
    short[-1] -= 1
    with pytest.raises(ge.GeError):
        call(A, (short, PT[1]), vA, cA, rA, 2, iterations=1)
    cols = A[1].copy()
    cols[0] = lv["n"]
    with pytest.raises(ge.GeError, match="column"):
        call((A[0], cols), PT, vA, cA, rA, 2, iterations=1)


def test_dropin_embedder_compiles(tmp_path):
    """minimizationToMultilevel composes with embedVia under -Wall -Wextra -Werror."""
    assert os.path.exists(build_driver(tmp_path))
