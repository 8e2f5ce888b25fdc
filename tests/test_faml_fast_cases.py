"""CPU checks of the multilevel FAST-mode level (tests/faml_fast_cases.py): that the
level has the shapes the GPU tests rely on, and that it is well conditioned enough
for the per-iteration bar of tests/test_gpu_faml_fast.py to be about the kernel and
not about the dynamics."""
import numpy as np
import pytest

import faml_fast_cases as F


def test_level_shapes():
    lv = F.level()
    pip, pix = lv["PT"]
    assert list(np.diff(pip)) == F.SIZES
    assert sorted(F.SIZES[a] for a in F.STREAMED) == [257, 320, 321, 512, 575]
    assert sorted(F.SIZES[a] for a in F.RESIDENT) == [1, 7, 64, 65, 256]
    # with R rows per lane: 64 R + 1, 2 x 64 R (full items only), 2 x 64 R + 63
    assert {64 * F.R + 1, 2 * 64 * F.R, 2 * 64 * F.R + 63} <= set(F.SIZES)
    # two streamed aggregates adjacent in P_T storage
    assert F.STREAMED[:2] == [0, 1]
    # member lists interleave: ascending ids, no aggregate a contiguous range
    for a, s in enumerate(F.SIZES):
        v = pix[pip[a]:pip[a + 1]]
        assert (np.diff(v) > 0).all()
        assert s < 7 or v[-1] - v[0] > s - 1
    assert F.fast_items() == 2 + 2 + 2 + 2 + 3


def test_level_graph():
    lv = F.level()
    ip, ix, dx = lv["A"]
    n = lv["n"]
    rows = np.repeat(np.arange(n), np.diff(ip))
    key = rows.astype(np.int64) * n + ix
    back = ix.astype(np.int64) * n + rows
    assert np.array_equal(np.sort(key), np.sort(back))  # symmetric pattern
    w = dict(zip(key.tolist(), dx.tolist()))
    assert all(w[b] == x for b, x in zip(back.tolist(), dx.tolist()))  # symmetric weights
    assert (dx != np.round(dx)).any()  # fractional
    internal = lv["vA"][rows] == lv["vA"][ix]
    assert internal.any() and (~internal).any()
    # one hub with at least 200 internal neighbours, in the largest aggregate
    deg_in = np.bincount(rows[internal], minlength=n)
    hub = int(np.argmax(deg_in))
    assert deg_in[hub] >= 200 and lv["vA"][hub] == F.HUB_AGG
    # use_weights changes deg + 1
    assert not np.array_equal(F.internal_dp1(lv, 1), F.internal_dp1(lv, 0))


@pytest.mark.parametrize("dim", F.DIMS)
def test_degenerate_start(oracle, dim):
    lv = F.level()
    X = F.start(oracle, dim, degenerate=True)
    plain = F.start(oracle, dim)
    pip = lv["PT"][0]
    for a in (0, F.HUB_AGG):
        x = X[pip[a]:pip[a + 1]]
        s = len(x)
        assert np.array_equal(x[3], x[s - 1])
        gap = np.sqrt(((x[70] - x[s // 2 + 9]) ** 2).sum())
        assert 0.0 < gap < F.KFAEPS
        assert not x[64].any()
    other = np.ones(lv["n"], bool)
    for a in (0, F.HUB_AGG):
        other[pip[a]:pip[a + 1]] = False
    assert np.array_equal(X[other], plain[other])


def test_reference_sums(oracle):
    """The long-double reference against a plain double loop on one aggregate, and its
    clamp: a coincident pair contributes nothing, a pair inside eps is divided by
    eps^3."""
    lv = F.level()
    X = F.start(oracle, 2, degenerate=True)
    dp1 = F.internal_dp1(lv, 1)
    Fr, Ar = F.repulsion_reference(lv, X, dp1, 3.5)
    pip = lv["PT"][0]
    b0, b1 = int(pip[0]), int(pip[1])
    i = 70
    acc = np.zeros(2)
    for j in range(b1 - b0):
        if j == i:
            continue
        e = X[b0 + i] - X[b0 + j]
        dis = max(float(np.sqrt((e * e).sum())), F.KFAEPS)
        acc += e / dis * (dp1[b0 + i] * dp1[b0 + j] * 3.5 / (dis * dis))
    assert np.allclose(np.asarray(Fr[b0 + i], dtype=np.float64), acc, rtol=1e-12, atol=0)
    assert (Ar[b0:b1] >= np.abs(Fr[b0:b1])).all()
    near = 257 // 2 + 9
    t = 0.25 * F.KFAEPS * dp1[b0 + near] * dp1[b0 + i] * 3.5 / F.KFAEPS ** 3
    assert Ar[b0 + near, 0] > t * (1 - 1e-9)
    res = np.ones(lv["n"], bool)
    for a in F.STREAMED:
        res[pip[a]:pip[a + 1]] = False
    assert not Fr[res].any()


@pytest.mark.parametrize("dim,repel,use_weights", F.CASES, ids=F.CASE_IDS)
def test_two_iterations_are_well_conditioned(oracle, dim, repel, use_weights):
    """The condition under which the per-iteration bar (REL_TOL_FAST = 1e-5 after 1 and
    2 iterations) says something about the kernel: the oracle's own response to a
    start perturbed by relative 2^-40 stays below 1e-7 after 2 iterations, on the
    streamed members of every case.  A FAST pass perturbs each force by ~1e-16 .. 1e-14
    relative, far less than 2^-40 = 9e-13."""
    lv = F.level()
    X0 = F.start(oracle, dim)
    pert = X0 * (1.0 + 2.0 ** -40 * np.random.RandomState(dim).standard_normal(X0.shape))
    mem = F.members_of(lv, F.STREAMED)
    for it in (1, 2):
        run = lambda s: oracle.force_atlas_ml(lv["A"], lv["PT"], lv["vA"], lv["cA"][dim],
                                              lv["rA"], dim, iterations=it, init=s,
                                              repel=repel, use_weights=use_weights)
        d = F.drift(run(pert), run(X0), mem)
        print(f"oracle response to 2^-40 at {it} iteration(s), {dim=} {repel=} {use_weights=}: {d:.3e}")
        assert d < 1e-7
