"""CPU checks of the single-level FAST repulsion inputs (tests/fa_fast_cases.py): the
sizes sit on the kernel's edges, the degenerate vertices are where the formulas say, and
a float64 numpy restatement of the kernel's order meets the bound of that module's
docstring on every input -- the inputs and the bound are sound before a device is
involved (tests/test_gpu_fa_fast.py holds fa_repulse_fast to the same bound).

Largest error / bound of the restatement over the 7 cases of an input (each case prints
its figure before it asserts): 0.138 at n = 2 and 0.065 at n = 5 (few terms: the term
error dominates), 0.046-0.058 at n = 255..257, 0.017-0.020 at n = 1 023..1 025 and 0.005-0.006
at n = 4 096, 4 097 (the worst case n u of the chains dominates the bound, random roundings
use ~sqrt(n) u of it); the degenerate inputs 0.048 / 0.016 / 0.005 at n = 257 / 1 025 /
4 097; 0.015 at x1e9 and 0.008 at x1e-300 (every pair clamped).
"""
import numpy as np
import pytest

import fa_fast_cases as C


def test_sizes_sit_on_the_kernel_edges():
    for n in C.SIZES:
        C.case(n)  # asserts chunking(n) == EXPECT[n] and the sha256
        jb, jchunk = C.chunking(n)
        assert 1 <= jb <= C.FAST_JBLOCKS and jb * jchunk >= n > (jb - 1) * jchunk
    assert C.ROW_BLOCK == 1024
    assert [C.chunking(n)[0] for n in (255, 256, 257)] == [1, 1, 2]
    assert C.chunking(257)[1] == 129  # two ragged tiles
    assert C.slot_of(1023) == (0, 3, 255) and C.slot_of(1024) == (1, 0, 0)
    assert [C.chunking(n)[0] for n in (1024, 1025)] == [4, 5]
    assert C.chunking(4096) == (16, C.TILE_J)  # every chunk exactly one tile
    assert C.chunking(4097) == (16, C.TILE_J + 1)  # a full tile and a tile of one
    assert -(-4097 // C.TILE_J) == 17 > C.FAST_JBLOCKS
    assert C.chunk_of(256, 4097) == (0, 1) and C.chunk_of(257, 4097) == (1, 0)


@pytest.mark.parametrize("n", C.SIZES)
def test_graph(n):
    ip, ix, dx = C.case(n)[0]
    assert len(ip) == n + 1 and ip[-1] == len(ix) == len(dx)
    rows = np.repeat(np.arange(n), np.diff(ip))
    assert (rows != ix).all()
    key = rows.astype(np.int64) * n + ix
    back = ix.astype(np.int64) * n + rows
    assert len(np.unique(key)) == len(key)
    assert np.array_equal(np.sort(key), np.sort(back))  # symmetric pattern
    w = dict(zip(key.tolist(), dx.tolist()))
    assert all(w[b] == x for b, x in zip(back.tolist(), dx.tolist()))  # symmetric weights
    for r in range(n):
        assert (np.diff(ix[ip[r]:ip[r + 1]]) > 0).all()
    if n >= 2:
        assert (np.diff(ip) >= 1).all()  # the ring: no isolated vertex
        assert (dx != np.round(dx)).any()
        assert not np.array_equal(C.masses(n, 1), C.masses(n, 0))  # use_weights matters
    assert (C.masses(n, 1) >= 1).all() and (C.masses(n, 0) >= 1).all()


@pytest.mark.parametrize("n", C.DEGENERATE)
@pytest.mark.parametrize("d", C.DIMS)
def test_degenerate_placement(n, d):
    twin_a, twin_b, near_a, near_b, origin = C.placement(n)
    X, plain = C.coords(n, d, "degenerate"), C.coords(n, d)
    assert np.array_equal(X[twin_a], X[twin_b])
    gap = np.sqrt(((X[near_a] - X[near_b]) ** 2).sum())
    assert 0.0 < gap < C.KFAEPS and abs(gap - 0.25 * C.KFAEPS) < 1e-12
    assert not X[origin].any()
    other = np.ones(n, bool)
    other[[twin_b, near_b, origin]] = False
    assert np.array_equal(X[other], plain[other])


def test_scaled_inputs():
    n = C.SCALED
    for d in C.DIMS:
        X = C.coords(n, d)
        big, tiny = C.coords(n, d, "x1e9"), C.coords(n, d, "x1e-300")
        assert np.array_equal(big, X * 1e9) and np.array_equal(tiny, X * 1e-300)
        e = tiny[:, None, :] - tiny[None, :, :]
        assert not (e * e).any()  # every squared difference underflows: every pair clamped
        assert np.isfinite(big * big).all()  # far inside the domain of include/ge.h


def test_reference_clamp_and_self_pair():
    """The long-double reference on the degenerate input against a plain double loop, and
    its clamp: the coincident pair contributes nothing, the near pair is divided by
    eps^3, a single vertex has no force."""
    n, d, repel = 257, 2, 3.5
    X, m = C.coords(n, d, "degenerate"), C.masses(n, 1)
    Fr, T = C.reference(n, "degenerate", d, repel, 1)
    twin_a, twin_b, near_a, near_b, origin = C.placement(n)
    for i in (twin_a, near_b, origin, 0):
        acc = np.zeros(d)
        for j in range(n):
            if j == i:
                continue
            e = X[i] - X[j]
            dis = max(float(np.sqrt((e * e).sum())), C.KFAEPS)
            acc += e / dis * (m[i] * m[j] * repel / (dis * dis))
        assert np.allclose(np.asarray(Fr[i], dtype=np.float64), acc, rtol=1e-12, atol=0)
    assert (T >= np.abs(Fr)).all()
    t = 0.25 * C.KFAEPS * m[near_a] * m[near_b] * repel / C.KFAEPS ** 3
    assert T[near_b, 0] > t * (1 - 1e-9)
    # the coincident pair adds exactly 0, like the self pair
    F2, T2 = C.FAR.pair_sums(X[[twin_a]], m[[twin_a]] * repel, X[[twin_b, twin_a]],
                             m[[twin_b, twin_a]])
    assert not F2.any() and not T2.any()
    F1, T1 = C.reference(1, "plain", 3, 1.0, 1)
    assert not F1.any() and not T1.any()


@pytest.mark.parametrize("dim,repel,use_weights", C.CASES, ids=C.CASE_IDS)
@pytest.mark.parametrize("n,variant", C.INPUTS, ids=C.INPUT_IDS)
def test_restatement_meets_the_bound(n, variant, dim, repel, use_weights):
    X, m = C.coords(n, dim, variant), C.masses(n, use_weights)
    Fr, T = C.reference(n, variant, dim, repel, use_weights)
    got = C.restate(X, m, repel)
    assert np.isfinite(got).all()
    worst, ok = C.ratio(got, n, Fr, T)
    print(f"restatement n={n} {variant} {dim=} {repel=} {use_weights=}: "
          f"max |F - F*| / bound = {worst:.4f}")
    assert (T > 0).all() == (n > 1)  # rows without a term only at n = 1
    if n == 1:
        assert not got.any()
    assert ok, worst
