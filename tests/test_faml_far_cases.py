"""CPU checks of tests/faml_far_cases.py: the per-aggregate restatement of the multilevel
far field (tests/far_cases.py applied to one aggregate's members, Morton keys of
faml_far_cases.key_bits(d) bits per axis) is a valid approximation on the level the device
tests use, and the inputs are not trivial.  The bound and its derivation are in
tests/test_far_cases.py's docstring; here d_i is (internal deg_i + 1) repel and the exact
sum is include/forceatlas.hpp:394-410 over the aggregate's members.
"""
import numpy as np
import pytest

import far_cases as F
import faml_far_cases as C

ROWS, THETA = 64, 0.5


@pytest.fixture(scope="module")
def layouts():
    """{(aggregate, d): (X, m, layout)} of every streamed aggregate, built once."""
    out = {}
    m = C.masses()
    for a in C.STREAMED:
        b, e = C.span(a)
        for d in C.DIMS:
            X = C.level()["X"][d][b:e]
            out[a, d] = (X, m[b:e], C.own_layout(X, m[b:e], ROWS, THETA, C.key_bits(d)))
    return out


def test_inputs():
    lv = C.level()
    assert lv["n"] == sum(C.SIZES)
    assert all(C.masses()[slice(*C.span(a))].min() > 1.0 for a in C.STREAMED)
    assert (lv["A"][2] != np.round(lv["A"][2])).any()
    pip, pix = lv["PT"]
    for a in C.STREAMED:  # no aggregate is a contiguous range of vertex ids
        v = pix[pip[a]:pip[a + 1]]
        assert (np.diff(v) > 0).all() and (np.diff(v) > 1).sum() > len(v) // 8
    assert [C.key_bits(d) for d in C.DIMS] == [41, 20, 13, 10]
    shapes = {s: [c for c, _ in F.level_shape(s)] for s in C.SIZES if s > 256}
    assert shapes == {257: [5], 1024: [16], 300: [5], 1025: [17, 2], 4097: [65, 5],
                      16449: [258, 17, 2]}
    assert C.far_aggs(257) == [8, 7, 6, 4, 5, 0] and C.far_aggs(1025) == [8, 7, 6]
    assert C.fast_items() == 2 + 4 + 2 + 5 + 17 + 65 and C.fast_items(1025) == 2 + 4 + 2


@pytest.mark.parametrize("d", C.DIMS)
def test_layout_orders_each_aggregate(layouts, d):
    for a in C.STREAMED:
        X, m, lay = layouts[a, d]
        s = len(X)
        assert np.array_equal(np.sort(lay["perm"]), np.arange(s))
        k = lay["keys"]
        assert (k[1:] >= k[:-1]).all() and int(k.max()) < 1 << (d * C.key_bits(d))
        tie = k[1:] == k[:-1]
        assert (lay["perm"][1:][tie] > lay["perm"][:-1][tie]).all()
        for q in C.sample_items(s, ROWS):  # a walk covers the aggregate once, in order
            at = 0
            for l, idx, _ in F.walk(lay, q, s):
                lo, hi = F.cell_range(l, idx, s)
                assert lo == at
                at = hi
            assert at == s


@pytest.mark.parametrize("d", C.DIMS)
def test_restatement_meets_the_bound(layouts, d):
    worst = 0.0
    for a in C.STREAMED:
        X, m, lay = layouts[a, d]
        mom = F.cell_moments(lay, X, m)
        for q in C.sample_items(len(X), ROWS):
            pos, Fa, T, terms, order = F.replay_item(lay, q, X, m, 1.0)
            ids = lay["perm"][pos]
            Fx, _ = F.exact_rows(X, m, 1.0, ids)
            err = np.sqrt(((Fa - Fx) ** 2).sum(axis=1))
            bound = F.truncation_bound(lay, order, mom, X[ids], m[ids]) + F.rounding(T, terms)
            assert (err <= bound).all(), (a, q)
            if any(acc for _, _, acc in order):
                worst = max(worst, float((err / bound).max()))
    print(f"d = {d}: largest error / bound {worst:.3f}")
    assert worst > 0.0  # something was approximated


def test_every_level_accepts_a_cell(layouts):
    """theta = 0.5, 64-row items: accepted cells per level of every streamed aggregate.
    At d <= 3 every aggregate accepts at least one cell at every level of its hierarchy --
    except the 300-member one at d = 2 and d = 3, which accepts none: its 5 leaves of
    uniform points overlap every item's ball (so do those of 39 other coordinate seeds
    tried; 257 members accept 3 cells, 1024 members 2 at d = 3).  At d = 4 the aggregates
    of 300 and 1024 members accept nothing and the others not much: the figures are
    printed, and the leaf and top levels of the two largest are asserted."""
    none = []
    for d in C.DIMS:
        for a in C.STREAMED:
            X, m, lay = layouts[a, d]
            acc, leaves, terms = F.accepted_counts(lay, len(X))
            print(f"d = {d} s = {len(X)}: accepted {acc}, exact leaves {leaves}, terms {terms}")
            if min(acc) == 0:
                none.append((d, len(X)))
            else:
                assert terms <= len(X) * (len(X) - 1)  # = : only the one-point leaf was taken
            if d == 4 and len(X) >= 4097:
                assert acc[0] > 0 and acc[-1] > 0, (d, len(X), acc)
    assert [x for x in none if x[0] <= 3] == [(2, 300), (3, 300)], none
    assert [x for x in none if x[0] == 4] == [(4, 1024), (4, 300)], none


def test_degenerate_variant():
    m = C.masses()
    for d in C.DIMS:
        X = C.degenerate(d)
        b, e = C.span(C.A4097)
        lay = C.own_layout(X[b:e], m[b:e], ROWS, THETA, C.key_bits(d))
        assert lay["cells"][0][0, d + 1] == 0.0  # the clump's leaf
        assert np.array_equal(np.sort(lay["perm"][:70]), np.arange(100, 170))
        assert np.array_equal(X[b + 10], X[b + 11])
        assert 0 < np.abs(X[b + 20] - X[b + 21]).max() < F.KFAEPS
        b, e = C.span(C.A1025)
        lay = C.own_layout(X[b:e], m[b:e], ROWS, THETA, C.key_bits(d))
        assert lay["box"][d] == 0.0 and not lay["keys"].any()  # scale 0: P_T order
        assert np.array_equal(lay["perm"], np.arange(e - b))
        assert all(not acc for q in (0, 16) for _, _, acc in F.walk(lay, q, e - b))
