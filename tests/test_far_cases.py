"""CPU checks of tests/far_cases.py: the numpy restatement of GE_MODE_FARFIELD is a
correct statement of the scheme, and the inputs exercise it.

The bound (include/ge.h).  Row i has d_i = (deg_i + 1) repel, the reference sums
m_j f(x_i - x_j) over j != i with f(y) = y / |y|^3 (clamped below kFaEps, which no pair of
an accepted cell reaches: acceptance requires Dist - a_I - a_C >= kFaEps and |x_i - x_j|
>= Dist - a_I - a_C).  For an accepted cell C write y0 = x_i - c_C, rho = |y0| and
x_i - x_j = y0 + h_j with h_j = c_C - x_j, |h_j| <= a*_C < rho (theta < 1, a_C >= a*_C).
Taylor about y0 with the remainder in Lagrange form along the segment, every point of
which is at least rho - a*_C from the origin:
    f(y0 + h) = f(y0) + Df(y0) h + R,   |R| <= 1/2 sup |D^2 f| |h|^2.
Df(y) = I / |y|^3 - 3 y y^T / |y|^5 has eigenvalues 1 / |y|^3 (across) and -2 / |y|^3
(along y), so |Df(y)| = 2 / |y|^3; D^2 f is minus the third derivative of 1 / |y|, whose
largest value on unit vectors is the radial one, 6 / |y|^4.  Summed with the masses,
    sum_j m_j f(y0 + h_j) - M_C f(y0) = Df(y0) sum_j m_j h_j + sum_j m_j R_j,
    | . | <= 2 mu_C / rho^3 + 3 S_C / (rho - a*_C)^4,
mu_C = |sum_j m_j (x_j - c_C)| (zero for the exact centre; the float64 c_C leaves a
rounding-sized residue, which the bound carries), S_C = sum_j m_j |x_j - c_C|^2.  Times
d_i and summed over the accepted cells this is the truncation bound.  Every evaluated
term is fast_rep_pair's, so the rounding term is the FAST test's
(terms_i + 24) u sum |t~| with terms_i the partners of row i (accepted cells count one
each): the count in tests/test_gpu_faml_fast.py's docstring does not depend on whether
a partner is a vertex or a centre, both are float64 inputs of the same instructions.
"""
import numpy as np
import pytest

import far_cases as F


def _m(n):
    return F.masses(F.case(n)[0])


def test_inputs():
    for n in F.SIZES:
        A, X = F.case(n)
        assert len(A[0]) == n + 1 and (A[2] != np.round(A[2])).any()
        assert _m(n).min() > 1.0
        for d in F.DIMS:
            assert X[d].shape == (n, d) and np.abs(X[d]).max() <= 1.0
    assert F.level_shape(4097) == [(65, 64), (5, 1024)]
    assert F.level_shape(16449) == [(258, 64), (17, 1024), (2, 16384)]
    assert F.level_shape(1 << 20) == [(16384, 64), (1024, 1024), (64, 16384), (4, 262144)]


@pytest.mark.parametrize("d", F.DIMS)
def test_walk_covers_every_point_once(d):
    """Accepted cells and exact leaves of an item partition the sorted order, in
    ascending order: the walk is the row sum's fixed order."""
    for n, rows in ((4097, 256), (16449, 64)):
        X = F.case(n)[1][d]
        lay = F.own_layout(X, _m(n), rows, 0.5)
        assert np.array_equal(np.sort(lay["perm"]), np.arange(n))
        for q in range(0, len(lay["items"]), 7 if n > 5000 else 1):
            at = 0
            for l, idx, _ in F.walk(lay, q, n):
                a, b = F.cell_range(l, idx, n)
                assert a == at
                at = b
            assert at == n


@pytest.mark.parametrize("d", F.DIMS)
def test_restatement_meets_the_bound(d):
    n, rows, theta = 4097, 256, 0.5
    A, Xs = F.case(n)
    X, m = Xs[d], _m(n)
    lay = F.own_layout(X, m, rows, theta)
    mom = F.cell_moments(lay, X, m)
    worst = 0.0
    for q in range(len(lay["items"])):
        pos, Fa, T, terms, order = F.replay_item(lay, q, X, m, 1.0)
        ids = lay["perm"][pos]
        Fx, _ = F.exact_rows(X, m, 1.0, ids)
        err = np.sqrt(((Fa - Fx) ** 2).sum(axis=1))
        bound = F.truncation_bound(lay, order, mom, X[ids], m[ids]) + F.rounding(T, terms)
        assert (err <= bound).all()
        if any(a for _, _, a in order):
            worst = max(worst, float((err / bound).max()))
    print(f"d = {d}: largest error / bound {worst:.3f}")
    assert worst > 0.0  # something was approximated


def test_inputs_are_not_trivial():
    """Shares of accepted cells, so the device test cannot pass without a far field.
    n = 4 097 with 256-row items: a share of the (item, leaf) pairs is covered by an
    accepted cell at every d, most at d = 1; n = 16 449: every level accepts a cell at
    d = 1, 2, 3 (64-row items), at d = 3 also with 256-row items, and the leaf and top
    levels at d = 4."""
    n = 4097
    share = {}
    for d in F.DIMS:
        lay = F.own_layout(F.case(n)[1][d], _m(n), 256, 0.5)
        acc, leaves, terms = F.accepted_counts(lay, n)
        total = len(lay["items"]) * 65
        share[d] = 1.0 - leaves / total
        print(f"n = {n} d = {d}: accepted {acc}, exact leaves {leaves} of {total}, terms {terms}")
        assert 0 < leaves < total and terms < n * (n - 1)
    assert share[1] > 0.5 and share[1] > share[2] > share[3] > share[4] > 0.0
    n = 16449
    for d, rows in ((1, 64), (2, 64), (3, 64), (3, 256), (4, 64)):
        lay = F.own_layout(F.case(n)[1][d], _m(n), rows, 0.5)
        acc, leaves, terms = F.accepted_counts(lay, n)
        print(f"n = {n} d = {d} rows = {rows}: accepted {acc}, exact leaves {leaves}, terms {terms}")
        assert acc[0] > 0 and acc[-1] > 0 and terms < n * (n - 1)
        if d < 4:
            assert min(acc) > 0


def test_degenerate_has_a_zero_radius_leaf():
    for d in F.DIMS:
        X = F.degenerate(d)
        lay = F.own_layout(X, _m(4097), 256, 0.5)
        assert lay["cells"][0][0, d + 1] == 0.0 and np.array_equal(np.sort(lay["perm"][:70]),
                                                                  np.arange(100, 170))
        assert np.array_equal(X[10], X[11]) and 0 < np.abs(X[20] - X[21]).max() < F.KFAEPS
