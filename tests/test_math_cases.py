"""The directed operand families of tests/math_cases.py, checked on the CPU: the
exact reference against the host's own IEEE `/` and sqrt (which the oracle uses),
every operand inside the domain the strict kernels admit, every geometry exactly
what it claims to be, and every family at its promised size.  This is what lets
tests/test_gpu_math_exact.py compare the device with the reference alone.
"""
import math

import numpy as np
import pytest

import graphs as G
import math_cases as M
import pyref


def test_exact_reference_itself():
    """exact_sqrt and exact_div on values whose rounding is known by hand."""
    assert M.exact_sqrt(4.0) == 2.0 and M.exact_sqrt(2.0) == math.sqrt(2.0)
    assert M.exact_sqrt(2.0 ** -504) == 2.0 ** -252 and M.exact_sqrt(2.0 ** 405) == math.sqrt(2.0 ** 405)
    # sqrt(1 - 2^-53) = 1 - 2^-54 - ...: the midpoint of 1 - 2^-53 and 1, less a bit
    assert M.exact_sqrt(1.0 - 2.0 ** -53) == 1.0 - 2.0 ** -53
    # sqrt(1 + 2^-52) = 1 + 2^-53 - 2^-107...: just below the midpoint of 1 and 1 + 2^-52
    assert M.exact_sqrt(1.0 + 2.0 ** -52) == 1.0
    # the issue's example: 0.5 / (1 - 2^-53) = 0.5 + 2^-54 + 2^-107...: just above a midpoint
    assert M.exact_div(0.5, 1.0 - 2.0 ** -53) == 0.5 + 2.0 ** -53
    assert M.midpoint_distance(0.5, 1.0 - 2.0 ** -53) < M.NEAR
    assert M.midpoint_distance(1.0, 3.0) > 2.0 ** -56
    z = M.exact_div(-0.0, 2.0)
    assert z == 0.0 and math.copysign(1.0, z) == -1.0


def test_family_sizes():
    """No family is filtered when it is built: each has the size its definition gives."""
    assert len(M.DENOMINATORS) == M.N_DENOMINATORS == 137
    assert len(set(M.DENOMINATORS)) == 137
    assert len(M.HARD_SQUARE_NORMS) == 27
    assert len(M.DIV_N) == len(M.DIV_D) == M.N_DIV == 137 * 4375
    assert len(M.SQRT_S) == M.N_SQRT == 1612
    assert len(M.PAIR_S) == len(M.PAIR_N) == len(M.PAIR_C) == M.N_PAIR == 144447
    assert len(M.GEOMETRIES) == M.N_GEOMETRIES == 24 * 12
    for dim in (1, 2, 3, 4):
        assert len(M.rep_cases(dim)) == M.N_REP[dim]
    assert M.N_REP == {1: 296, 2: 576, 3: 576, 4: 576}
    sigs = {M._sig(d) for d in M.DENOMINATORS}
    assert set(M.HIGH_SIGS) | set(M.LOW_SIGS) <= sigs
    for E in (-17, -3, -1, 0, 5, 52, 201):  # the binades the families must reach
        assert any(M.binade(d) == E for d in M.DENOMINATORS), E
    assert M.EPS in M.DENOMINATORS
    # the integers 1..4096 over every hard square, and every one of them over some norm
    assert set(M.PAIR_C) == {float(k) for k in M.INTS}
    for dis in M.HARD_SQUARE_NORMS:
        assert M._sig(dis * dis) in M.HIGH_SIGS + M.LOW_SIGS
        assert (M.PAIR_S == dis * dis).sum() == len(M.INTS)
    # 2^53 - 1 (all ones) is no double's rounded square: a significand pattern's square
    # depends on the exponent's parity alone, and neither parity reaches it
    got = {M._sig(d * d) for d in M.HARD_SQUARE_NORMS}
    assert got == ({2 ** 53 - k for k in (2, 4, 7)} | {2 ** 52 + k for k in (1, 2, 3, 5, 6, 8)})


def test_reference_equals_host_arithmetic():
    """The exact reference and the host's `/` and sqrt agree on every case: the
    generator is right, and the oracle's arithmetic is correctly rounded here."""
    assert np.array_equal(M.bits(M.div_reference()), M.bits(M.DIV_N / M.DIV_D))
    assert np.array_equal(M.bits(M.sqrt_reference()), M.bits(np.sqrt(M.SQRT_S)))
    dis = np.maximum(np.sqrt(M.PAIR_S), M.EPS)
    host = np.stack([dis, M.PAIR_N / dis, M.PAIR_C / (dis * dis)], axis=1)
    assert np.array_equal(M.bits(M.pair_reference()), M.bits(host))
    for dim in (1, 2, 3, 4):
        rows = M.rep_cases(dim)
        xi, xj = rows[:, :dim], rows[:, dim:2 * dim]
        e = xi - xj
        s = e[:, 0] * e[:, 0]
        for k in range(1, dim):
            s = s + e[:, k] * e[:, k]
        d = np.maximum(np.sqrt(s), M.EPS)
        val = rows[:, 2 * dim] * rows[:, 2 * dim + 1] * rows[:, 2 * dim + 2] / (d * d)
        host = (e / d[:, None]) * val[:, None]
        assert np.array_equal(M.bits(M.rep_reference(rows, dim)), M.bits(host)), dim


def test_operands_lie_in_the_kernels_domain():
    """coord_ok, weight_ok, exact_den (ge_math.hpp) restated: nothing exercises the
    out-of-domain `/` fallback without saying so."""
    for d in M.DENOMINATORS + M.HARD_SQUARE_NORMS:
        assert M.norm_ok(d) and M.exact_den(d) and M.exact_den(d * d), M.hexf(d)
    for n, d in zip(M.DIV_N[::7].tolist() + M.DIV_N[-4375:].tolist(),
                    M.DIV_D[::7].tolist() + M.DIV_D[-4375:].tolist()):
        assert M.quotient_ok(n, d), (M.hexf(n), M.hexf(d))
    # every numerator family of every binade (the families repeat per denominator)
    for E in set(M.HIGH_BINADES + M.LOW_BINADES):
        d = next(x for x in M.DENOMINATORS if M.binade(x) == E)
        assert all(M.quotient_ok(n, d) for n in M.numerators(d)), E
    assert M.SQRT_S.min() >= 2.0 ** -504 and M.SQRT_S.max() <= 2.0 ** 405
    assert M.PAIR_S.min() >= 2.0 ** -504 and M.PAIR_S.max() <= 2.0 ** 405
    assert all(n == 0.0 or 2.0 ** -200 <= abs(n) <= 2.0 ** 202 for n in M.PAIR_N)
    assert all(M.weight_ok(c) for c in M.PAIR_C)
    for dim in (1, 2, 3, 4):
        rows = M.rep_cases(dim)
        assert all(M.coord_ok(x) for x in rows[:, :2 * dim].reshape(-1))
        assert all(M.weight_ok(w) for w in rows[:, 2 * dim:].reshape(-1))
        assert all(M.weight_ok(r[2 * dim] * r[2 * dim + 1] * r[2 * dim + 2]) for r in rows)
        assert not (rows[:, :dim] == rows[:, dim:2 * dim]).all(axis=1).any()


def test_geometries_are_exact():
    """Every (T, e0) combination is reachable, the stored points differ by e exactly,
    and the correctly rounded root of fl(e0^2 + fl(e1^2)) is T."""
    assert all(g[2] is not None for g in M.GEOMETRIES)
    assert len({(g[0], g[1]) for g in M.GEOMETRIES}) == 288 >= 144
    for g in M.GEOMETRIES:
        T, e0, e1 = g
        assert M._sig(T) in M.HIGH_SIGS + M.LOW_SIGS and 0.0 < e0 < T and 0.0 < e1 < T
        assert M.exact_sqrt(e0 * e0 + e1 * e1) == T
        for dim in (2, 3, 4):
            a, b = M.antipodal(g, dim)
            e = a - b
            assert e[0] == e0 and e[1] == e1 and not e[2:].any() and a.any() and b.any()
            for p in (a, b):  # the gravity division: |x| = T / 2
                s = p[0] * p[0]
                for k in range(1, dim):
                    s = s + p[k] * p[k]
                assert M.exact_sqrt(s) == T / 2


def test_geometry_quotients_near_midpoints():
    """At least 72 geometries have a component quotient within 2^-100 (relative) of a
    rounding boundary; the all-ones distances (k = 1) are among them with every
    power-of-two first component."""
    assert len(M.HARD_PAIRS) == 90 >= 72
    ones = [g for g in M.HARD_PAIRS if M._sig(g[0]) == 2 ** 53 - 1]
    assert len(ones) == 18
    for T, e0, _ in ones:
        assert math.frexp(e0)[0] == 0.5 and M.midpoint_distance(e0, T) < M.NEAR
        # the exact quotient lies above the midpoint: 2^-j (1 + 2^-53 + 2^-106 ...)
        assert M.exact_div(e0, T) == math.nextafter(e0 / M.geo_scale(T), math.inf)


def test_layout_holds_the_pairs():
    X = M.layout(400, 3)
    for p, g in enumerate(M.HARD_PAIRS):
        e = X[2 * p] - X[2 * p + 1]
        assert e[0] == g[1] and e[1] == g[2] and e[2] == 0.0
    assert all(M.coord_ok(v) for v in X.reshape(-1))
    A, _ = M.crafted_fa_case(400, 3)
    ps, pd = M.pair_edges()
    assert len(ps) == 30
    for a, b in zip(ps, pd):
        assert b in A[1][A[0][a]:A[0][a + 1]] and a in A[1][A[0][b]:A[0][b + 1]]
    # the heavy pairs: joined, all-ones distances of three binades, deg + 1 inside weight_ok
    for p, w in M.HEAVY_PAIRS.items():
        assert 2 * p in ps and M._sig(M.HARD_PAIRS[p][0]) == 2 ** 53 - 1
        for a, b in ((2 * p, 2 * p + 1), (2 * p + 1, 2 * p)):
            row = slice(A[0][a], A[0][a + 1])
            assert A[2][row][A[1][row] == b] == w
            assert M.weight_ok(A[2][row].sum() + 1)
    assert len({M.geo_scale(M.HARD_PAIRS[p][0]) for p in M.HEAVY_PAIRS}) == 3


@pytest.mark.parametrize("dim", [2, 3])
def test_oracle_and_pyref_agree_on_a_crafted_layout(oracle, dim):
    """One iteration over the hard pairs: the C++ oracle and the pure-Python restatement
    give the same bits (both divide and take roots with the host's IEEE operations)."""
    n = 2 * len(M.HARD_PAIRS) + 12
    A, X0 = M.crafted_fa_case(n, dim)
    want = oracle.force_atlas(A, dim, coords=X0, iterations=1)
    ip, ix, dx = G.as_lists(A)
    got = np.array(pyref.force_atlas(ip, ix, dx, dim, coords=X0.tolist(), iterations=1))
    assert np.array_equal(M.bits(got), M.bits(want))
