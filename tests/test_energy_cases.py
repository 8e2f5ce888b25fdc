"""The layout energy's inputs, references and bounds (tests/energy_cases.py) on the CPU: the
inputs are the hashed ones, a float64 numpy restatement of the kernels' order meets every
bound against the long-double reference (so the bounds are attainable by that order and not
tuned to the device), the restated reduction is a pure function of the row values, and the
energy is the potential of the reference's force: -dE/dx_i = F_i for a symmetric graph
with nohubs = 0, and demonstrably not under nohubs (the caveat of include/ge.h).

The gradient bar, 1e-6 of max |F_i|: central differences with h = 1e-5 in long double have a
truncation error of h^2 |E'''| / 6 ~ 1.5e-8 relative on this layout (12 points, d = 3,
smallest separation 0.46) and a rounding error of 2^-64 E / h ~ 1e-13; measured 3.2e-10
(linear and linlog: the repulsion sets both figures); with nohubs 4.2e-4 and 2.4e-4.
"""
import numpy as np
import pytest

import energy_cases as E
import fa_fast_cases as C
import ge_amd as ge


def test_inputs_are_the_hashed_ones():
    for n, _ in E.INPUTS:
        C.case(n)
    A, X = E.hub()
    lens = np.diff(A[0])
    assert set(E.HUB_ROWS) <= set(lens.tolist())
    assert [int(lens[h]) for h, _ in E.HUB_STARS] == [k for _, k in E.HUB_STARS]
    assert (A[2] < 0).sum() == 2 and (A[2] != np.round(A[2])).any()
    assert (E.masses(A, 1) > 0).all()
    for n in E.WIDE_SIZES:
        for d in E.WIDE_DIMS:
            assert E.wide_coords(n, d).shape == (n, d)
    E.grad_case()


def _check(A, X, m, p, R, T, what):
    got = E.restate(A, X, m, p)
    B = E.bounds(A, X.shape[1], T, p, abs(p["gravity"]) * np.abs(m))
    worst, ok = E.ratio(got, R, B)
    print(f"{what}: restatement, max |err| / bound = {worst:.4f}")
    assert ok, (what, worst)
    tot = E.reduce_totals(got)
    err = np.abs(tot.astype(E.LD) - R.sum(axis=0))
    assert (err <= E.totals_bound(B, T)).all(), (what, err)
    return got


# the restatement walks n partners in Python: the sizes up to 1 025 in every variant, and
# the two largest once each
@pytest.mark.parametrize("n,variant", [iv for iv in E.INPUTS if iv[0] <= 1025]
                         + [(4096, "plain"), (4097, "degenerate")])
def test_restatement_meets_the_bounds(n, variant):
    cases = E.CASES if n <= 1025 else [E.CASES[4]]
    for d, repel, w in cases:
        A = C.case(n)[0]
        R, T = E.reference(n, variant, d, repel, w)
        _check(A, C.coords(n, d, variant), C.masses(n, w), E.params(repel=repel, use_weights=w),
               R, T, f"n={n} {variant} d={d} repel={repel} w={w}")


@pytest.mark.parametrize("linlog,nohubs,delta,w", E.HUB_CASES, ids=E.HUB_IDS)
def test_restatement_meets_the_bounds_on_the_hub_input(linlog, nohubs, delta, w):
    A, X = E.hub()
    R, T = E.hub_reference(linlog, nohubs, delta, w)
    _check(A, X, E.masses(A, w), E.hub_params(linlog, nohubs, delta, w), R, T,
           f"hub linlog={linlog} nohubs={nohubs} delta={delta} w={w}")


@pytest.mark.parametrize("d", E.WIDE_DIMS)
def test_restatement_meets_the_bounds_above_four_dimensions(d):
    n = 257
    R, T = E.wide_reference(n, d)
    _check(C.case(n)[0], E.wide_coords(n, d), C.masses(n, 1), E.params(), R, T, f"n={n} d={d}")


def test_reduction_is_a_pure_function_of_the_values():
    rs = np.random.RandomState(3)
    for rows in (1, 3, 4, 5, 1023, 1024, 1025, 4097):
        v = rs.uniform(-1, 1, size=(rows, E.COLS)) * 10.0 ** rs.randint(-8, 8, size=(rows, 1))
        keep = v.copy()
        a = E.reduce_totals(v)
        assert np.array_equal(v, keep)
        assert a.tobytes() == E.reduce_totals(v.copy()).tobytes()
        # its error against the exact sum is within its own count of roundings
        exact = v.astype(E.LD).sum(axis=0)
        lim = E.LD((10 + -(-rows // E.BLOCK_ROWS)) * E.U) * np.abs(v).astype(E.LD).sum(axis=0)
        assert (np.abs(a.astype(E.LD) - exact) <= lim).all()
    # the order matters, so it is one order: a permutation changes the bits
    v = rs.uniform(-1, 1, size=(4097, E.COLS))
    assert E.reduce_totals(v).tobytes() != E.reduce_totals(v[::-1]).tobytes()
    v[7, 2] = np.nan
    t = E.reduce_totals(v)
    assert np.isnan(t[2]) and np.isfinite(np.delete(t, 2)).all()


@pytest.mark.parametrize("linlog", [0, 1])
def test_energy_is_the_potential_of_the_reference_force(linlog):
    A, X = E.grad_case()
    m = E.masses(A, 1)
    p = E.params(linlog=linlog, repel=1.5, attract=0.75, gravity=2.0)
    F = E.force_ld(A, X, m, p)
    g = E.gradient_ld(A, X, m, p)
    rel = float(np.abs(g + F).max() / np.abs(F).max())
    print(f"linlog={linlog}: max |grad E + F| / max |F| = {rel:.3e}")
    assert rel < 1e-6
    # with nohubs the reference divides row i's attraction by m_i and row j's by m_j: the
    # two halves of an edge pull with different strengths and no potential has that force
    p = E.params(linlog=linlog, repel=1.5, attract=0.75, gravity=2.0, nohubs=1)
    F = E.force_ld(A, X, m, p)
    g = E.gradient_ld(A, X, m, p)
    rel = float(np.abs(g + F).max() / np.abs(F).max())
    print(f"linlog={linlog} nohubs: max |grad E + F| / max |F| = {rel:.3e}")
    assert rel > 100 * 1e-6  # two orders above the bar the identity meets without nohubs


def test_header_declares_the_energy_calls():
    syms = ge.header_symbols()
    for name in ("ge_fa_plan_energy", "ge_layout_energy", "ge_layout_energy_dist"):
        assert name in syms and name in ge._SIGS
    assert (ge.ENERGY_REP, ge.ENERGY_ATT, ge.ENERGY_GRAV, ge.ENERGY_PAIRDIST,
            ge.ENERGY_EDGELEN) == (E.REP, E.ATT, E.GRAV, E.PAIRDIST, E.EDGELEN)
    assert ge.ENERGY_COLS == E.COLS
    t = np.array([0.0, 0.0, 0.0, 12.0, 2.0])
    assert ge.relative_edge_length(t, 4, 4) == 0.5
