"""CPU proof of tests/rows_cases.py: every row has the class it is named for, the serial
chain restated in numpy is the oracle's force bit for bit, the integer formula equals it
where the row is valid (or only nominally out of range) and DIFFERS where a condition
really fails -- the difference that makes a missing check on the device visible in the
bits -- and the structure graphs hold the degrees, tiles and classes they are built for."""
import numpy as np
import pytest

import rows_cases as R


def _oracle_forces(oracle, g, **kw):
    A, X = g["A"], g["X"]
    fprev = np.zeros_like(g["frep"])
    xn = X.copy()
    oracle.fa_step_rows_frep(A, X, oracle.degrees(A), 0, g["n"], g["frep"], fprev, xn, **kw)
    return fprev, xn


@pytest.fixture(scope="module", params=R.DIMS)
def proved(request, oracle):
    d = request.param
    g = R.binade_case(d)
    F, xn = _oracle_forces(oracle, g, gravity=0.0, ksmax=R.KSMAX)
    return d, g, F, xn


def test_binade_rows_have_their_class(proved):
    d, g, F, _ = proved
    A, X = g["A"], g["X"]
    names = [r.name for r in g["rows"]]
    assert len(set(names)) == len(names)
    for want in ("valid-low-pos", "valid-high-neg", "edge-low-neg", "edge-high-pos",
                 "cross-low-pos", "cross-high-neg", "tie-0-odd", "tie-1199-even", "tie-deg577",
                 "tie-one-dim", "large-2^36", "large-2^36-1", "large-nan", "base-subnormal"):
        assert want in names
    comps = set()
    for r in g["rows"]:
        assert r.deg > R.TILE_CAP, r.name  # heavy in tile mode
        terms = R.row_terms(A, X, r.hub)
        # the terms are what the case says: delta w in one component, +0 in the others
        for (c, dl, w), t in zip(r.terms, terms):
            if np.isfinite(dl):
                assert abs(dl) >= 2e-5 and 1.0 + dl - 1.0 == dl and X[r.hub + 0, c] == 1.0
                want = np.zeros(d)
                want[c] = dl * w
                assert np.array_equal(t.view(np.uint64), want.view(np.uint64)), (r.name, t, want)
            else:
                assert np.isnan(t).all(), (r.name, t)
        comps.update(c for c, _, _ in r.terms)
        serial = R.serial_force(r.base, terms, X[r.hub], 0.0, r.deg + 1.0)
        assert R.same_bits(serial, F[r.hub]), (r.name, serial, F[r.hub])
        status, formula = R.binade_formula(r.base, terms)
        assert status == r.expect, (r.name, status, r.expect)
        if status == R.BINADE:
            assert R.same_bits(formula, serial), r.name  # what the device will store
        if r.formula_equal is not None and status != R.BINADE:
            # what the device would store if the check that failed were missing
            bases = [R._base_of(s) for s in r.base]
            forced = R.binade_formula_unchecked(r.base, terms)
            assert all(ok for ok, _, _ in bases)
            assert R.same_bits(forced, serial) == r.formula_equal, (r.name, forced, serial)
    assert comps == set(range(d))  # the special component moves through the dimensions
    assert max(r.deg for r in g["rows"]) > 2 * R.TILE_CAP  # three segments


def test_binade_status_words_cover_every_reason(proved):
    d, g, _, _ = proved
    seen = {r.expect for r in g["rows"]}
    assert {R.BINADE, R.FLAG, R.RANGE, R.FLAG | R.BASE} <= seen
    assert (R.FLAG | R.RANGE in seen) == (d == 1)


def test_binade_second_pass_has_no_tie(proved):
    """frep doubled: u doubles, (K + .5) u is (K / 2 + .25) u' -- the tie rows turn valid
    (the state-between-passes case of the device test)."""
    d, g, _, _ = proved
    for r in g["rows"]:
        if r.name.startswith("tie-"):
            terms = R.row_terms(g["A"], g["X"], r.hub)
            assert R.binade_formula(2.0 * np.array(r.base), terms)[0] == R.BINADE, r.name


def test_tile_groups_are_tiles():
    A, degrees = R.tiles_graph()
    deg = np.diff(A[0])
    assert list(deg[:len(degrees)]) == degrees and (deg[len(degrees):] == 0).all()
    assert set(R.TILE_DEGREES) <= set(degrees)
    c = R.classify(deg, tiles=True)
    tiles = c["tiles"]
    q = 0
    for t, (name, group) in zip(tiles, R.TILE_GROUPS[:-1]):
        assert t == list(range(q, q + len(group))), name  # the tile closes where intended
        q += len(group)
    by = {name: tiles[i] for i, (name, _) in enumerate(R.TILE_GROUPS[:-1])}
    ents = {name: int(deg[t].sum()) for name, t in by.items()}
    assert ents["exact-512"] == ents["257+255"] == ents["512"] == R.TILE_CAP
    assert len(by["65th-row"]) == len(by["64-empty"]) == len(by["leading-empty"]) == R.TILE_ROWS
    assert ents["64-empty"] == 0 and ents["65th-row"] == 64
    assert deg[by["leading-empty"][0]] == 0 and deg[by["leading-empty"][-1]] > 0
    assert deg[by["trailing-empty"][0]] > 0 and deg[by["trailing-empty"][-1]] == 0
    assert sorted(deg[c["heavy"]]) == sorted(R.TILE_HEAVY) and c["nseg"] == 2 + 3
    assert c["heavy"] == [len(degrees) - 1, len(degrees) - 2]  # longest first
    for q in range(len(deg)):  # no self loops, distinct sorted neighbours
        row = A[1][A[0][q]:A[0][q + 1]]
        assert (np.diff(row) > 0).all() and q not in row
    assert R.census(deg, tiles=True, segments=False)["seg_mode"] == 0


def test_classed_rows_sit_on_their_edges():
    A, degrees = R.classed_graph()
    deg = np.diff(A[0])
    assert list(deg[:len(degrees)]) == degrees
    c = R.classify(deg, tiles=False)
    assert not c["tiles"] and c["nseg"] == 0
    assert sorted(deg[c["heavy"]]) == sorted(k for k in degrees if k > R.HEAVY_DEG)
    assert {4}.issubset(deg[c["light"]]) and deg[c["light"]].max() == 4
    assert deg[c["med"]].min() == 5 and deg[c["med"]].max() == R.HEAVY_DEG
    for d in R.CLASSED_DIMS:
        ch = R.split_chunk(d)
        assert ch == {3: 768, 5: 384, 8: 384, 9: 192, 16: 192}[d]
        rem = {k % ch for k in degrees if k > R.HEAVY_DEG}
        assert {ch - 1, 0, 1, 31, 32, 33} <= rem, (d, rem)
    assert {63, 64, 65, 127, 128, 129} <= set(degrees)  # ordered_edge_sum<D, 1>'s stride


def test_natural_thresholds():
    A, deg = R.natural_graph()
    assert np.array_equal(np.diff(A[0]), deg) and len(deg) > R.TILE_MIN_ROWS
    a, b, c = (R.census(deg[:m]) for m in R.NATURAL_PLANS)
    assert a["ntiles"] == 0 and a["seg_mode"] == 0 and a["nheavy"] == 2  # 2049 and 2100
    assert a["nmed"] == int(((deg[:65535] > 4) & (deg[:65535] <= 2048)).sum()) > 4
    assert a["nlight"] == int((deg[:65535] <= 4).sum())
    for t in (b, c):
        assert t["ntiles"] > 1000 and t["nmed"] == t["nlight"] == 0
        assert t["nheavy"] == 4 and t["seg_mode"] == 1  # 513, 600, 2049, 2100
        assert t["nseg"] == 2 + 2 + 5 + 5


@pytest.mark.parametrize("which", list(R.ML_PLANS))
def test_ml_plans_hold_their_rows(which):
    case = R.ml_case(which)
    deg = np.diff(case["A"][0])
    assert list(deg[case["targets"]]) == list(R.ML_PLANS[which])
    assert (case["vA"][case["targets"]] == 0).all()  # members of the streamed aggregate
    c = R.ml_census(case)
    want = R.ML_PLANS[which]
    assert c["nheavy"] == len(want)  # no other member row is heavy
    assert c["nearly"] == sum(k >= R.CHAIN_EARLY for k in want)
    assert {"late": c["nearly"] == 0, "early": c["nearly"] == c["nheavy"],
            "both": 0 < c["nearly"] < c["nheavy"]}[which]
    sizes = np.diff(case["PT"][0])
    assert (sizes > int(R.ML_RES_CAP)).sum() == 1 and sizes[0] > int(R.ML_RES_CAP)
