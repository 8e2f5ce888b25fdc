"""The CSR row pass on the device (graph-embed_amd/csrc/ge_rows.hpp) against the oracle, on
the rows of tests/rows_cases.py (proved on the CPU by tests/test_rows_cases.py).

Every case runs FaPlan.attract and compares FaPlan.forces() -- the row's force itself,
where x_next = F speed + x hides a last-place error about half the time -- and x_next
with oracle.fa_step_rows_frep bit for bit, and FaPlan.rows_info() with the classes the
rows are built for; heavy rows also with how the pass must have finished them (the
binade sum, or the serial sum and why).  The multilevel stored-term chains run through
force_atlas_ml with the census of FamlPlan.classes()."""
import numpy as np
import pytest

import rows_cases as R
from faml_plan import run_plan

pytestmark = pytest.mark.gpu

_wants = {}


def _want(oracle, key, A, X, passes, rb, re, **kw):
    """The oracle's (force rows, x_next rows) of consecutive passes over rows [rb, re),
    computed once per key and never modified."""
    if key not in _wants:
        deg = oracle.degrees(A)
        fprev = np.zeros((re - rb, X.shape[1]))
        out = []
        for frep in passes:
            xn = X.copy()
            oracle.fa_step_rows_frep(A, X, deg, rb, re, frep, fprev, xn, **kw)
            res = (fprev.copy(), xn[rb:re].copy())
            for a in res:
                a.setflags(write=False)
            out.append(res)
        _wants[key] = out
    return _wants[key]


def _device(ctx, A, X, passes, rb, re, **kw):
    """The same passes on one plan: [(forces, x_next rows, rows_info)]."""
    import torch
    dev = torch.device("cuda:0")
    n, d = X.shape

    def up(a, dt):
        # a copy: the cases' arrays are read-only
        return torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)

    ip, ix, dx, x = up(A[0], np.int32), up(A[1], np.int32), up(A[2], np.float64), up(X, np.float64)
    y = torch.zeros_like(x)
    f = torch.zeros((max(re - rb, 1), d), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    plan = ctx.fa_plan(n, int(A[0][-1]), ip.data_ptr(), ix.data_ptr(), dx.data_ptr(), d, rb, re,
                       **kw)
    out = []
    try:
        before = plan.rows_info()
        assert (before["heavy_status"] == (R.WHOLE if before["seg_mode"] == 0 else R.NONE)).all()
        for frep in passes:
            fr = up(frep, np.float64)
            plan.attract(x.data_ptr(), fr.data_ptr(), y.data_ptr())
            plan.forces(f.data_ptr())
            ctx.sync()
            out.append((f[:re - rb].cpu().numpy(), y[rb:re].cpu().numpy(), plan.rows_info()))
    finally:
        plan.close()
    return out


def _check(got, want, census):
    for (F, xn, info), (wF, wxn) in zip(got, want):
        assert R.same_bits(F, wF), np.argwhere(F.view(np.uint64) != wF.view(np.uint64))[:8]
        assert R.same_bits(xn, wxn)
        assert {k: info[k] for k in census} == census, info


def _status(info):
    return dict(zip(info["heavy_rows"].tolist(), info["heavy_status"].tolist()))


def _tile_env(monkeypatch, tiles="1", segments=None):
    monkeypatch.setenv("GE_ROWS_TILES", tiles)
    for k in ("GE_ROWS_MED", "GE_ROWS_HEAVY", "GE_ROWS_SERIAL"):
        monkeypatch.delenv(k, raising=False)
    if segments is None:
        monkeypatch.delenv("GE_ROWS_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("GE_ROWS_SEGMENTS", segments)


BINADE_KW = dict(gravity=0.0, ksmax=R.KSMAX)


# --------------------------------------------------------------------------
# binade sums

@pytest.mark.parametrize("d", R.DIMS)
def test_binade_rows(ctx, oracle, monkeypatch, d):
    """Every binade row: the force and x_next on bits, and the finish the row is built
    for -- the binade sum one unit inside each end of the binade, the serial sum at
    m - A = 2^52 and m + A = 2^53 exactly, on a real crossing, on a tie wherever it sits,
    on a term of 2^36 units (2^36 - 1 is summed), a non-finite term, and on every base
    that is not a normal number."""
    _tile_env(monkeypatch)
    g = R.binade_case(d)
    deg = np.diff(g["A"][0])
    want = _want(oracle, ("binade", d), g["A"], g["X"], [g["frep"]], 0, g["n"], **BINADE_KW)
    got = _device(ctx, g["A"], g["X"], [g["frep"]], 0, g["n"], **BINADE_KW)
    _check(got, want, R.census(deg, tiles=True))
    st = _status(got[0][2])
    bad = {r.name: (st[r.hub], r.expect) for r in g["rows"] if st[r.hub] != r.expect}
    assert not bad, bad


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("order", ["tie-first", "tie-second"])
def test_binade_state_between_passes(ctx, oracle, monkeypatch, d, order):
    """Two passes on one plan: the rows' frep, under which the tie rows tie, and twice
    it, under which no row ties (u doubles).  The second pass's status and bits must not
    remember the first: hflag and hacc are cleared by heavy_finish_kernel."""
    _tile_env(monkeypatch)
    g = R.binade_case(d)
    with np.errstate(over="ignore"):  # the largest finite base becomes inf
        f1, f2 = g["frep"], 2.0 * g["frep"]
    passes = [f1, f2] if order == "tie-first" else [f2, f1]
    want = _want(oracle, ("state", d, order), g["A"], g["X"], passes, 0, g["n"], **BINADE_KW)
    got = _device(ctx, g["A"], g["X"], passes, 0, g["n"], **BINADE_KW)
    _check(got, want, R.census(np.diff(g["A"][0]), tiles=True))
    for (_, _, info), frep in zip(got, passes):
        st = _status(info)
        for r in g["rows"]:
            model = R.binade_formula(frep[r.hub], R.row_terms(g["A"], g["X"], r.hub))[0]
            assert st[r.hub] == model, (r.name, st[r.hub], model)
            if r.name.startswith("tie-"):
                assert model == (R.FLAG if frep is f1 else R.BINADE)


def test_binade_row_shard(ctx, oracle, monkeypatch):
    """A plan over [rb, n) with rb > 0: Frep and Fprev are indexed by row - rb."""
    _tile_env(monkeypatch)
    g = R.binade_case(2)
    rb, n = 5, g["n"]
    frep = g["frep"][rb:]
    want = _want(oracle, ("shard", 2), g["A"], g["X"], [frep], rb, n, **BINADE_KW)
    got = _device(ctx, g["A"], g["X"], [frep], rb, n, **BINADE_KW)
    _check(got, want, R.census(np.diff(g["A"][0])[rb:], tiles=True))
    st = _status(got[0][2])
    assert sorted(st) == [r.hub for r in g["rows"] if r.hub >= rb]
    assert all(st[r.hub] == r.expect for r in g["rows"] if r.hub >= rb)


def test_binade_rows_whole(ctx, oracle, monkeypatch):
    """GE_ROWS_SEGMENTS=0: the same rows whole, one block each: serial, no segments."""
    _tile_env(monkeypatch, segments="0")
    g = R.binade_case(3)
    want = _want(oracle, ("binade", 3), g["A"], g["X"], [g["frep"]], 0, g["n"], **BINADE_KW)
    got = _device(ctx, g["A"], g["X"], [g["frep"]], 0, g["n"], **BINADE_KW)
    _check(got, want, R.census(np.diff(g["A"][0]), tiles=True, segments=False))
    assert set(_status(got[0][2]).values()) == {R.WHOLE}


# --------------------------------------------------------------------------
# structure

@pytest.mark.parametrize("d,segments", [(d, "1") for d in R.TILE_DIMS] + [(3, "0")])
def test_tile_edges(ctx, oracle, monkeypatch, d, segments):
    """Tiles closed at exactly 512 entries, by the 65th row, with leading, trailing and
    only empty rows, rows on a thread's second entry slot, lane_chain_any's blocks of 8
    with and without a tail, and rows of 513 and 1025 entries as segments or (once)
    whole on the side stream."""
    _tile_env(monkeypatch, segments=segments)
    A, _ = R.tiles_graph()
    n = len(A[0]) - 1
    X, frep = R.structure_inputs(A, d, seed=d)
    want = _want(oracle, ("tiles", d), A, X, [frep], 0, n)
    got = _device(ctx, A, X, [frep], 0, n)
    _check(got, want, R.census(np.diff(A[0]), tiles=True, segments=segments == "1"))


@pytest.mark.parametrize("d", R.CLASSED_DIMS)
def test_classed_edges(ctx, oracle, monkeypatch, d):
    """Light | medium at 4 | 5, the wave's stride of 64, the heavy cut at 2048 | 2049 and
    the split sum's chunk edges (768, 384 or 192 terms) with lane_chain's pair of blocks
    and its remainder loop."""
    _tile_env(monkeypatch, tiles="0")
    A, _ = R.classed_graph()
    n = len(A[0]) - 1
    X, frep = R.structure_inputs(A, d, seed=d)
    want = _want(oracle, ("classed", d), A, X, [frep], 0, n)
    got = _device(ctx, A, X, [frep], 0, n)
    _check(got, want, R.census(np.diff(A[0]), tiles=False))
    assert set(_status(got[0][2]).values()) == {R.WHOLE}


_natural = {}


@pytest.mark.parametrize("rows", R.NATURAL_PLANS)
def test_natural_thresholds(ctx, oracle, monkeypatch, rows):
    """No environment override: 65 535 rows are classed (medium above 4 entries), 65 536
    and 65 537 are tiled, their heavy rows (above 512 entries) as binade segments."""
    for k in ("GE_ROWS_TILES", "GE_ROWS_MED", "GE_ROWS_HEAVY", "GE_ROWS_SEGMENTS", "GE_ROWS_SERIAL"):
        monkeypatch.delenv(k, raising=False)
    if not _natural:
        A, _ = R.natural_graph()
        _natural["A"] = A
        _natural["X"], _natural["frep"] = R.structure_inputs(A, 3, seed=5)
    A, X, frep = _natural["A"], _natural["X"], _natural["frep"][:rows]
    want = _want(oracle, ("natural", rows), A, X, [frep], 0, rows)
    got = _device(ctx, A, X, [frep], 0, rows)
    census = R.census(np.diff(A[0])[:rows])
    assert (census["ntiles"] > 0) == (rows >= R.TILE_MIN_ROWS)
    _check(got, want, census)


# --------------------------------------------------------------------------
# multilevel: stored terms and the chain kernels

_ml_wants = {}


def _ml_want(oracle, which, dim):
    if (which, dim) not in _ml_wants:
        case = R.ml_case(which, dim)
        x = oracle.force_atlas_ml(case["A"], case["PT"], case["vA"], case["cA"], case["rA"], dim,
                                  iterations=case["iterations"], seed=case["seed"], **case["kw"])
        x.setflags(write=False)
        _ml_wants[(which, dim)] = (case, x)
    return _ml_wants[(which, dim)]


ML_RUNS = [(w, 3, v) for w in R.ML_PLANS for v in ("overlap", "serial", "whole")] + [
    ("both", 1, "overlap"), ("both", 4, "overlap")]


@pytest.mark.parametrize("which,dim,variant", ML_RUNS, ids=["-".join(map(str, r)) for r in ML_RUNS])
def test_ml_stored_term_chains(ctx, oracle, monkeypatch, which, dim, variant):
    """Member rows of 513, 767 | 768 | 769 and 8191 entries (late chains, 256 / 8) and of
    8192 | 8193, 8192 + 31 | 32 | 33 (early chains, 512 / 16) in a streamed aggregate: plans
    whose heavy rows are all late, all early, and both; on the two streams, one after
    the other (GE_ROWS_SERIAL=1) and as whole rows (GE_ROWS_SEGMENTS=0)."""
    monkeypatch.setenv("GE_ROWS_TILES", "1")
    monkeypatch.setenv("GE_FAML_RES_CAP", R.ML_RES_CAP)
    for k in ("GE_ROWS_MED", "GE_ROWS_HEAVY", "GE_ROWS_SERIAL", "GE_ROWS_SEGMENTS"):
        monkeypatch.delenv(k, raising=False)
    if variant == "serial":
        monkeypatch.setenv("GE_ROWS_SERIAL", "1")
    elif variant == "whole":
        monkeypatch.setenv("GE_ROWS_SEGMENTS", "0")
    case, want = _ml_want(oracle, which, dim)
    got, cls, _ = run_plan(ctx, case)
    census = R.ml_census(case, segments=variant != "whole")
    assert cls["streamed"] == 1 and cls["ntiles"] > 0, cls
    assert {k: cls[k] for k in census} == census, cls
    assert np.array_equal(got, want)
