"""forceAtlasMultilevel on the device: every size class, option and domain edge
against the oracle, with the census that shows which kernels ran.

Every test runs its case through ge_faml_plan_* (tests/faml_plan.py run_plan) and
asserts two things: the bits (np.array_equal against oracle/ge_oracle.cpp; the
linlog / delta cases alone carry a tolerance) and FamlPlan.classes() /
.schedule(): the size class of every aggregate, the blocks of the resident
launches, the schedule of the streamed aggregates and the classes of their rows,
computed from the sizes and the device's CU count.  A heuristic change that moves
a case onto another kernel fails the census, not silently the coverage.

Layouts (tests/ref_cases.py LAYOUTS), all with fractional symmetric weights:
  packed    the M1 sizes: faml_resident<D, 64, 64> and <D, 256, 256> packs;
  large     [1031, 700, 257, 90] under GE_FAML_RES_CAP=4096:
            faml_resident<D, 256, large_cap(D)>, one aggregate per block;
  streamed  the M2 sizes with two hub rows, under GE_FAML_RES_CAP=256, three times:
            symmetric sweeps, row blocks (faml_sym_repulse) and ordered pairs
            (faml_big_repulse); member rows through FamlRows.
"""
import numpy as np
import pytest

import graphs as G
import ref_cases as C
from faml_plan import assert_census, assert_schedule, large_cap, run_plan

pytestmark = pytest.mark.gpu

MODES = {
    "sweeps": {"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"},
    "row-blocks": {"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "1e9"},
    "ordered": {"GE_FAML_SYM": "0"},
}
CONFIGS = [("packed", None), ("large", None), ("streamed", "sweeps"), ("streamed", "row-blocks"),
           ("streamed", "ordered")]
CONFIG_IDS = [l if m is None else f"{l}-{m}" for l, m in CONFIGS]

_wants = {}


def _want(oracle, key, case, init=None):
    """The oracle's result of a case, computed once per key and never modified."""
    if key not in _wants:
        x = oracle.force_atlas_ml(case["A"], case["PT"], case["vA"], case["cA"], case["rA"],
                                  case["dim"], iterations=case["iterations"], seed=case["seed"],
                                  init=init, **case["kw"])
        x.setflags(write=False)
        _wants[key] = x
    return _wants[key]


def _setenv(monkeypatch, knob, mode=None):
    if knob is None:
        monkeypatch.delenv("GE_FAML_RES_CAP", raising=False)
    else:
        monkeypatch.setenv("GE_FAML_RES_CAP", knob)
    for k, v in MODES.get(mode, {}).items():
        monkeypatch.setenv(k, v)


def _heavy_rows(case, streamed):
    """Rows of the streamed aggregates' members longer than the classed rows' heavy
    bound (ge_rows.hpp kHeavyDeg, no tiles below 65 536 rows)."""
    deg = np.diff(case["A"][0])
    sizes = np.diff(case["PT"][0])
    members = np.concatenate([case["PT"][1][case["PT"][0][a]:case["PT"][0][a + 1]]
                              for a in range(len(sizes)) if sizes[a] in streamed] or
                             [np.zeros(0, np.int64)]).astype(np.int64)
    return int((deg[members] > 2048).sum())


def _run_layout(ctx, monkeypatch, layout, mode, case, init=None):
    """Runs a case of a layout on its kernels and asserts the census of the layout."""
    sizes, _, knob = C.LAYOUTS[layout]
    _setenv(monkeypatch, knob, mode)
    got, cls, sched = run_plan(ctx, case, init=init)
    want = assert_census(cls, sizes, case["dim"], knob)
    assert_schedule(sched, cls, want["streamed"], mode)
    if layout == "packed":
        assert not want["large"] and not want["streamed"]
        assert cls["blocks_small"] >= 2 and cls["blocks_mid"] >= 2
    elif layout == "large":
        assert want["large"] == [1031, 700, 257] and not want["streamed"]
    else:
        assert want["streamed"] == [2600, 320, 700, 257, 1031, 300] and not want["large"]
        # classed rows (fewer than 65 536): the 3 000-entry hub row whole, on the side stream
        assert (cls["ntiles"], cls["nseg"], cls["seg_mode"]) == (0, 0, 0), cls
        assert cls["nheavy"] == _heavy_rows(case, want["streamed"]) >= 1, cls
    return got


# --------------------------------------------------------------------------
# B1: size classes and their boundaries

B1 = [
    # dim, sizes, GE_FAML_RES_CAP, expected large-resident, expected streamed
    (3, [4096, 4097, 257, 300, 256, 65, 64, 1], "4096", [4096, 257, 300], [4097]),
    (4, [2048, 2049, 257, 100], "4096", [2048, 257], [2049]),
    (1, [1000, 257, 256, 65, 64, 30, 1], "4096", [1000, 257], []),
    (2, [1000, 257, 256, 65, 64, 30, 1], "4096", [1000, 257], []),
]


def _b1_case(dim, sizes):
    n = sum(sizes)
    A = C.symmetric_weights(G.rmat(n, 6 * n, seed=len(sizes) + dim))
    return C._ml(A, sizes, n, dim, 3, 41)


@pytest.mark.parametrize("dim,sizes,knob,large,streamed", B1,
                         ids=["d3-4096|4097", "d4-2048|2049", "d1-classes", "d2-classes"])
def test_size_class_boundaries(ctx, oracle, monkeypatch, dim, sizes, knob, large, streamed):
    """The resident side of the large kernel's capacity (4096 members, 2048 at dim 4:
    8-double records) next to the streamed side one member above it, and the 256|257
    and 64|65 boundaries, under GE_FAML_RES_CAP=4096 (clamped to the capacity)."""
    _setenv(monkeypatch, knob)
    case = _b1_case(dim, sizes)
    got, cls, sched = run_plan(ctx, case)
    want = assert_census(cls, sizes, dim, knob)
    assert cls["res_cap"] == large_cap(dim)
    assert want["large"] == large and want["streamed"] == streamed
    if dim <= 2:  # every resident class
        assert cls["small"] >= 1 and cls["mid"] >= 1 and cls["large"] >= 1
    assert_schedule(sched, cls, streamed, None)
    assert np.array_equal(got, _want(oracle, ("b1", dim, tuple(sizes)), case))


def test_size_classes_natural_rule(ctx, oracle, monkeypatch):
    """No knob: res_cap = sqrt(sum s^2 / CUs / 4), 314 on 256 CUs -- 300 and 257 resident,
    320, 1000 and 10 000 streamed.  The expectation follows the device's CU count."""
    _setenv(monkeypatch, None)
    sizes = [10000, 1000, 320, 300, 257]
    case = _b1_case(3, sizes)
    got, cls, sched = run_plan(ctx, case)
    want = assert_census(cls, sizes, 3, None)
    assert want["streamed"] and cls["streamed"] == len(want["streamed"])
    assert_schedule(sched, cls, want["streamed"], None)
    assert np.array_equal(got, _want(oracle, ("b1-natural",), case))


# --------------------------------------------------------------------------
# B2: options on every class

OPTION_SETS = {
    "params": C.ML_OPTIONS,
    "unweighted": dict(use_weights=0),
    "nohubs": dict(nohubs=1),
    "nohubs-unweighted-repel2^70": dict(nohubs=1, use_weights=0, repel=2.0 ** 70),
}
B2 = [(3, k) for k in OPTION_SETS] + [(1, "params"), (4, "params")]


@pytest.mark.parametrize("layout,mode", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("dim,opts", B2, ids=[f"d{d}-{k}" for d, k in B2])
def test_options(ctx, oracle, monkeypatch, layout, mode, dim, opts):
    """ks, ksmax, tolerate, attract, gravity, repel; use_weights on fractional weights
    (the internal degree and every attraction term); the nohubs division by deg + 1; all
    of them outside the shared-reciprocal domain (repel = 2^70)."""
    case = C.ml_layout(layout, dim=dim, **OPTION_SETS[opts])
    got = _run_layout(ctx, monkeypatch, layout, mode, case)
    want = _want(oracle, ("b2", layout, dim, opts), case)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want)


def _heavy_row_case(weighted, **kw):
    """The graph of test_gpu_parity.py test_faml_early_heavy_row_chains."""
    sizes = [12000, 3000, 2000, 300]
    n = sum(sizes)
    A = G.with_hubs(G.rmat(n, 8 * n, seed=23), [(5, 12000), (600, 9000), (40, 5000)], seed=3)
    deg = np.diff(A[0])
    assert (deg >= 8192).sum() >= 2 and ((deg > 512) & (deg < 8192)).any()
    if weighted:
        A = C.symmetric_weights(A)
    return C._ml(A, sizes, 9, 3, 3, 29, **kw), sizes


@pytest.mark.parametrize("use_weights", [1, 0])
def test_heavy_row_terms_with_weights(ctx, oracle, monkeypatch, use_weights):
    """FamlRows tiles, stored-term segments and chain waves on fractional weights, used
    and ignored: early rows (>= 8 192 entries, side stream) and a late heavy row."""
    monkeypatch.setenv("GE_ROWS_TILES", "1")
    _setenv(monkeypatch, None)
    case, sizes = _heavy_row_case(True, use_weights=use_weights)
    got, cls, sched = run_plan(ctx, case)
    want = assert_census(cls, sizes, 3, None)
    assert 12000 in want["streamed"]
    assert cls["seg_mode"] == 2 and cls["ntiles"] > 0, cls
    assert cls["nearly"] >= 2 and cls["nheavy"] - cls["nearly"] >= 1, cls
    assert cls["nseg_early"] >= 2 * 16 and cls["nseg"] > cls["nseg_early"], cls
    assert np.array_equal(got, _want(oracle, ("b2-heavy", use_weights), case))


LOG_POW_SETS = {"linlog": dict(linlog=1), "delta2": dict(delta=2.0),
                "delta0.5-linlog": dict(delta=0.5, linlog=1)}


@pytest.mark.parametrize("layout,mode", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("opts", list(LOG_POW_SETS))
def test_linlog_delta(ctx, oracle, monkeypatch, layout, mode, opts):
    """Device log / pow (ocml) against glibc in the multilevel attraction: the project's
    bar for them, 1e-12 after one iteration (test_gpu_configs.py
    test_linlog_delta_tolerance), per aggregate as max|got - want| <= 1e-12 max|want|
    (the final centring subtracts the aggregate's mean, so an element-wise relative
    error is unbounded near zero by construction).
    Largest measured on an MI355X over the 15 cases: 0 -- every case came out
    bit-identical to the oracle (the last-place differences of log / pow did not
    survive the sums they enter); each case prints its figure before it asserts."""
    case = C.ml_layout(layout, iterations=1, **LOG_POW_SETS[opts])
    got = _run_layout(ctx, monkeypatch, layout, mode, case)
    want = _want(oracle, ("b2-logpow", layout, opts), case)
    assert np.isfinite(want).all()
    PT = case["PT"]
    worst = 0.0
    for a in range(len(PT[0]) - 1):
        v = PT[1][PT[0][a]:PT[0][a + 1]]
        scale = np.abs(want[v]).max()
        assert scale > 0.0
        worst = max(worst, np.abs(got[v] - want[v]).max() / scale)
    print(f"linlog/delta {layout} {mode} {opts}: max|got-want| / max|want| = {worst:.3e}")
    assert worst <= 1e-12


# --------------------------------------------------------------------------
# B3: domain edges

def _largest_tiles(case):
    sizes = np.diff(case["PT"][0])
    a = int(np.argmax(sizes))
    return a, int(sizes[a]), (int(sizes[a]) - 1) // 64


@pytest.mark.parametrize("layout,mode", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("edge", ["one-edge-2^61", "all-2^61", "all-2^-70"])
def test_weight_domain_edges(ctx, oracle, monkeypatch, layout, mode, edge):
    """Weights that take deg + 1 out of weight_ok (ge_math.hpp): one internal edge per
    aggregate (two members fall back, their tiles mix with fast ones), every weight
    (every tile falls back), and weights far below 1."""
    base = C.ml_layout(layout)
    if edge == "one-edge-2^61":
        case = C.with_heavy_edges(base)
        a, s, last = _largest_tiles(case)
        out = np.flatnonzero(~(C.internal_degree_plus_one(case, a) <= 2.0 ** 60))
        assert len(out) == 2
        if s > 64:  # different 64-row tiles, one of them the last
            assert out[0] // 64 != out[1] // 64 and out[1] // 64 == last
        if layout == "streamed":
            assert s % 64 != 0  # ragged
    else:
        case = C.with_scaled_weights(base, 2.0 ** 61 if edge == "all-2^61" else 2.0 ** -70)
    got = _run_layout(ctx, monkeypatch, layout, mode, case)
    want = _want(oracle, ("b3-w", layout, edge), case)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("layout,mode", CONFIGS, ids=CONFIG_IDS)
def test_coarse_coordinate_edges(ctx, oracle, monkeypatch, layout, mode):
    """coords_A with a 1e-70 component (ca_ok false for its members, `/` for the pulls
    towards it), an aggregate at the exact origin, two joined aggregates at identical
    coordinates (the dis clamp of pull_edge) and r_A = 0."""
    base = C.ml_layout(layout)
    spec = C.COARSE_EDGES[layout]
    assert C.edges_between(base, *spec["same"]) >= 1
    case = C.with_coarse_edges(base, layout)
    assert np.array_equal(case["cA"][spec["same"][0]], case["cA"][spec["same"][1]])
    assert (case["cA"][list(spec["tiny"])] == C.TINY).sum() == len(spec["tiny"])
    assert not case["cA"][spec["origin"]].any() and case["rA"][spec["zero_r"]] == 0.0
    got = _run_layout(ctx, monkeypatch, layout, mode, case)
    want = _want(oracle, ("b3-c", layout), case)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want)


# aggregates of each layout whose start is overwritten: one per size class
START_AGGS = {"packed": (8, 7, 12, 11), "large": (0, 2), "streamed": (0, 3, 6)}


def _edge_start(oracle, case, layout, where):
    """The seeded start with, in one aggregate of every class: one coordinate of a member
    at 1e-70 (its tile leaves the domain; `where` places it in the first, a middle or the
    last row tile), two members coincident (s == 0 off the diagonal) and one member at
    the exact origin (the mag clamp, neg_over)."""
    dim = case["dim"]
    PT = case["PT"]
    n = len(case["vA"])
    init = oracle.uniform_stream(case["seed"], n * dim).reshape(n, dim).copy()
    placed = {}
    for a in START_AGGS[layout]:
        base, s = int(PT[0][a]), int(PT[0][a + 1] - PT[0][a])
        assert s >= 30
        tiles = (s + 63) // 64
        tiny = {"first": 5, "middle": min((tiles // 2) * 64 + 7, s - 4), "last": s - 3}[where]
        twin_a, twin_b, origin = 1, s // 2 + 1, s - 1
        assert len({tiny, twin_a, twin_b, origin}) == 4
        init[base + tiny, 0] = C.TINY
        init[base + twin_b] = init[base + twin_a]
        init[base + origin] = 0.0
        placed[a] = (tiny, tiles)
    return init, placed


@pytest.mark.parametrize("layout,mode", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_start_domain_edges(ctx, oracle, monkeypatch, layout, mode, where):
    """A supplied start (d_init on the device, init= on the oracle, whose entry equals
    the seeded one bit for bit: test_oracle.py) outside the domain in single members, so
    that a sweep meets a fallback tile before and after fast ones."""
    case = C.ml_layout(layout)
    init, placed = _edge_start(oracle, case, layout, where)
    a, s, last = _largest_tiles(case)
    tiny, tiles = placed[a]
    if layout == "streamed":
        assert tiles == last + 1 >= 3 and s % 64 != 0
        assert tiny // 64 == {"first": 0, "middle": tiles // 2, "last": last}[where]
        assert 0 < tiles // 2 < last
    got = _run_layout(ctx, monkeypatch, layout, mode, case, init=init)
    want = _want(oracle, ("b3-s", layout, where), case, init=init)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want)
