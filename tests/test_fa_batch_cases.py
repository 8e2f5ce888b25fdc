"""The batched single-level forceAtlas without a device: fa_batch_schedule pinned to the
hand-written table of tests/fa_batch_cases.py, its knobs, every argument error that
ge_force_atlas_batch / ge_embed_via_force_atlas_ml decide before they touch a device, the
numpy restatement of anyToMultilevel's extraction and placement, and the oracle's own
outputs on the inputs the GPU tests compare bit for bit."""
import numpy as np
import pytest

import fa_batch_cases as C
import ge_amd as ge
import graphs as G
import min_cases as M


def _sched(dim, **kw):
    sizes, entries = C.sizes_entries(C.cases())
    return ge.fa_batch_schedule(sizes, entries, dim, **kw)


@pytest.mark.parametrize("dim", [3, 8])
@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_schedule_table(dim, mode):
    s = _sched(dim, mode=ge.MODE_FAST if mode == "fast" else ge.MODE_STRICT)
    want = [C.TABLE[(dim, mode)][n] for n in C.SIZES]
    assert list(zip(s["cls"].tolist(), s["lanes"].tolist())) == want
    per = [sum(c == k for c, _ in want) for k in (C.WAVE, C.BLOCK, C.SERIAL)]
    assert [s["waves"], s["blocks"], s["serials"]] == per
    assert s["wave_workgroups"] == (per[0] + 3) // 4


def test_schedule_totals_strict_d3():
    s = _sched(3)
    assert (s["waves"], s["blocks"], s["serials"], s["wave_workgroups"]) == (15, 5, 1, 4)


def test_farfield_is_serial_below_the_wide_schedule():
    assert set(_sched(3, mode=ge.MODE_FARFIELD, theta=0.5)["cls"].tolist()) == {C.SERIAL}
    assert _sched(8, mode=ge.MODE_FARFIELD, theta=0.5)["cls"].tolist() == _sched(8)["cls"].tolist()


def test_knob_small_g(monkeypatch):
    monkeypatch.setenv("GE_SMALL_G", "2")
    s = _sched(3)
    # where 2 lanes per row fit the wave (n <= 32) or the 512-thread block (n <= 256)
    want = {n: 2 if n <= 32 or 64 < n <= 256 else 1 for n in C.SIZES if n <= 512}
    got = dict(zip(C.SIZES, s["lanes"].tolist()))
    assert {n: got[n] for n in want} == want and got[513] == 0
    monkeypatch.delenv("GE_SMALL_G")
    assert s["cls"].tolist() == _sched(3)["cls"].tolist()  # a knob moves no class


def test_knob_wide_min_dim(monkeypatch):
    monkeypatch.setenv("GE_WIDE_MIN_DIM", "3")
    for mode in (ge.MODE_STRICT, ge.MODE_FAST):  # the wide schedule runs FAST exactly
        s = _sched(3, mode=mode)
        want = [C.TABLE[(8, "strict")][n] for n in C.SIZES]
        assert list(zip(s["cls"].tolist(), s["lanes"].tolist())) == want
    s2 = _sched(2, mode=ge.MODE_FAST)  # below the bound: untouched
    assert set(s2["cls"].tolist()) == {C.SERIAL}


def test_schedule_empty_graph_and_empty_batch():
    s = ge.fa_batch_schedule([0, 5], [0, 8], 3)
    assert s["cls"].tolist() == [C.SERIAL, C.WAVE] and s["lanes"].tolist() == [0, 8]
    s = ge.fa_batch_schedule([], [], 3)
    assert (s["waves"], s["blocks"], s["serials"], s["wave_workgroups"]) == (0, 0, 0, 0)
    with pytest.raises(ge.GeError, match="1..16"):
        ge.fa_batch_schedule([3], [2], 17)


def _raw(off, ip, ix, dx, dim=3, iterations=1, n=None):
    off, ip, ix = (np.asarray(a, dtype=np.int32) for a in (off, ip, ix))
    X = np.zeros((int(off[-1]) if n is None else n, dim))
    return ge._force_atlas_batch_raw(None, off, ip, ix, np.asarray(dx, dtype=np.float64), dim, X,
                                     False, None, iterations, {})


def test_argument_errors_before_the_device():
    """Two paths of two vertices each: rows 0-1 and 2-3."""
    off, ip, ix, dx = [0, 2, 4], [0, 1, 2, 3, 4], [1, 0, 3, 2], [1.0] * 4
    with pytest.raises(ge.GeError, match="null context"):  # everything else is in order
        _raw(off, ip, ix, dx)
    with pytest.raises(ge.GeError, match=r"1001.*graph 1: .*outside"):
        _raw(off, ip, [1, 0, 1, 2], dx)  # graph 1's first entry points into graph 0
    with pytest.raises(ge.GeError, match=r"graph 0: .*outside"):
        _raw(off, ip, [2, 0, 3, 2], dx)
    with pytest.raises(ge.GeError, match=r"graph 0: .*outside"):
        _raw(off, ip, [-1, 0, 3, 2], dx)
    with pytest.raises(ge.GeError, match=r"graph 1: .*offsets"):
        _raw([0, 3, 2, 4], ip, ix, dx, n=4)  # descending
    with pytest.raises(ge.GeError, match=r"graph 0: .*offsets"):
        _raw([1, 2, 4], ip, ix, dx)  # does not start at 0
    with pytest.raises(ge.GeError, match=r"graph 1: indptr"):
        _raw(off, [0, 1, 2, 1, 4], ix, dx)
    for dim in (0, 17):
        with pytest.raises(ge.GeError, match="1..16"):
            _raw(off, ip, ix, dx, dim=dim)
    with pytest.raises(ge.GeError, match="negative iteration"):
        _raw(off, ip, ix, dx, iterations=-1)
    # the Python layer's own shape checks
    with pytest.raises(ValueError):
        ge.force_atlas_batch(C.cases()[:2], 3, coords=[np.zeros((1, 3))])
    with pytest.raises(ValueError):
        ge.force_atlas_batch(C.cases()[:2], 3, seeds=[1])


def test_multilevel_argument_errors_before_the_device():
    lv = C.ml_level()
    args = lambda **o: ge.embed_via_force_atlas_ml(  # noqa: E731
        o.get("A", lv["A"]), o.get("PT", lv["PT"]), o.get("vA", lv["vA"]), lv["cA"][3], lv["rA"],
        o.get("dim", 3), iterations=o.get("iterations", 1))
    with pytest.raises(ge.GeError, match="null context"):
        args()
    twice = lv["PT"][1].copy()
    twice[1] = twice[0]
    with pytest.raises(ge.GeError, match="every fine vertex once"):
        args(PT=(lv["PT"][0], twice))
    wrong = lv["vA"].copy()
    wrong[lv["PT"][1][0]] = lv["m"] - 1
    with pytest.raises(ge.GeError, match="vertex_A does not match"):
        args(vA=wrong)
    with pytest.raises(ge.GeError, match="negative iteration"):
        args(iterations=-1)
    with pytest.raises(ge.GeError):
        ge.embed_via_force_atlas_ml(lv["A"], lv["PT"], lv["vA"], lv["cA"][3], lv["rA"], 17)


def test_concat_graphs_is_block_diagonal():
    gs = C.cases()[:6]
    off, ip, ix, dx = ge.concat_graphs(gs)
    assert off.tolist() == np.cumsum([0] + [len(A[0]) - 1 for A in gs]).tolist()
    for g, A in enumerate(gs):
        e0, e1 = ip[off[g]], ip[off[g + 1]]
        assert np.array_equal(ip[off[g]:off[g + 1] + 1] - e0, A[0])
        assert np.array_equal(ix[e0:e1] - off[g], A[1]) and np.array_equal(dx[e0:e1], A[2])


def test_cases_cover_the_extras():
    gs = C.cases()
    assert [len(A[0]) - 1 for A in gs] == list(C.SIZES)
    iso = [A for A in gs if len(A[0]) > 3 and A[0][-1] == A[0][-2]]
    selfe = [A for A in gs if A[0][1] > 0 and 0 in A[1][:A[0][1]]]
    wts = [A for A in gs if len(A[2]) and not np.all(A[2] == 1.0)]
    assert iso and selfe and wts
    for ip, ix, dx in gs:  # symmetric patterns and weights
        n = len(ip) - 1
        D = np.zeros((n, n))
        D[np.repeat(np.arange(n), np.diff(ip)), ix] = dx
        assert np.array_equal(D, D.T)


def test_sub_matrix_and_place_restate_the_reference_checked_helpers():
    """tests/min_cases.py's sub_pattern / place are pinned to the reference binary's own
    anyToMultilevel (tests/golden/ref_min_*.npz); the restatement here adds the values."""
    lv = M.level("small")
    for a in range(lv["m"]):
        sip, six, sdx = C.sub_matrix(lv["A"], lv["PT"], lv["vA"], a)
        wip, wix = M.sub_pattern(lv, a)
        assert np.array_equal(sip, wip) and np.array_equal(six, wix) and np.all(sdx == 1.0)
        nc = np.random.RandomState(a).uniform(-1, 1, size=(len(sip) - 1, 3))
        assert C.same(C.place(lv["cA"][3][a], lv["rA"][a], nc), M.place(lv, a, 3, nc), nan_ok=True)


def test_sub_matrix_sums_duplicates_and_keeps_self_entries():
    # vertices 0..3; aggregate 0 = (2, 0), aggregate 1 = (3, 1); row 2 stores 0 twice and itself
    A = (np.array([0, 2, 3, 6, 7]), np.array([2, 1, 3, 0, 0, 2, 1]), np.full(7, 9.0))
    PT = (np.array([0, 2, 4]), np.array([2, 0, 3, 1]))
    vA = np.array([0, 1, 0, 1])
    sip, six, sdx = C.sub_matrix(A, PT, vA, 0)
    assert sip.tolist() == [0, 2, 3] and six.tolist() == [0, 1, 0] and sdx.tolist() == [1.0, 2.0, 1.0]
    sip, six, sdx = C.sub_matrix(A, PT, vA, 1)
    assert sip.tolist() == [0, 1, 2] and six.tolist() == [1, 0] and sdx.tolist() == [1.0, 1.0]


def test_place_divides_zero_by_zero_as_the_reference():
    """A layout that ends at the origin (what the reference's 0 / 0 gives): NaN."""
    out = C.place(np.array([0.25, -0.5]), 0.3, np.zeros((1, 2)))
    assert np.isnan(out).all()


def test_oracle_outputs_are_finite_where_the_gpu_tests_compare_bits(oracle):
    gs = C.cases()
    for dim in (1, 3, 8):
        for A, X0 in zip(gs, C.start(gs, dim)):
            assert np.isfinite(oracle.force_atlas(A, dim, coords=X0, iterations=C.ITERATIONS)).all()


def test_restatement_on_a_three_level_hierarchy(oracle):
    """Level 0 of a 3-level R-MAT hierarchy through the restatement over the oracle's
    forceAtlas: every vertex is placed once, inside its aggregate's ball (the result is
    x / max, so |x - c_a| <= r_a up to rounding) with the farthest member on the ball.  A
    single member's layout is one point away from the origin (gravity moves it from its
    random start, it does not reach 0 in 50 iterations), so it lands on the ball too."""
    A = G.largest_component(G.rmat(600, 3000, seed=31))
    hier = oracle.partition(A, 0.2)
    assert len(hier) >= 2  # three levels
    PT = hier[0]
    vA = oracle.vertex_of(PT)
    m, rs = PT[2], np.random.RandomState(3)
    cA, rA = rs.uniform(-1, 1, size=(m, 3)), rs.uniform(0.1, 0.5, m)
    X = C.ml_compose(A, PT, vA, cA, rA, 3,
                     lambda S, d: oracle.force_atlas(S, d, iterations=50, seed=9))
    assert (np.diff(PT[0]) == 1).any()
    for a in range(m):
        v = PT[1][PT[0][a]:PT[0][a + 1]]
        dist = np.sqrt(((X[v] - cA[a]) ** 2).sum(axis=1))
        assert np.isfinite(X[v]).all() and dist.max() <= rA[a] * (1 + 1e-12)
        assert dist.max() >= rA[a] * (1 - 1e-12)  # the farthest member sits on the ball
