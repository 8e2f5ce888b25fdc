"""The exact k nearest neighbours and the neighbourhood precision on the CPU: the library's
host path (ctx=None; graph-embed_amd/csrc/ge_knn.cpp) against the independent references
of tests/knn_cases.py, bit for bit, and proof that the inputs are what they claim.  The
device path is pinned to both in tests/test_gpu_knn.py.
"""
import numpy as np
import pytest

import ge_amd as ge
import knn_cases as K


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GE_KNN_HOST", "GE_KNN_JSPLIT"):
        monkeypatch.delenv(k, raising=False)


def _same(got, want, k):
    idx, d2 = got
    assert idx.dtype == np.int32 and idx.shape == (len(want[0]), k)
    assert np.array_equal(idx, want[0][:, :k])
    assert d2.tobytes() == np.ascontiguousarray(want[1][:, :k]).tobytes()


HOST_INPUTS = [("exact", 300, 3), ("exact", 65, 1), ("exact", 66, 16), ("lattice", 125, 3),
               ("lattice", 100, 2), ("coincident", 70, 2), ("duplicated", 131, 4),
               ("closer", 200, 1), ("farther", 200, 2), ("nan", 90, 3), ("inf", 90, 1),
               ("overflow", 90, 5), ("doubles", 300, 3), ("doubles", 120, 1),
               ("doubles", 100, 2), ("doubles", 100, 4), ("doubles", 90, 5), ("doubles", 80, 8),
               ("doubles", 70, 16)]


@pytest.mark.parametrize("kind,n,d", HOST_INPUTS, ids=lambda v: str(v))
def test_host_path_equals_the_reference(kind, n, d):
    X, idx, d2 = K.case(kind, n, d)
    for k in (1, 2, 16, 63, 64):
        _same(ge.layout_knn(X, k, dist=True), (idx, d2), k)
    only = ge.layout_knn(X, 5)
    assert np.array_equal(only, idx[:, :5])


@pytest.mark.parametrize("n", [1, 2, 5, 6, 7])
def test_host_path_with_fewer_candidates_than_k(n):
    X, idx, d2 = K.case("exact", n, 3)
    got = ge.layout_knn(X, 5, dist=True)
    _same(got, (idx, d2), 5)
    cand = min(5, n - 1)
    assert (got[0][:, cand:] == -1).all() and np.isposinf(got[1][:, cand:]).all()
    assert (got[0][:, :cand] >= 0).all()


def test_rows_in_any_order_with_repeats_and_none():
    X, idx, d2 = K.case("lattice", 125, 3)
    rows = np.random.RandomState(5).randint(0, 125, size=300)
    assert len(set(rows.tolist())) < len(rows)
    got = ge.layout_knn(X, 7, rows=rows, dist=True)
    _same(got, (idx[rows], d2[rows]), 7)
    none = ge.layout_knn(X, 7, rows=np.zeros(0, np.int32), dist=True)
    assert none[0].shape == (0, 7) and none[1].shape == (0, 7)


# --------------------------------------------------------------------------
# the inputs are what they claim

def test_a_tie_straddles_the_kth_place():
    for kind, n, d, k in (("lattice", 125, 3, 4), ("lattice", 100, 2, 3),
                          ("duplicated", 131, 4, 1), ("coincident", 70, 2, 16)):
        X, idx, d2 = K.case(kind, n, d)
        straddle = d2[:, k - 1] == d2[:, k]  # the k-th and the (k + 1)-th are equally far
        assert straddle.any(), kind
        # and the order between them is the index's
        assert (idx[straddle, k - 1] < idx[straddle, k]).all(), kind
    X, idx, d2 = K.case("coincident", 70, 2)
    for i in (0, 1, 35, 69):  # the k lowest other indices
        assert idx[i].tolist() == [j for j in range(70) if j != i][:K.MAX_K]
    assert not d2.any()
    X, idx, d2 = K.case("duplicated", 131, 4)
    assert (d2[:65, 0] == 0).all() and np.array_equal(idx[:65, 0], np.arange(65) + 66)


def test_the_overflow_case_overflows_and_leaves_the_rest_alone():
    n, d = 90, 5
    X, idx, d2 = K.case("overflow", n, d)
    a, b = K.bad_vertices("overflow", n)
    assert np.isfinite(X).all()
    with np.errstate(over="ignore"):
        assert np.isposinf((X[a, 0] - X[b, 0]) ** 2) and np.isposinf((X[a, 0] - X[0, 0]) ** 2)
    assert K.dist2_fraction(tuple(X[a]), tuple(X[b])) == K.INF
    for kind in K.BAD_KINDS:
        X, idx, d2 = K.case(kind, n, {"nan": 3, "inf": 1, "overflow": 5}[kind])
        bad = K.bad_vertices(kind, n)
        assert (idx[bad] == -1).all() and np.isposinf(d2[bad]).all()  # no neighbours as rows
        assert not np.isin(idx, bad).any()                           # excluded as partners
        good = np.setdiff1d(np.arange(n), bad)
        Y = X[good]  # everyone else: what they get without the bad vertices
        widx, wd2 = K.reference(Y)
        m = len(good) - 1
        assert np.array_equal(good[widx[:, :m]], idx[good, :m])
        assert wd2[:, :m].tobytes() == np.ascontiguousarray(d2[good, :m]).tobytes()


def test_the_lines_insert_as_often_as_they_claim():
    n, k = 200, 16
    assert K.restate_insertions(K.closer_line(n), [0], k) == n - 1
    assert K.restate_insertions(K.farther_line(n), [0], k) == k
    assert K.restate_insertions(K.farther_line(n), [0], k, jsplit=3) == 3 * k
    assert K.restate_insertions(K.closer_line(n), [0], k, jsplit=3) == n - 1
    # every insert of the closer line is at the head: the nearest is the last partner
    X, idx, _ = K.case("closer", 200, 1)
    assert idx[0, :k].tolist() == list(range(n - 1, n - 1 - k, -1))
    X, idx, _ = K.case("farther", 200, 2)
    assert idx[0, :k].tolist() == list(range(1, k + 1))


def test_the_reference_chain_rounds_once_per_fma():
    # fma and multiply + add differ on these: the Fraction chain follows the fma
    xi, xj = (0.1, 0.7, 0.3), (0.9, 0.2, 0.6)
    X = np.array([xi, xj])
    got = ge.layout_knn(X, 1, dist=True)[1]
    assert got[0, 0] == got[1, 0] == K.dist2_fraction(xi, xj)
    rs = np.random.RandomState(11)
    P = rs.uniform(-1, 1, size=(200, 3))
    differ = 0
    for a, b in zip(P[:100], P[100:]):
        e = a - b
        differ += ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) != K.dist2_fraction(tuple(a), tuple(b))
    assert differ > 0


def test_rows_per_workgroup_switch_points():
    # k = 64 cannot have 256 rows in 160 KiB at all, and not 128 in half of it
    assert 256 * 64 * K.ENTRY_BYTES > 160 * 1024
    for d in (1, 2, 3, 4, 5, 8, 16):
        a, b = K.switch_ks(d)
        assert 1 <= a < b < 64
        assert [K.rows_per_wg(k, d) for k in (a, a + 1, b, b + 1, 64)] == [256, 128, 128, 64, 64]
    assert K.switch_ks(3) == [24, 49] and K.switch_ks(8) == [16, 32]
    assert K.TILE_J * 16 * 8 + 64 * 64 * K.ENTRY_BYTES == K.LDS_BUDGET  # filled exactly


# --------------------------------------------------------------------------
# neighbourhood precision

def test_ring_on_a_circle_has_precision_one():
    n = 257
    A, X = K.ring(n), K.circle(n)
    per, tot = ge.layout_neighbourhood(A, X)
    assert (per == [2, 2]).all() and tot.tolist() == [n, 2 * n, 2 * n]
    assert ge.neighbourhood_precision(per) == (1.0, 1.0)
    nb, _ = K.reference_fraction(X, 16)
    wper, wtot = K.neighbourhood_reference(A, nb, 16)
    assert np.array_equal(per, wper) and np.array_equal(tot, wtot)
    # the same ring with the coordinates permuted: the layout no longer knows the graph
    perm = np.random.RandomState(6).permutation(n)
    per, tot = ge.layout_neighbourhood(A, X[perm])
    nb, d2 = K.reference_fraction(X[perm], 16)
    assert (d2[:, 1] < d2[:, 2]).all()  # k_i = 2 reads the first two, and they are clear
    wper, wtot = K.neighbourhood_reference(A, nb, 16)
    assert np.array_equal(per, wper) and np.array_equal(tot, wtot)
    mean, pooled = ge.neighbourhood_precision(per)
    assert mean == pooled == tot[ge.NBHD_HITS] / tot[ge.NBHD_K] and pooled < 0.1


def test_mixed_graph_integers():
    n = 60
    A, X = K.mixed_graph(n), K.case("exact", n, 3)[0]
    nb = K.case("exact", n, 3)[1]
    kmax = K.HUB_KMAX
    per, tot = ge.layout_neighbourhood(A, X, kmax=kmax)
    wper, wtot = K.neighbourhood_reference(A, nb, kmax)
    assert np.array_equal(per, wper) and np.array_equal(tot, wtot)
    assert np.diff(A[0])[0] > kmax and per[0, 0] == kmax      # the hub exceeds kmax
    assert per[1, 0] == 3                                     # {2, 5, 7}: self and repeats dropped
    assert per[2].tolist() == [0, 0] and per[3].tolist() == [0, 0]  # isolated; only a self entry
    assert tot[ge.NBHD_ROWS] == n - 2
    mean, pooled = ge.neighbourhood_precision(per)
    live = per[:, 0] > 0
    assert mean == (per[live, 1] / per[live, 0]).mean() and pooled == per[:, 1].sum() / per[:, 0].sum()
    rows = np.array([2, 0, 0, 59, 1], np.int32)  # a sample, with a repeat
    per_s, tot_s = ge.layout_neighbourhood(A, X, kmax=kmax, rows=rows)
    assert np.array_equal(per_s, per[rows])
    assert tot_s.tolist() == [4, int(per[rows, 0].sum()), int(per[rows, 1].sum())]
    assert np.isnan(ge.neighbourhood_precision(per[2:4])).all()


def test_descending_row_names_the_row():
    n = 60
    ip, ix, dx = K.mixed_graph(n)
    ix = ix.copy()
    e = ip[7]
    ix[e], ix[e + 1] = ix[e + 1], ix[e]
    with pytest.raises(ge.GeError, match="row 7 is not ascending"):
        ge.layout_neighbourhood((ip, ix, dx), K.case("exact", n, 3)[0])


# --------------------------------------------------------------------------
# arguments, symbols

def test_argument_errors_name_the_range():
    X = K.case("exact", 65, 1)[0]
    for dim in (0, 17):
        with pytest.raises(ge.GeError, match=r"1\.\.16"):
            ge.layout_knn(np.zeros((5, dim)), 1)
    for k in (0, 65, -1):
        with pytest.raises(ge.GeError, match=r"k must be 1\.\.64"):
            ge.layout_knn(X, k)
        with pytest.raises(ge.GeError, match=r"kmax must be 1\.\.64"):
            ge.layout_neighbourhood(K.ring(65), X, kmax=k)
    with pytest.raises(ge.GeError, match="n must be at least 1"):
        ge.layout_knn(np.zeros((0, 3)), 1)
    for bad in (-1, 65):
        with pytest.raises(ge.GeError, match=rf"row id {bad} at position 1 is outside 0\.\.64"):
            ge.layout_knn(X, 2, rows=[3, bad])
    L = ge.lib()
    idx = np.zeros(65 * 2, np.int32)
    assert L.ge_layout_knn(None, 65, 1, X.reshape(-1), 2, 64, None, idx.ctypes.data, None) == 1001
    assert b"n_rows must be n" in L.ge_last_error()
    assert L.ge_layout_knn(None, 65, 1, X.reshape(-1), 2, 65, None, None, None) == 1001
    assert b"null idx" in L.ge_last_error()
    assert L.ge_layout_knn_device(None, 65, 1, None, 2, 65, None, None, None) == 1001
    assert b"needs a context" in L.ge_last_error()
    assert L.ge_knn_info(None, None, None, None, None, None) == 1001


def test_header_declares_the_knn_calls():
    syms = ge.header_symbols()
    for name in ("ge_layout_knn", "ge_layout_knn_device", "ge_layout_neighbourhood", "ge_knn_info"):
        assert name in syms and name in ge._SIGS and hasattr(ge.lib(), name)
    txt = open(ge.HEADER).read()
    for macro, val in (("GE_KNN_MAX_K", ge.KNN_MAX_K), ("GE_NBHD_ROWS", ge.NBHD_ROWS),
                       ("GE_NBHD_K", ge.NBHD_K), ("GE_NBHD_HITS", ge.NBHD_HITS),
                       ("GE_NBHD_TOTALS", ge.NBHD_TOTALS)):
        assert f"#define {macro} {val}\n" in txt
    assert ge.KNN_MAX_K == K.MAX_K
    for name in ("host", "device"):
        assert f"#define GE_KNN_PATH_{name.upper()} {ge.KNN_PATHS.index(name)}" in txt
    for name in ("narrow", "wide"):
        assert f"#define GE_KNN_FORM_{name.upper()} {ge.KNN_FORMS.index(name)}" in txt
