"""The exact k nearest neighbours and the neighbourhood precision on the device
(ge_layout_knn_device, ge_layout_knn, ge_layout_neighbourhood, partition::layoutNeighbours;
graph-embed_amd/csrc/ge_knn.hip) against the library's host path and the independent
references of tests/knn_cases.py: idx equal, dist2 bit-equal.  tests/test_knn_cases.py pins
the host path to the references on the CPU and proves the inputs.

Every device call here reads its coordinates from a buffer that ends in rows of NaN (a
partner read past row n - 1 would be no candidate and go unnoticed, but a query row read
there loses all its neighbours) and writes into outputs followed by sentinel guard rows.
"""
import os
import subprocess

import numpy as np
import pytest

import ge_amd as ge
import knn_cases as K
from test_dropin import HERE, PKG, REPO, write_csr

pytestmark = pytest.mark.gpu

SENT_I, SENT_D = -7, 7.0
GUARD = 3      # rows past the last query row in both outputs: they keep the sentinels
NAN_ROWS = 16  # rows of NaN behind the coordinates


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GE_KNN_HOST", "GE_KNN_JSPLIT"):
        monkeypatch.delenv(k, raising=False)


def _buffers(X, k, rows):
    import torch
    dev = torch.device("cuda:0")
    n, d = X.shape
    x = torch.full((n + NAN_ROWS, d), float("nan"), dtype=torch.float64, device=dev)
    x[:n] = torch.from_numpy(np.array(X, np.float64)).to(dev)
    n_rows = n if rows is None else len(rows)
    r = None
    if rows is not None:  # an empty list still needs a pointer
        r = torch.zeros(max(n_rows, 1), dtype=torch.int32, device=dev)
        r[:n_rows] = torch.from_numpy(np.array(rows, np.int32)).to(dev)
    idx = torch.full((n_rows + GUARD, k), SENT_I, dtype=torch.int32, device=dev)
    d2 = torch.full((n_rows + GUARD, k), SENT_D, dtype=torch.float64, device=dev)
    return x, r, idx, d2, n_rows


def _take(idx, d2, n_rows, dist):
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert (idx[n_rows:] == SENT_I).all() and (d2[n_rows:] == SENT_D).all()
    if not dist:
        assert (d2 == SENT_D).all()
    return idx[:n_rows], d2[:n_rows]


def dev_knn(ctx, X, k, rows=None, dist=True):
    """(idx, dist2, info) of ge_layout_knn_device on guarded buffers."""
    import torch
    x, r, idx, d2, n_rows = _buffers(X, k, rows)
    torch.cuda.synchronize()
    ctx.layout_knn_device(X.shape[0], X.shape[1], x.data_ptr(), k, n_rows,
                          None if r is None else r.data_ptr(), idx.data_ptr(),
                          d2.data_ptr() if dist else None)
    ctx.sync()
    info = ctx.knn_info()
    return _take(idx, d2, n_rows, dist) + (info,)


def _check(ctx, kind, n, d, k, rows=None, host=True):
    """The device against the reference of a named input (and the host path)."""
    X, widx, wd2 = K.case(kind, n, d)
    if rows is not None:
        widx, wd2 = widx[rows], wd2[rows]
    idx, d2, info = dev_knn(ctx, X, k, rows)
    assert np.array_equal(idx, widx[:, :k]), (kind, n, d, k)
    assert d2.tobytes() == np.ascontiguousarray(wd2[:, :k]).tobytes(), (kind, n, d, k)
    n_rows = n if rows is None else len(rows)
    assert info["path"] == "device" and info["form"] == ("narrow" if d <= 4 else "wide")
    assert info["rows_per_wg"] == K.rows_per_wg(k, d)
    if "GE_KNN_JSPLIT" not in os.environ:
        assert info["jsplit"] == K.auto_jsplit(n, n_rows, k, d)
    if host:
        hidx, hd2 = ge.layout_knn(X, k, rows=rows, dist=True)
        assert np.array_equal(idx, hidx) and d2.tobytes() == hd2.tobytes()
    return idx, d2, info


# --------------------------------------------------------------------------
# sizes

@pytest.mark.parametrize("k", [1, 2, 5, 64])
def test_fewer_vertices_than_neighbours_asked_for(ctx, k):
    for n in sorted({1, 2, k, k + 1, k + 2}):
        idx, d2, _ = _check(ctx, "exact", n, 3, k)
        cand = min(k, n - 1)
        assert (idx[:, cand:] == -1).all() and np.isposinf(d2[:, cand:]).all()
        assert (idx[:, :cand] >= 0).all()


# the tile and the 256-row block: 255 .. 257; the 128- and 64-row blocks with the k that
# select them; the auto split's steps (one per tile up to 16): 511 .. 513, 1 023 .. 1 025,
# 4 096 / 4 097
EDGE_SIZES = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4096,
              4097]


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_tile_row_block_and_split_edges(ctx, n):
    for d, k in ((3, 16), (3, 25), (3, 50)) + (((8, 16),) if n <= 1025 else ()):
        _check(ctx, "exact", n, d, k, host=n <= 1025)


@pytest.mark.parametrize("n", [1025, 4097])
@pytest.mark.parametrize("d", [3, 8])
def test_device_equals_host_path_on_random_doubles(ctx, n, d):
    X = K.random_doubles(n, d, seed=n + d)
    for k in (16, 64):
        idx, d2, _ = dev_knn(ctx, X, k)
        hidx, hd2 = ge.layout_knn(X, k, dist=True)
        assert np.array_equal(idx, hidx) and d2.tobytes() == hd2.tobytes()
        assert (idx >= 0).all() and np.isfinite(d2).all() and (np.diff(d2, axis=1) >= 0).all()


@pytest.mark.parametrize("d", [3, 8])
def test_every_k_at_which_the_shape_changes(ctx, d):
    a, b = K.switch_ks(d)
    seen = set()
    for k in sorted({1, 2, 63, 64, a - 1, a, a + 1, b - 1, b, b + 1}):
        _, _, info = _check(ctx, "exact", 513, d, k)
        seen.add(info["rows_per_wg"])
    assert seen == {256, 128, 64}


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8, 16])
def test_every_dimension(ctx, d):
    for n in (257, 1025):
        _check(ctx, "exact", n, d, 16)
    n = {1: 120, 2: 100, 3: 300, 4: 100, 5: 90, 8: 80, 16: 70}[d]
    for k in (3, 64):
        _check(ctx, "doubles", n, d, k)  # against the Fraction chain


# --------------------------------------------------------------------------
# ties and cuts

TIES = [("lattice", 1025, 3), ("lattice", 4097, 2), ("coincident", 1025, 2),
        ("duplicated", 1025, 4), ("lattice", 513, 8)]


@pytest.mark.parametrize("kind,n,d", TIES, ids=lambda v: str(v))
def test_ties_and_every_j_split_give_the_same_bits(ctx, monkeypatch, kind, n, d):
    X, widx, wd2 = K.case(kind, n, d)
    for k in (4, 16):
        assert (wd2[:, k - 1] == wd2[:, k]).any()  # a tie straddles the k-th place
    first = None
    for split in (None, 1, 2, 3, K.MAX_SPLIT):
        if split is None:
            monkeypatch.delenv("GE_KNN_JSPLIT", raising=False)
        else:
            monkeypatch.setenv("GE_KNN_JSPLIT", str(split))
        for k in (4, 16):
            idx, d2, info = _check(ctx, kind, n, d, k, host=split is None and n <= 1025)
            assert split is None or info["jsplit"] == split
        first = first or (idx, d2)
        assert np.array_equal(idx, first[0]) and d2.tobytes() == first[1].tobytes()
    if kind == "coincident":
        assert idx[0].tolist() == list(range(1, 17)) and idx[9].tolist() == [
            j for j in range(18) if j != 9][:16]


def test_rows_in_shuffled_order_with_repeats_and_no_rows(ctx, monkeypatch):
    n, d, k = 1025, 3, 16
    rs = np.random.RandomState(8)
    rows = np.concatenate([rs.permutation(n)[:300], rs.randint(0, n, size=90)]).astype(np.int32)
    assert len(set(rows.tolist())) < len(rows)
    for split in (None, 3):
        if split:
            monkeypatch.setenv("GE_KNN_JSPLIT", str(split))
        _check(ctx, "lattice", n, d, k, rows=rows)
        _check(ctx, "lattice", n, d, k, rows=rows[:1])
    X = K.case("lattice", n, d)[0]
    idx, d2, info = dev_knn(ctx, X, k, rows=np.zeros(0, np.int32))
    assert idx.shape == (0, k) and info["insertions"] == 0
    hidx = ctx.layout_knn(X, k, rows=np.zeros(0, np.int32))
    assert hidx.shape == (0, k)
    # an id the device form cannot check reads nothing and gets no neighbours
    idx, d2, _ = dev_knn(ctx, X, k, rows=np.array([5, n, -1, 7], np.int32))
    want = K.case("lattice", n, d)[1]
    assert np.array_equal(idx[[0, 3]], want[[5, 7], :k])
    assert (idx[1:3] == -1).all() and np.isposinf(d2[1:3]).all()


# --------------------------------------------------------------------------
# order: the insertion count

@pytest.mark.parametrize("split", [1, 3])
def test_monotone_lines_insert_as_counted(ctx, monkeypatch, split):
    n, k = 4097, 16
    monkeypatch.setenv("GE_KNN_JSPLIT", str(split))
    _, _, info = _check(ctx, "closer", n, 1, k, rows=np.array([0], np.int32), host=False)
    assert info["insertions"] == n - 1  # every partner, at the head every time
    _, _, info = _check(ctx, "farther", n, 1, k, rows=np.array([0], np.int32), host=False)
    assert info["insertions"] == split * k
    monkeypatch.delenv("GE_KNN_JSPLIT")
    # all rows of a short line, the call's own split
    n = 513
    for kind in ("closer", "farther"):
        X = K.case(kind, n, 2)[0]
        _, _, info = _check(ctx, kind, n, 2, 5)
        assert info["insertions"] == K.restate_insertions(X, range(n), 5, info["jsplit"])
    # the host path counts its one chain
    monkeypatch.setenv("GE_KNN_HOST", "1")
    idx = ctx.layout_knn(X, 5)
    info = ctx.knn_info()
    assert info["path"] == "host" and info["insertions"] == K.restate_insertions(X, range(n), 5)
    assert np.array_equal(idx, K.case("farther", n, 2)[1][:, :5])


# --------------------------------------------------------------------------
# domain

@pytest.mark.parametrize("kind,d", [("nan", 3), ("inf", 1), ("overflow", 5), ("overflow", 2)])
def test_vertices_outside_the_domain(ctx, kind, d):
    n = 1025
    idx, d2, _ = _check(ctx, kind, n, d, 16)
    bad = K.bad_vertices(kind, n)
    assert (idx[bad] == -1).all() and np.isposinf(d2[bad]).all()
    assert not np.isin(idx, bad).any()
    good = np.setdiff1d(np.arange(n), bad)
    assert (idx[good] >= 0).all() and np.isfinite(d2[good]).all()
    widx, wd2 = K.reference(K.case(kind, n, d)[0][good], 16)  # everyone else is unaffected
    assert np.array_equal(good[widx], idx[good]) and wd2.tobytes() == d2[good].tobytes()


# --------------------------------------------------------------------------
# the host-pointer form, and the device form's stream

def test_host_pointer_form(ctx):
    X, widx, wd2 = K.case("lattice", 1025, 3)
    idx, d2 = ctx.layout_knn(X, 16, dist=True)
    assert np.array_equal(idx, widx[:, :16]) and d2.tobytes() == np.ascontiguousarray(wd2[:, :16]).tobytes()
    assert ctx.knn_info()["path"] == "device"
    assert np.array_equal(ctx.layout_knn(X, 3, rows=[7, 7, 0]), widx[[7, 7, 0], :3])
    for dim in (0, 17):
        with pytest.raises(ge.GeError, match=r"1\.\.16"):
            ctx.layout_knn(np.zeros((5, dim)), 1)
    with pytest.raises(ge.GeError, match=r"k must be 1\.\.64"):
        ctx.layout_knn(X, 65)
    with pytest.raises(ge.GeError, match="row id 1025 at position 0"):
        ctx.layout_knn(X, 2, rows=[1025])


def test_device_call_enqueues_without_synchronising():
    import torch
    n, d, k = 1025, 3, 16
    X, widx, wd2 = K.case("lattice", n, d)
    c = ge.Context(0)
    try:
        assert c.knn_info() == {"path": "none", "form": "narrow", "rows_per_wg": 0, "jsplit": 0,
                                "insertions": 0}
        st = torch.cuda.Stream()
        c.set_stream(st.cuda_stream)
        x, r, idx, d2, n_rows = _buffers(X, k, None)
        a = torch.rand(4096, 4096, dtype=torch.float64, device=x.device)
        args = (n, d, x.data_ptr(), k, n_rows, None, idx.data_ptr(), d2.data_ptr())
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            b = a @ a
            c.layout_knn_device(*args)  # the first call makes the scratch
        torch.cuda.synchronize()
        idx.fill_(SENT_I)
        d2.fill_(SENT_D)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for _ in range(8):  # some milliseconds of work ahead of the call on its stream
                b = a @ a
            c.layout_knn_device(*args)
            pending = not st.query()
        c.sync()
        assert st.query()
        assert pending, "the call returned only after its stream had drained"
        gi, gd = _take(idx, d2, n_rows, True)
        assert np.array_equal(gi, widx[:, :k]) and gd.tobytes() == np.ascontiguousarray(wd2[:, :k]).tobytes()
        assert c.knn_info()["insertions"] > 0 and b.shape == a.shape
    finally:
        c.close()


# --------------------------------------------------------------------------
# neighbourhood precision

def test_neighbourhood_of_a_ring_on_a_circle(ctx):
    n = 257
    A, X = K.ring(n), K.circle(n)
    per, tot = ctx.layout_neighbourhood(A, X)
    hper, htot = ge.layout_neighbourhood(A, X)
    assert np.array_equal(per, hper) and np.array_equal(tot, htot)
    assert (per == [2, 2]).all() and tot.tolist() == [n, 2 * n, 2 * n]
    assert ge.neighbourhood_precision(per) == (1.0, 1.0)
    perm = np.random.RandomState(6).permutation(n)
    per, tot = ctx.layout_neighbourhood(A, X[perm])
    wper, wtot = K.neighbourhood_reference(A, K.reference_fraction(X[perm], 16)[0], 16)
    assert np.array_equal(per, wper) and np.array_equal(tot, wtot)
    assert ge.neighbourhood_precision(per)[1] < 0.1


def test_neighbourhood_of_the_mixed_graph(ctx):
    n, kmax = 60, K.HUB_KMAX
    A = K.mixed_graph(n)
    X, nb, _ = K.case("exact", n, 3)
    per, tot = ctx.layout_neighbourhood(A, X, kmax=kmax)
    wper, wtot = K.neighbourhood_reference(A, nb, kmax)
    assert np.array_equal(per, wper) and np.array_equal(tot, wtot)
    assert per[0, 0] == kmax and per[1, 0] == 3 and not per[2:4].any()
    rows = np.array([2, 0, 0, 59, 1], np.int32)
    per_s, tot_s = ctx.layout_neighbourhood(A, X, kmax=kmax, rows=rows)
    assert np.array_equal(per_s, per[rows])
    assert tot_s.tolist() == [4, int(per[rows, 0].sum()), int(per[rows, 1].sum())]
    ip, ix, dx = A
    ix = ix.copy()
    e = ip[7]
    ix[e], ix[e + 1] = ix[e + 1], ix[e]
    with pytest.raises(ge.GeError, match="row 7 is not ascending"):
        ctx.layout_neighbourhood((ip, ix, dx), X)


# --------------------------------------------------------------------------
# the drop-in header

def test_dropin_layout_neighbours(ctx, tmp_path):
    exe = str(tmp_path / "knn_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "knn_driver.cpp"), f"-L{PKG}/lib", "-lge",
                           f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    n, d, k, kmax = 60, 3, 5, K.HUB_KMAX
    A = K.mixed_graph(n)
    X, widx, _ = K.case("exact", n, d)
    paths = [str(tmp_path / f) for f in ("a.bin", "x.bin", "idx.bin", "tot.bin")]
    write_csr(paths[0], A)
    np.ascontiguousarray(X).tofile(paths[1])
    r = subprocess.run([exe, paths[0], paths[1], str(d), str(k), str(kmax), paths[2], paths[3]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(paths[2], dtype=np.int32).reshape(n, k), widx[:, :k])
    got = np.fromfile(paths[3], dtype=np.int64)
    assert np.array_equal(got, ctx.layout_neighbourhood(A, X, kmax=kmax)[1])
    assert np.array_equal(got, K.neighbourhood_reference(A, widx, kmax)[1])
