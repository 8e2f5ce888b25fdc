"""GE_MODE_FARFIELD on the device (graph-embed_amd/csrc/ge_far.hip) against the numpy
restatement of tests/far_cases.py; the bound and its derivation are in
tests/test_far_cases.py's docstring.  GE_FAR_MIN=0 lets the small inputs run the far
field; GE_FAR_R selects 64- or 256-row items.

Measured on an MI355X (each case prints its figure before it asserts): largest error /
bound against STRICT (test_bound_against_strict, n = 4 097, theta = 0.5, 256-row items)
0.387 / 0.270 / 0.092 / 0.021 at d = 1 / 2 / 3 / 4; largest error / rounding term against
the replay of the device's own decomposition (test_kernel_equals_replay) 0.061 (d = 1),
0.013-0.028 at d = 2..4.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import far_cases as F
import ge_amd as ge

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "graph-embed_amd")
LD = np.longdouble


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GE_FAR_MIN", "0")
    for k in ("GE_FAR_R", "GE_WIDE_MIN_DIM", "GE_MODE", "GE_THETA"):
        monkeypatch.delenv(k, raising=False)


class Dev:
    """A graph and coordinates on the device, and plans over them."""

    def __init__(self, ctx, A, X):
        import torch
        self.torch, self.ctx = torch, ctx
        self.dev = torch.device("cuda:0")
        self.A = [torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in A]
        self.n, self.d = X.shape
        self.nnz = len(A[1])
        self.x = torch.from_numpy(np.ascontiguousarray(X)).to(self.dev)

    def plan(self, rb=0, re=None, **kw):
        re = self.n if re is None else re
        return self.ctx.fa_plan(self.n, self.nnz, *(t.data_ptr() for t in self.A), self.d, rb, re,
                                **kw)

    def repulse(self, plan, rows=None, x=None):
        f = self.torch.full((self.n if rows is None else rows, self.d), 7.0,
                            dtype=self.torch.float64, device=self.dev)
        plan.repulse((self.x if x is None else x).data_ptr(), f.data_ptr())
        return f.cpu().numpy()


def far_pass(ctx, n, d, X=None, rows=256, **kw):
    """(Dev, plan, Frep, info, layout) of one far-field pass."""
    A, Xs = F.case(n)
    dv = Dev(ctx, A, Xs[d] if X is None else X)
    os.environ["GE_FAR_R"] = "1" if rows == 64 else "4"
    try:
        plan = dv.plan(mode=ge.MODE_FARFIELD, **kw)
    finally:
        del os.environ["GE_FAR_R"]
    f = dv.repulse(plan)
    info = plan.far_info()
    assert info["active"] and info["reason"] == "active" and not info["fallback"]
    assert info["item_rows"] == rows
    return dv, plan, f, info, plan.far_layout()


@functools.lru_cache(maxsize=None)
def _masses(n):
    return F.masses(F.case(n)[0])


# -- 1. the layout ----------------------------------------------------------------------

@pytest.mark.parametrize("n,d,rows", [(4097, 1, 256), (4097, 2, 256), (4097, 3, 256),
                                      (4097, 4, 256), (16449, 3, 64), (16449, 2, 256)])
def test_layout_is_valid(ctx, n, d, rows):
    dv, plan, _, info, lay = far_pass(ctx, n, d, rows=rows)
    plan.close()
    X, m = F.case(n)[1][d], _masses(n)
    shape = F.level_shape(n)
    assert info["level_cells"] == [c for c, _ in shape]
    assert info["level_points"] == [p for _, p in shape]
    perm, keys = lay["perm"], lay["keys"]
    assert np.array_equal(np.sort(perm), np.arange(n))
    box = F.box_of(X)
    assert np.array_equal(lay["box"], box)
    assert np.array_equal(keys, F.keys_of(X, box)[perm])
    assert (keys[1:] >= keys[:-1]).all()
    tie = keys[1:] == keys[:-1]
    assert (perm[1:][tie] > perm[:-1][tie]).all()
    Xs, ms = X[perm], m[perm]
    for cells, pts in list(zip(lay["cells"], info["level_points"])) + [(lay["items"], rows)]:
        ref = F.summaries(Xs, ms, pts, dtype=LD)
        cnt = np.minimum(pts, n - np.arange(len(ref)) * pts)
        assert cells.shape == ref.shape
        # M: a sum of cnt positive terms; c: a quotient of two such sums
        assert (np.abs(cells[:, d] - ref[:, d]) <= (cnt + 2) * F.U * ref[:, d]).all()
        scale = np.array([(ms[q * pts:(q + 1) * pts, None].astype(LD)
                           * np.abs(Xs[q * pts:(q + 1) * pts]).astype(LD)).sum(axis=0)
                          for q in range(len(ref))]) / ref[:, d:d + 1]
        assert (np.abs(cells[:, :d] - ref[:, :d]) <= (2 * cnt[:, None] + 8) * F.U * scale).all()
        # a is an upper bound of max |x_j - c| about the DEVICE's centre
        for q in range(len(ref)):
            dx = Xs[q * pts:(q + 1) * pts].astype(LD) - cells[q, :d].astype(LD)
            astar = np.sqrt((dx * dx).sum(axis=1).max())
            assert cells[q, d + 1] >= astar
            assert cells[q, d + 1] <= astar * (1 + 2.0 ** -39) + 1e-300
    # every row lies inside its item's ball
    q = np.arange(n) // rows
    r = np.sqrt(((Xs.astype(LD) - lay["items"][q, :d].astype(LD)) ** 2).sum(axis=1))
    assert (r <= lay["items"][q, d + 1]).all()


# -- 2. the kernel computes the approximation it claims -----------------------------------

def check_items(f, lay, X, m, repel, items):
    worst = 0.0
    for q in items:
        pos, Fa, T, terms, _ = F.replay_item(lay, q, X, m, repel)
        got = f[lay["perm"][pos]]
        tol = 1.01 * (terms + F.K_TERM) * F.U * T
        bad = ~(np.abs(got - Fa) <= tol)
        assert not bad.any(), (q, np.argwhere(bad)[:4], got[bad][:4], Fa[bad][:4])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(tol > 0, np.abs(got - Fa) / tol, 0))))
    return worst


@pytest.mark.parametrize("repel", [1.0, 3.5])
@pytest.mark.parametrize("theta", [0.25, 0.5])
@pytest.mark.parametrize("d", F.DIMS)
def test_kernel_equals_replay(ctx, d, theta, repel):
    n = 4097
    dv, plan, f, info, lay = far_pass(ctx, n, d, theta=theta, repel=repel)
    plan.close()
    assert lay["theta"] == theta
    worst = check_items(f, lay, F.case(n)[1][d], _masses(n), repel, range(len(lay["items"])))
    print(f"d = {d} theta = {theta} repel = {repel}: largest error / rounding term {worst:.3f}")
    acc, leaves, terms = F.accepted_counts(lay, n)
    assert info["accepted"] == acc and info["exact_leaves"] == leaves
    assert info["pair_terms"] == terms


@pytest.mark.parametrize("d", F.DIMS)
def test_kernel_equals_replay_degenerate(ctx, d):
    n, X = 4097, F.degenerate(d)
    dv, plan, f, info, lay = far_pass(ctx, n, d, X=X)
    plan.close()
    assert lay["cells"][0][0, d + 1] == 0.0  # the clump's leaf
    assert np.isfinite(f).all()
    check_items(f, lay, X, _masses(n), 1.0, range(len(lay["items"])))
    assert sum(info["accepted"]) > 0


@pytest.mark.parametrize("d,rows", [(1, 64), (2, 64), (3, 64), (3, 256), (4, 64)])
def test_kernel_equals_replay_three_levels(ctx, d, rows):
    n = 16449
    dv, plan, f, info, lay = far_pass(ctx, n, d, rows=rows)
    plan.close()
    nit = len(lay["items"])
    items = sorted(set(range(0, nit, 7)) | {0, nit - 1, nit - 2, 16384 // rows - 1, 16384 // rows})
    check_items(f, lay, F.case(n)[1][d], _masses(n), 1.0, items)
    assert info["levels"] == 3 and info["accepted"][0] > 0 and info["accepted"][2] > 0
    if d < 4:
        assert min(info["accepted"]) > 0
    assert 0 < info["pair_terms"] < n * (n - 1)


# -- 3. the approximation meets the bound ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_abs(d):
    """sum_j |t_ijk| of the exact sum for every row of the n = 4 097 input (repel 1)."""
    n = 4097
    X, m = F.case(n)[1][d], _masses(n)
    return np.concatenate([F.exact_rows(X, m, 1.0, np.arange(a, min(n, a + 512)))[1]
                           for a in range(0, n, 512)])


@pytest.mark.parametrize("d", F.DIMS)
def test_bound_against_strict(ctx, d):
    n = 4097
    dv, plan, f, info, lay = far_pass(ctx, n, d, theta=0.5)
    plan.close()
    strict = dv.plan(mode=ge.MODE_STRICT)
    fs = dv.repulse(strict)
    strict.close()
    X, m = F.case(n)[1][d], _masses(n)
    mom = F.cell_moments(lay, X, m)
    strict_round = F.rounding(_exact_abs(d), n)
    worst = 0.0
    for q in range(len(lay["items"])):
        pos, _, T, terms, order = F.replay_item(lay, q, X, m, 1.0)
        ids = lay["perm"][pos]
        err = np.sqrt(((f[ids].astype(LD) - fs[ids].astype(LD)) ** 2).sum(axis=1))
        bound = (F.truncation_bound(lay, order, mom, X[ids], m[ids]) + F.rounding(T, terms)
                 + strict_round[ids])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (q, float((err / bound).max()))
    print(f"d = {d}: largest error / bound against STRICT {worst:.3f}")
    assert sum(info["accepted"]) > 0 and info["pair_terms"] < n * (n - 1)


# -- 4. edges --------------------------------------------------------------------------------

def _fast(dv, rb=0, re=None):
    p = dv.plan(rb, re, mode=ge.MODE_FAST)
    f = dv.repulse(p, rows=(dv.n if re is None else re) - rb)
    p.close()
    return f


def test_theta_zero_is_fast_within_rounding(ctx):
    n, d = 4097, 2
    X = F.degenerate(d)
    dv, plan, f, info, lay = far_pass(ctx, n, d, X=X, theta=0.0)
    plan.close()
    for l, cells in enumerate(lay["cells"]):  # only cells of radius 0 can be accepted
        assert info["accepted"][l] <= int((cells[:, d + 1] == 0.0).sum()) * len(lay["items"])
    assert info["accepted"][0] > 0  # the clump's leaf, from far items
    T = np.concatenate([F.exact_rows(X, _masses(n), 1.0, np.arange(a, min(n, a + 512)))[1]
                        for a in range(0, n, 512)])
    assert (np.abs(f - _fast(dv)) <= 2 * 1.01 * (n + F.K_TERM) * F.U * T).all()


@pytest.mark.parametrize("d", [3, 5])
def test_falls_back_to_fast_bits(ctx, monkeypatch, d):
    """GE_FAR_MIN above n, d = 5 (FAST means the STRICT kernels there), a row shard and
    a non-positive mass: the reason is reported and the bits are FAST's."""
    n = 4097
    A = F.case(n)[0]
    X = np.random.RandomState(5).uniform(-1, 1, (n, d))
    dv = Dev(ctx, A, X)
    if d == 5:
        p = dv.plan(mode=ge.MODE_FARFIELD)
        assert p.far_info()["reason"] == "dim" and not p.far_info()["active"]
        f = dv.repulse(p)
        p.close()
        s = dv.plan(mode=ge.MODE_STRICT)
        assert np.array_equal(f, dv.repulse(s))
        s.close()
        return
    want = _fast(dv)
    monkeypatch.setenv("GE_FAR_MIN", str(n + 1))
    p = dv.plan(mode=ge.MODE_FARFIELD)
    assert p.far_info()["reason"] == "small"
    assert np.array_equal(dv.repulse(p), want)
    with pytest.raises(ge.GeError):
        p.far_layout()
    p.close()
    monkeypatch.setenv("GE_FAR_MIN", "0")
    lo, hi = 1000, 3000
    p = dv.plan(lo, hi, mode=ge.MODE_FARFIELD)
    assert p.far_info()["reason"] == "row_shard"
    shard = dv.repulse(p, rows=hi - lo)
    assert np.array_equal(shard, _fast(dv, lo, hi)) and np.array_equal(shard, want[lo:hi])
    p.close()
    # one vertex with deg + 1 <= 0 (negative weights on its edges)
    ip, ix, dx = (a.copy() for a in A)
    v = 77
    for e in range(ip[v], ip[v + 1]):
        u = ix[e]
        dx[e] = -1.0
        back = ip[u] + int(np.searchsorted(ix[ip[u]:ip[u + 1]], v))
        dx[back] = -1.0
    dn = Dev(ctx, (ip, ix, dx), X)
    p = dn.plan(mode=ge.MODE_FARFIELD)
    assert p.far_info()["reason"] == "mass"
    got = dn.repulse(p)
    p.close()
    assert got.tobytes() == _fast(dn).tobytes()


@pytest.mark.parametrize("theta", [1.0, -0.1, float("nan"), float("inf")])
def test_bad_theta_is_an_argument_error(ctx, theta):
    dv = Dev(ctx, F.case(4097)[0], F.case(4097)[1][2])
    with pytest.raises(ge.GeError, match="1001.*theta"):
        dv.plan(mode=ge.MODE_FARFIELD, theta=theta)
    dv.plan(mode=ge.MODE_FAST, theta=theta).close()  # read in no other mode
    with pytest.raises(ge.GeError, match="1001.*theta"):
        ctx.force_atlas(F.case(4097)[0], 2, coords=F.case(4097)[1][2], iterations=1,
                        mode=ge.MODE_FARFIELD, theta=theta)


def test_nan_coordinate_runs_fast(ctx):
    n, d = 4097, 3
    X = F.case(n)[1][d].copy()
    X[1234, 1] = np.nan
    X[17, 0] = np.inf
    dv = Dev(ctx, F.case(n)[0], X)
    p = dv.plan(mode=ge.MODE_FARFIELD)
    got = dv.repulse(p)
    info = p.far_info()
    assert info["active"] and info["fallback"] and info["pair_terms"] == 0
    # the next pass on finite coordinates runs the far field again
    x2 = dv.torch.from_numpy(F.case(n)[1][d]).to(dv.dev)
    dv.repulse(p, x=x2)
    assert not p.far_info()["fallback"] and sum(p.far_info()["accepted"]) > 0
    p.close()
    want = _fast(dv)
    assert np.isnan(want).any() and got.tobytes() == want.tobytes()


def test_deterministic(ctx):
    n, d = 16449, 3
    dv, plan, f, _, _ = far_pass(ctx, n, d, rows=64)
    assert dv.repulse(plan).tobytes() == f.tobytes()
    plan.close()
    _, plan2, f2, _, _ = far_pass(ctx, n, d, rows=64)
    plan2.close()
    assert f2.tobytes() == f.tobytes()


# -- 5. whole iterations --------------------------------------------------------------------

@pytest.mark.parametrize("d", [2, 3])
def test_iterations_equal_hand_stepped_plan(ctx, d):
    n = 4097
    A, Xs = F.case(n)
    dv = Dev(ctx, A, Xs[d])
    plan = dv.plan(mode=ge.MODE_FARFIELD, theta=0.5)
    assert plan.far_info()["active"]
    t = dv.torch
    x, y = dv.x.clone(), t.empty_like(dv.x)
    f = t.empty_like(dv.x)
    for it in (1, 2):
        plan.repulse(x.data_ptr(), f.data_ptr())
        plan.attract(x.data_ptr(), f.data_ptr(), y.data_ptr())
        ctx.sync()
        x, y = y, x
        got = ctx.force_atlas(A, d, coords=Xs[d], iterations=it, mode=ge.MODE_FARFIELD, theta=0.5)
        assert np.array_equal(got, x.cpu().numpy()), it
    plan.close()
    fast = ctx.force_atlas(A, d, coords=Xs[d], iterations=2, mode=ge.MODE_FAST)
    assert not np.array_equal(got, fast)  # the far field ran (the drift is recorded, not gated)


def test_hundred_iterations_stay_finite(ctx):
    A, Xs = F.case(4097)
    got = ctx.force_atlas(A, 3, coords=Xs[3], iterations=130, mode=ge.MODE_FARFIELD)
    assert np.isfinite(got).all()
    # the multilevel entry points take the mode as FAST
    import graphs as G
    B = G.largest_component(G.rmat(2000, 14000, seed=1))
    hier = ctx.partition(B, 0.125)
    PT = hier[0]
    vA = ge.vertex_of(PT)
    cA = G.random_coords(PT[2], 3, seed=3)
    rA = np.full(PT[2], 0.25)
    a = ctx.force_atlas_ml(B, PT, vA, cA, rA, 3, iterations=5, seed=4, mode=ge.MODE_FARFIELD)
    b = ctx.force_atlas_ml(B, PT, vA, cA, rA, 3, iterations=5, seed=4, mode=ge.MODE_FAST)
    assert np.array_equal(a, b)


# -- 6. the drop-in -------------------------------------------------------------------------

def test_dropin_reproduces_the_binding(ctx, tmp_path):
    n, d, theta = 4097, 2, 0.25
    A, Xs = F.case(n)
    exe = str(tmp_path / "farfield_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "farfield_driver.cpp"), f"-L{PKG}/lib",
                           "-lge", f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    a, x0 = str(tmp_path / "a.bin"), str(tmp_path / "x0.bin")
    with open(a, "wb") as fh:
        np.array([n, len(A[1])], np.int32).tofile(fh)
        for arr in A:
            arr.tofile(fh)
    Xs[d].tofile(x0)
    want = ctx.force_atlas(A, d, coords=Xs[d], iterations=2, mode=ge.MODE_FARFIELD, theta=theta)
    other = ctx.force_atlas(A, d, coords=Xs[d], iterations=2, mode=ge.MODE_FARFIELD, theta=0.75)
    assert not np.array_equal(want, other)  # theta reaches the kernel
    env = dict(os.environ)
    for how, extra in (("set", {}), ("env", {"GE_MODE": "farfield", "GE_THETA": str(theta)})):
        out = str(tmp_path / f"out_{how}.bin")
        r = subprocess.run([exe, a, x0, out, str(d), "2", how, str(theta)], env={**env, **extra},
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(out).reshape(n, d), want), how
    r = subprocess.run([exe, a, x0, str(tmp_path / "o.bin"), str(d), "1", "env", "0"],
                       env={**env, "GE_MODE": "farfield", "GE_THETA": "2"}, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 5 and "theta" in r.stderr
