"""GE_MODE_FARFIELD on the streamed aggregates of a multilevel level (the segmented
engine of graph-embed_amd/csrc/ge_far.hip behind ge_faml_plan_*), on the level of
tests/faml_far_cases.py under GE_FAML_RES_CAP=256 and, unless a test says otherwise,
GE_FAR_MIN_ML=257, so every streamed aggregate takes the far field.  The bound and its
derivation are in tests/test_far_cases.py's docstring; the restatement is tests/far_cases.py
applied per aggregate (tests/faml_far_cases.py).

Measured on an MI355X (each case prints its figure before it asserts): largest error /
bound against the exact clamped sum (test_bound_against_exact_sum, theta = 0.5, 64-row items)
0.469 / 0.148 / 0.077 / 0.095 at d = 1 / 2 / 3 / 4 (degenerate variant 0.469 / 0.148 / 0.075 /
0.047); largest error / rounding term against the replay of the device's own layout
(test_kernel_equals_replay) 0.112 at d = 1, 0.048-0.064 at d = 2..4.
"""
import os
import socket
import subprocess

import numpy as np
import pytest

import far_cases as F
import faml_far_cases as C
import ge_amd as ge
import graphs as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "graph-embed_amd")
LD = np.longdouble
ROWS = 64  # the plan's default item
FAR_ALL = C.far_aggs(257)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GE_FAML_RES_CAP", C.RES_CAP)
    monkeypatch.setenv("GE_FAR_MIN_ML", "257")
    for k in ("GE_FAML_SYM", "GE_FAML_SYM_CHAIN", "GE_FAML_R", "GE_FAML_U", "GE_WIDE_MIN_DIM",
              "GE_MODE", "GE_THETA", "GE_FAR_R"):
        monkeypatch.delenv(k, raising=False)


class _Device:
    """The level's arrays on the device for one dimension (uploaded once)."""

    def __init__(self, dim, A=None, cA=None):
        import torch
        self.torch = torch
        lv = C.level()
        self.lv, self.dim, self.n = lv, dim, lv["n"]
        up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to("cuda:0")
        A, PT = lv["A"] if A is None else A, lv["PT"]
        cA = lv["cA"][dim] if cA is None else cA
        self.t = [up(A[0], np.int32), up(A[1], np.int32), up(A[2], np.float64),
                  up(PT[0], np.int32), up(PT[1], np.int32), up(lv["vA"], np.int32),
                  up(cA, np.float64), up(lv["rA"], np.float64)]
        self.p = [x.data_ptr() for x in self.t]
        torch.cuda.synchronize()

    def plan(self, ctx, iterations=1, **kw):
        p = self.p
        return ge.FamlPlan(ctx, self.n, p[0], p[1], p[2], self.lv["PT"][0], p[3], p[4], p[5],
                           self.dim, iterations=iterations, **kw)

    def run(self, ctx, plan, init):
        torch = self.torch
        d_init = torch.from_numpy(np.array(init, dtype=np.float64, order="C").reshape(-1)).to("cuda:0")
        X = torch.zeros((self.n, self.dim), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        plan.run(self.p[6], self.p[7], d_init.data_ptr(), X.data_ptr())
        ctx.sync()
        return X.cpu().numpy()

    def repulse(self, plan, X):
        """Sums by P_T position; positions the plan does not write stay NaN."""
        torch = self.torch
        d_x = torch.from_numpy(np.array(X, dtype=np.float64, order="C")).to("cuda:0")
        out = torch.full((self.n, self.dim), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        plan.repulse(d_x.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy()


_devs, _fast = {}, {}


def _dev(dim):
    if dim not in _devs:
        _devs[dim] = _Device(dim)
    return _devs[dim]


def _coords(d, degenerate=False):
    return C.degenerate(d) if degenerate else C.level()["X"][d]


def _rows(a):
    return slice(*C.span(a))


def _far_pass(ctx, d, X, **kw):
    """(Frep, info, {aggregate: layout}) of one pass of a FARFIELD plan through the hook."""
    plan = _dev(d).plan(ctx, mode=ge.MODE_FARFIELD, **kw)
    try:
        f = _dev(d).repulse(plan, X)
        info = plan.far_info()
        lays = {a: plan.far_layout(a) for a in info["aggregates"]}
        mode = plan.mode()
    finally:
        plan.close()
    assert info["active"] and info["reason"] == "active" and mode[0] == ge.MODE_FARFIELD
    return f, info, lays


def _fast_pass(ctx, d, X, key=None, **kw):
    """The FAST plan's hook output on X (cached under `key`, never modified)."""
    if key is not None and (d, key) in _fast:
        return _fast[d, key]
    plan = _dev(d).plan(ctx, mode=ge.MODE_FAST, **kw)
    try:
        assert plan.mode() == (ge.MODE_FAST, C.fast_items())
        f = _dev(d).repulse(plan, X)
    finally:
        plan.close()
    f.setflags(write=False)
    if key is not None:
        _fast[d, key] = f
    return f


def _streamed_mask():
    m = np.zeros(C.level()["n"], bool)
    for a in C.STREAMED:
        m[_rows(a)] = True
    return m


# -- 1. info and layout ----------------------------------------------------------------------

@pytest.mark.parametrize("d", C.DIMS)
def test_info_and_layout(ctx, d):
    """far_info is active and its counts are the restatement's; per far aggregate the layout
    is a permutation of its members, keys ascending with ties in P_T order, box and keys the
    restatement's bits and every cell and item ball cell_summary's bits
    (faml_far_cases.device_cells)."""
    X, m = _coords(d), C.masses()
    f, info, lays = _far_pass(ctx, d, X)
    bits = C.key_bits(d)
    assert info["aggregates"] == FAR_ALL and info["rows"] == sum(C.SIZES[a] for a in FAR_ALL)
    assert (info["item_rows"], info["key_bits"], info["theta"]) == (ROWS, bits, 0.5)
    assert info["far_min_ml"] == 257 and info["bad_boxes"] == 0
    acc, leaves, terms = np.zeros(F.MAX_LEVELS, dtype=np.int64), 0, 0
    for a in FAR_ALL:
        lay, Xa, ma, s = lays[a], X[_rows(a)], m[_rows(a)], C.SIZES[a]
        perm, keys = lay["perm"], lay["keys"]
        assert np.array_equal(np.sort(perm), np.arange(s))
        box = C.box_of(Xa, bits)
        assert np.array_equal(lay["box"], box)
        assert np.array_equal(keys, C.keys_of(Xa, box, bits)[perm])
        assert (keys[1:] >= keys[:-1]).all()
        tie = keys[1:] == keys[:-1]
        assert (perm[1:][tie] > perm[:-1][tie]).all()
        Xs, ms = Xa[perm], ma[perm]
        shape = F.level_shape(s)
        assert [len(c) for c in lay["cells"]] == [c for c, _ in shape]
        for cells, pts in list(zip(lay["cells"], [p for _, p in shape])) + [(lay["items"], ROWS)]:
            assert np.array_equal(cells, C.device_cells(Xs, ms, C.cell_ranges(s, pts))), (a, pts)
        got = F.accepted_counts(lay, s)
        acc[:len(got[0])] += got[0]
        leaves, terms = leaves + got[1], terms + got[2]
    assert info["accepted"] == list(acc) and info["exact_leaves"] == leaves
    assert info["pair_terms"] == terms
    assert np.isnan(f[~_streamed_mask()]).all() and np.isfinite(f[_streamed_mask()]).all()


# -- 2. the kernel computes the approximation it claims ----------------------------------------

def _check_items(f, lay, Xa, ma, repel, items):
    """Largest error / rounding term of the items' rows against the replay of the device's
    own layout in long double (f: the aggregate's rows by position)."""
    worst = 0.0
    for q in items:
        pos, Fa, T, terms, _ = F.replay_item(lay, q, Xa, ma, repel)
        got = f[lay["perm"][pos]]
        tol = 1.01 * (terms + F.K_TERM) * F.U * T
        bad = ~(np.abs(got - Fa) <= tol)
        assert not bad.any(), (q, np.argwhere(bad)[:4], got[bad][:4], Fa[bad][:4])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(tol > 0, np.abs(got - Fa) / tol, 0))))
    return worst


@pytest.mark.parametrize("repel", [1.0, 3.5])
@pytest.mark.parametrize("theta", [0.25, 0.5])
@pytest.mark.parametrize("d", C.DIMS)
def test_kernel_equals_replay(ctx, d, theta, repel):
    X, m = _coords(d), C.masses()
    f, info, lays = _far_pass(ctx, d, X, theta=theta, repel=repel)
    assert info["theta"] == theta
    worst = 0.0
    for a in FAR_ALL:
        worst = max(worst, _check_items(f[_rows(a)], lays[a], X[_rows(a)], m[_rows(a)], repel,
                                        C.sample_items(C.SIZES[a], ROWS)))
    print(f"d = {d} theta = {theta} repel = {repel}: largest error / rounding term {worst:.3f}")


@pytest.mark.parametrize("d", [2, 3])
def test_kernel_equals_replay_256_row_items(ctx, monkeypatch, d):
    monkeypatch.setenv("GE_FAR_R", "4")
    X, m = _coords(d), C.masses()
    f, info, lays = _far_pass(ctx, d, X)
    assert info["item_rows"] == 256
    for a in FAR_ALL:
        _check_items(f[_rows(a)], lays[a], X[_rows(a)], m[_rows(a)], 1.0,
                     C.sample_items(C.SIZES[a], 256))


# -- 3. the approximation meets the bound -------------------------------------------------------

@pytest.mark.parametrize("degenerate", [False, True], ids=["plain", "degenerate"])
@pytest.mark.parametrize("d", C.DIMS)
def test_bound_against_exact_sum(ctx, d, degenerate):
    """Sampled items of every far aggregate against the exact clamped sum over the
    aggregate's members in long double: error <= truncation + rounding."""
    X, m = _coords(d, degenerate), C.masses()
    f, info, lays = _far_pass(ctx, d, X)
    if degenerate:
        assert lays[C.A4097]["cells"][0][0, d + 1] == 0.0  # the clump's leaf
        assert not lays[C.A1025]["keys"].any() and lays[C.A1025]["box"][d] == 0.0
    assert np.isfinite(f[_streamed_mask()]).all()
    worst = 0.0
    for a in FAR_ALL:
        lay, Xa, ma, fa = lays[a], X[_rows(a)], m[_rows(a)], f[_rows(a)]
        mom = F.cell_moments(lay, Xa, ma)
        for q in C.sample_items(C.SIZES[a], ROWS):
            pos, _, T, terms, order = F.replay_item(lay, q, Xa, ma, 1.0)
            ids = lay["perm"][pos]
            Fx, _ = F.exact_rows(Xa, ma, 1.0, ids)
            err = np.sqrt(((fa[ids].astype(LD) - Fx) ** 2).sum(axis=1))
            bound = F.truncation_bound(lay, order, mom, Xa[ids], ma[ids]) + F.rounding(T, terms)
            assert (err <= bound).all(), (a, q, err.max(), bound.max())
            ok = bound > 0  # the coincident aggregate: every term is an exact 0
            if ok.any():
                worst = max(worst, float((err[ok] / bound[ok]).max()))
    print(f"d = {d} degenerate = {degenerate}: largest error / bound {worst:.3f}")
    assert sum(info["accepted"]) > 0


# -- 4. what the far field leaves alone ------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 5])
def test_resident_aggregates_keep_fast_bits(ctx, iterations):
    d = _dev(3)
    X0 = ge.uniform_stream(7, d.n * 3).reshape(d.n, 3)
    out = []
    for mode in (ge.MODE_FARFIELD, ge.MODE_FAST):
        plan = d.plan(ctx, iterations, mode=mode)
        try:
            out.append(d.run(ctx, plan, X0))
        finally:
            plan.close()
    res = np.concatenate([C.level()["PT"][1][_rows(a)] for a in C.RESIDENT])
    big = np.concatenate([C.level()["PT"][1][_rows(a)] for a in C.STREAMED])
    assert np.array_equal(out[0][res], out[1][res])
    assert np.isfinite(out[0]).all() and not np.array_equal(out[0][big], out[1][big])


@pytest.mark.parametrize("d", [2, 3])
def test_mixed_plan(ctx, monkeypatch, d):
    """GE_FAR_MIN_ML=1025: the aggregates of 257, 300 and 1024 members are FAST items with
    the FAST plan's bits; the others run the far field with the bits they have when every
    streamed aggregate does."""
    X = _coords(d)
    every, _, _ = _far_pass(ctx, d, X)
    fast = _fast_pass(ctx, d, X, key="plain")
    monkeypatch.setenv("GE_FAR_MIN_ML", "1025")
    plan = _dev(d).plan(ctx, mode=ge.MODE_FARFIELD)
    try:
        assert plan.mode() == (ge.MODE_FARFIELD, C.fast_items(1025))
        got = _dev(d).repulse(plan, X)
        info = plan.far_info()
        with pytest.raises(ge.GeError, match="1001"):
            plan.far_layout(C.SIZES.index(1024))
    finally:
        plan.close()
    assert info["aggregates"] == C.far_aggs(1025) and info["far_min_ml"] == 1025
    for a in C.STREAMED:
        want = every if a in info["aggregates"] else fast
        assert got[_rows(a)].tobytes() == want[_rows(a)].tobytes(), a
        assert not np.array_equal(every[_rows(a)], fast[_rows(a)])
    assert np.isnan(got[~_streamed_mask()]).all()
    sched = ge.faml_schedule(C.level()["PT"][0], d, 256, 4, mode=ge.MODE_FARFIELD)
    assert list(sched["faraggs"]) == C.far_aggs(1025)
    assert len(sched["fitems"]) == 4 * C.fast_items(1025)
    assert set(sched["fitems"].reshape(-1, 4)[:, 0]) == set(C.STREAMED) - set(C.far_aggs(1025))


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_box(ctx, bad):
    """One coordinate of the 4097-member aggregate is not finite: the device flag rejects
    every cell of that aggregate and its rows are FAST's bits; the others are unchanged."""
    d = 3
    clean, _, _ = _far_pass(ctx, d, _coords(d))
    X = _coords(d).copy()
    b, _ = C.span(C.A4097)
    X[b + 1234, 1] = bad
    got, info, lays = _far_pass(ctx, d, X)
    fast = _fast_pass(ctx, d, X)
    assert info["bad_boxes"] == 1
    assert not lays[C.A4097]["keys"].any()
    assert np.array_equal(lays[C.A4097]["perm"], np.arange(4097))
    assert not np.isfinite(fast[_rows(C.A4097)]).all()
    for a in FAR_ALL:
        want = fast if a == C.A4097 else clean
        assert got[_rows(a)].tobytes() == want[_rows(a)].tobytes(), a


def test_theta_zero_is_fast_within_rounding(ctx):
    d = 2
    X, m = _coords(d, degenerate=True), C.masses()
    f, info, lays = _far_pass(ctx, d, X, theta=0.0)
    fast = _fast_pass(ctx, d, X)
    for a in FAR_ALL:
        s, Xa, ma = C.SIZES[a], X[_rows(a)], m[_rows(a)]
        for l, cells in enumerate(lays[a]["cells"]):  # only cells of radius 0 can be accepted
            if (cells[:, d + 1] > 0).all():
                assert not any(ok and lv == l for q in C.sample_items(s, ROWS)
                               for lv, _, ok in F.walk(lays[a], q, s))
        # sum_j |t_ijk| of every row in float64, by torch on the device (its own error,
        # about s 2^-53 relative, is inside the factor 1.01)
        import torch
        xt, mt = torch.from_numpy(Xa.copy()).to("cuda:0"), torch.from_numpy(ma.copy()).to("cuda:0")
        T = np.empty((s, d))
        for r0 in range(0, s, 2048):
            e = xt[r0:r0 + 2048, None, :] - xt[None, :, :]
            dis = torch.clamp((e * e).sum(dim=2).sqrt(), min=F.KFAEPS)
            w = mt[r0:r0 + 2048, None] * mt[None, :] / dis ** 3
            T[r0:r0 + 2048] = (e.abs() * w[:, :, None]).sum(dim=1).cpu().numpy()
        err = np.abs(f[_rows(a)] - fast[_rows(a)])
        assert (err <= 2 * 1.01 * (s + F.K_TERM) * F.U * T).all(), a
    assert info["accepted"][0] > 0  # the clump's leaf, from far items


# -- 5. determinism and cuts -------------------------------------------------------------------------

def test_runs_plans_and_subsets_agree(ctx):
    d = _dev(3)
    X0 = ge.uniform_stream(11, d.n * 3).reshape(d.n, 3)
    kw = dict(mode=ge.MODE_FARFIELD, repel=3.5)
    m = C.level()["m"]
    cuts = [[list(range(0, m, 2)), list(range(1, m, 2))],
            [list(range(k, m, 3)) for k in range(3)]]
    whole, other = d.plan(ctx, 3, **kw), d.plan(ctx, 3, **kw)
    try:
        a = d.run(ctx, whole, X0)
        assert np.array_equal(a, d.run(ctx, whole, X0))  # two runs of one plan
        assert np.array_equal(a, d.run(ctx, other, X0))  # two plans
    finally:
        whole.close()
        other.close()
    pip, pix = C.level()["PT"]
    for cut in cuts:
        parts = np.zeros_like(a)
        for aggs in cut:
            plan = d.plan(ctx, 3, aggs=aggs, **kw)
            try:
                far = [x for x in FAR_ALL if x in aggs]
                assert plan.far_info()["aggregates"] == far
                assert plan.mode() == (ge.MODE_FARFIELD if far else ge.MODE_STRICT, 0)
                mem = np.concatenate([pix[pip[x]:pip[x + 1]] for x in aggs])
                parts[mem] = d.run(ctx, plan, X0)[mem]
            finally:
                plan.close()
        assert np.array_equal(a, parts)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_SHARD = dict(dim=3, iterations=3, repel=3.5, seed=23)


def _shard_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      GE_DIST_SPLIT_MIN=str(max(C.SIZES)), GE_FAML_RES_CAP=C.RES_CAP,
                      GE_FAR_MIN_ML="257")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = ge.Context(0)
    comm = ge.Comm(ctx, world, rank, backend="transport")
    lv = C.level()
    dim = _SHARD["dim"]
    X = comm.force_atlas_ml(lv["A"], lv["PT"], lv["vA"], lv["cA"][dim], lv["rA"], dim,
                            iterations=_SHARD["iterations"], seed=_SHARD["seed"],
                            mode=ge.MODE_FARFIELD, repel=_SHARD["repel"])
    np.save(out_path % rank, X)
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


def test_shard_with_split_aggregate(tmp_path, ctx):
    """A 2-rank transport shard with the 16449-member aggregate split by force: the split
    aggregate has FAST's bits, the whole ones the whole plan's far-field bits."""
    import torch.multiprocessing as mp
    lv = C.level()
    dim = _SHARD["dim"]
    owner = ge.assign_aggregates_split(lv["PT"], lv["A"][0], 2, max(C.SIZES))
    assert list(np.flatnonzero(owner == -1)) == [C.A16449]
    args = (lv["A"], lv["PT"], lv["vA"], lv["cA"][dim], lv["rA"], dim)
    kw = dict(iterations=_SHARD["iterations"], seed=_SHARD["seed"], repel=_SHARD["repel"])
    far = ctx.force_atlas_ml(*args, mode=ge.MODE_FARFIELD, **kw)
    fast = ctx.force_atlas_ml(*args, mode=ge.MODE_FAST, **kw)
    out = str(tmp_path / "s%d.npy")
    mp.start_processes(_shard_worker, args=(2, _free_port(), out), nprocs=2, join=True,
                       start_method="spawn")
    pip, pix = lv["PT"]
    for r in range(2):
        got = np.load(out % r)
        for a in range(lv["m"]):
            v = pix[pip[a]:pip[a + 1]]
            assert np.array_equal(got[v], (fast if a == C.A16449 else far)[v]), (r, a)
    v = pix[_rows(C.A16449)]
    assert not np.array_equal(far[v], fast[v])


# -- 6. fall-backs and reasons ---------------------------------------------------------------------------

def _same_as_fast(ctx, dev, X, reason, **kw):
    out = []
    for mode in (ge.MODE_FARFIELD, ge.MODE_FAST):
        plan = dev.plan(ctx, mode=mode, **kw)
        try:
            if mode == ge.MODE_FARFIELD:
                info = plan.far_info()
                assert not info["active"] and info["reason"] == reason
                assert not info["aggregates"] and plan.mode()[0] != ge.MODE_FARFIELD
                with pytest.raises(ge.GeError, match="1001"):
                    plan.far_layout(C.A16449)
            out.append((dev.repulse(plan, X), plan.mode()))
        finally:
            plan.close()
    assert out[0][1] == out[1][1]
    assert out[0][0].tobytes() == out[1][0].tobytes()
    return out[0]


def test_falls_back_to_fast_bits(ctx, monkeypatch):
    X5 = np.random.RandomState(5).uniform(-1, 1, (C.level()["n"], 5))
    cA5 = np.random.RandomState(6).uniform(-1, 1, (C.level()["m"], 5))
    _, mode = _same_as_fast(ctx, _Device(5, cA=cA5), X5, "dim")
    assert mode == (ge.MODE_STRICT, 0)
    monkeypatch.setenv("GE_WIDE_MIN_DIM", "3")
    _, mode = _same_as_fast(ctx, _dev(3), _coords(3), "dim")
    assert mode == (ge.MODE_STRICT, 0)
    monkeypatch.delenv("GE_WIDE_MIN_DIM")
    # one member of the 4097 aggregate with internal deg + 1 <= 0
    lv = C.level()
    ip, ix, dx = (a.copy() for a in lv["A"])
    v = int(lv["PT"][1][C.span(C.A4097)[0] + 77])
    for e in range(ip[v], ip[v + 1]):
        u = ix[e]
        dx[e] = -2.0
        dx[ip[u] + int(np.searchsorted(ix[ip[u]:ip[u + 1]], v))] = -2.0
    _, mode = _same_as_fast(ctx, _Device(3, A=(ip, ix, dx)), _coords(3), "mass")
    assert mode == (ge.MODE_FAST, C.fast_items())
    plan = _Device(3, A=(ip, ix, dx)).plan(ctx, mode=ge.MODE_FARFIELD, use_weights=0)
    try:  # unweighted, every mass is a count + 1
        assert plan.far_info()["active"]
    finally:
        plan.close()


def test_default_far_min_ml(ctx, monkeypatch):
    """Without the override only aggregates of at least the default (never below 4096)
    take the far field; a plan over the smaller ones reports GE_FAR_SMALL and is a FAST
    plan."""
    monkeypatch.delenv("GE_FAR_MIN_ML")
    plan = _dev(3).plan(ctx, mode=ge.MODE_FARFIELD)
    try:
        info = plan.far_info()
    finally:
        plan.close()
    assert info["far_min_ml"] >= 4096
    assert info["aggregates"] == C.far_aggs(info["far_min_ml"])
    small = [a for a in range(C.level()["m"]) if C.SIZES[a] < info["far_min_ml"]]
    _, mode = _same_as_fast(ctx, _dev(3), _coords(3), "small", aggs=small)
    assert mode[0] == ge.MODE_FAST


@pytest.mark.parametrize("theta", [1.0, float("nan")])
def test_bad_theta_is_an_argument_error(ctx, theta):
    with pytest.raises(ge.GeError, match="1001.*theta"):
        _dev(2).plan(ctx, mode=ge.MODE_FARFIELD, theta=theta)
    _dev(2).plan(ctx, mode=ge.MODE_FAST, theta=theta).close()  # read in no other mode


# -- 7. whole runs and entry points -------------------------------------------------------------------------

@pytest.mark.parametrize("d", [2, 3])
def test_horizon_sanity(ctx, d):
    """100 iterations: finite, every streamed member inside its aggregate's ball."""
    lv, dev = C.level(), _dev(d)
    plan = dev.plan(ctx, 100, mode=ge.MODE_FARFIELD)
    try:
        got = dev.run(ctx, plan, ge.uniform_stream(3, dev.n * d).reshape(dev.n, d))
    finally:
        plan.close()
    assert np.isfinite(got).all()
    pip, pix = lv["PT"]
    for a in C.STREAMED:
        r = float(lv["rA"][a])
        norms = np.sqrt(((got[pix[pip[a]:pip[a + 1]]] - lv["cA"][d][a]) ** 2).sum(axis=1))
        assert (norms <= r * (1 + 1e-12)).all() and abs(norms.max() - r) <= 1e-12 * r, a


def test_force_atlas_ml_equals_plan_run(ctx):
    lv, dev, seed = C.level(), _dev(3), 31
    kw = dict(mode=ge.MODE_FARFIELD, theta=0.25, repel=3.5)
    plan = dev.plan(ctx, 3, **kw)
    try:
        want = dev.run(ctx, plan, ge.uniform_stream(seed, dev.n * 3).reshape(dev.n, 3))
    finally:
        plan.close()
    args = (lv["A"], lv["PT"], lv["vA"], lv["cA"][3], lv["rA"], 3)
    got = ctx.force_atlas_ml(*args, iterations=3, seed=seed, **kw)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, ctx.force_atlas_ml(*args, iterations=3, seed=seed,
                                                      **dict(kw, theta=0.5)))


def test_embed_entry(ctx, oracle, monkeypatch):
    """ge_embed(mode=FARFIELD) with the override: finite, differs from FAST where the
    finest level has far aggregates, and equals it bit for bit without one."""
    A = G.largest_component(G.rmat(6000, 40000, seed=41))
    hier = oracle.partition(A, 0.07)
    assert int((np.diff(hier[0][0]) > 256).sum()) >= 1
    As = oracle.hierarchy_As(A, hier)
    kw = dict(seed=11, base_iterations=0, ml_iterations=4)
    far = ctx.embed(As, hier, 3, mode=ge.MODE_FARFIELD, **kw)
    fast = ctx.embed(As, hier, 3, mode=ge.MODE_FAST, **kw)
    assert np.isfinite(far).all() and not np.array_equal(far, fast)
    monkeypatch.setenv("GE_FAR_MIN_ML", "100000")
    assert np.array_equal(ctx.embed(As, hier, 3, mode=ge.MODE_FARFIELD, **kw), fast)


def test_dropin_reproduces_the_binding(tmp_path, ctx):
    """forceAtlasMultilevel through the drop-in header: partition::setMode(GE_MODE_FARFIELD)
    with setTheta, and $GE_MODE=farfield with $GE_THETA, reproduce the binding's bits."""
    lv = C.level()
    dim, seed, iterations, repel, theta = 2, 31, 2, 3.5, 0.25
    exe = str(tmp_path / "faml_far_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "faml_far_driver.cpp"), f"-L{PKG}/lib",
                           "-lge", f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    inp = str(tmp_path / "level.bin")
    A, PT = lv["A"], lv["PT"]
    with open(inp, "wb") as f:
        np.array([lv["n"], len(A[1]), lv["m"]], dtype=np.int32).tofile(f)
        for a, dt in ((A[0], np.int32), (A[1], np.int32), (A[2], np.float64), (PT[0], np.int32),
                      (PT[1], np.int32), (lv["cA"][dim], np.float64), (lv["rA"], np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(f)
    args = (A, PT, lv["vA"], lv["cA"][dim], lv["rA"], dim)
    kw = dict(iterations=iterations, seed=seed, repel=repel)
    want = ctx.force_atlas_ml(*args, mode=ge.MODE_FARFIELD, theta=theta, **kw)
    assert not np.array_equal(want, ctx.force_atlas_ml(*args, mode=ge.MODE_FAST, **kw))
    assert not np.array_equal(want, ctx.force_atlas_ml(*args, mode=ge.MODE_FARFIELD, theta=0.75,
                                                       **kw))
    base = {k: v for k, v in os.environ.items() if k not in ("GE_MODE", "GE_THETA")}
    for how, extra in (("set", {}), ("env", {"GE_MODE": "farfield", "GE_THETA": str(theta)})):
        out = str(tmp_path / f"x_{how}.bin")
        r = subprocess.run([exe, inp, out, str(dim), str(seed), str(iterations), repr(repel), how,
                            str(theta)], capture_output=True, text=True, timeout=120,
                           env={**base, **extra})
        assert r.returncode == 0, (how, r.stderr)
        assert np.array_equal(np.fromfile(out, dtype=np.float64).reshape(-1, dim), want), how
