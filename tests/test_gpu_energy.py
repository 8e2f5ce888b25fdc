"""The layout energy on the device (ge_fa_plan_energy, ge_layout_energy,
ge_layout_energy_dist, partition::layoutEnergy; graph-embed_amd/csrc/ge_energy.hip) on the
inputs of tests/energy_cases.py, whose docstring derives every bound used here by counting
roundings; tests/test_energy_cases.py shows on the CPU that a float64 restatement of the
kernels' order meets them.  None is tuned to the device.

Measured on an MI355X, largest |error| / bound over the rows, columns and cases of an
input (each case prints its figure before it asserts):
    rows / totals
    n = 1, 2, 5                 0.12, 0.28, 0.36 / 0.04, 0.07, 0.10
    n = 255, 256, 257           0.44, 0.42, 0.38 / 0.06, 0.08, 0.08
    n = 1 023, 1 024, 1 025     0.43, 0.46, 0.46 / 0.06, 0.08, 0.08
    n = 4 096, 4 097            0.48, 0.49 / 0.05, 0.10
    degenerate 257, 1 025, 4 097   0.38, 0.46, 0.49 / 0.08, 0.09, 0.08
    n = 1 025 x1e9, x1e-300     0.48, 0.19 / 0.08, 0.01
    hub, its seven cases        0.39 / 0.06
    d = 5, 8, 16 at n = 257     0.34, 0.30, 0.26 / 0.08, 0.05, 0.05;  at n = 1 025  0.37, 0.30, 0.22 / 0.13, 0.05, 0.09
The row figure is the largest over the five columns, short sums with a handful of roundings
to spare included.  The uniform layout of the n = 1 025 ring with chords has a relative edge
length of 1.003.
"""
import os
import socket
import subprocess

import numpy as np
import pytest

import energy_cases as E
import fa_fast_cases as C
import ge_amd as ge
import graphs as G
from test_dropin import HERE, PKG, REPO, write_csr

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD = 3     # rows past the plan's last one in the output buffer: they keep the sentinel
NAN_ROWS = 16  # kEnergyJBlocks rows of NaN behind the coordinates


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GE_MODE", "GE_WIDE_MIN_DIM", "GE_SMALL_MAX", "GE_FA_SYM", "GE_NO_GRAPH",
              "GE_STREAM_MAX", "GE_FAR_MIN", "GE_FAR_R"):
        monkeypatch.delenv(k, raising=False)


class Dev:
    """A graph on the device (uploaded once per key) and plans over it."""

    def __init__(self, ctx, A):
        import torch
        self.torch, self.ctx = torch, ctx
        self.n, self.nnz = len(A[0]) - 1, len(A[1])
        self.dev = torch.device("cuda:0")
        self.A = [torch.from_numpy(np.array(a)).to(self.dev) for a in A]
        if self.nnz == 0:  # n = 1: no entries, but the pointers must not be null
            self.A[1] = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self.A[2] = torch.zeros(1, dtype=torch.float64, device=self.dev)

    def up(self, X):
        """X on the device as the first rows of a buffer that ends in 16 rows of NaN: a
        partner read past row n - 1 poisons every sum of its row."""
        n, d = X.shape
        buf = self.torch.full((n + NAN_ROWS, d), float("nan"), dtype=self.torch.float64,
                              device=self.dev)
        buf[:n] = self.torch.from_numpy(np.array(X, np.float64)).to(self.dev)  # the inputs are read-only
        return buf[:n]

    def plan(self, d, rb=0, re=None, **kw):
        re = self.n if re is None else re
        return self.ctx.fa_plan(self.n, self.nnz, *(t.data_ptr() for t in self.A), d, rb, re, **kw)

    def energy(self, plan, x, rb=0, re=None, out=None):
        """(rows buffer, totals): the plan's rows land at their own place in an (n + GUARD)
        x 5 buffer full of SENTINEL (or in `out`)."""
        if out is None:
            out = self.torch.full((self.n + GUARD, E.COLS), SENTINEL, dtype=self.torch.float64,
                                  device=self.dev)
        self.torch.cuda.synchronize()
        totals = plan.energy(x.data_ptr(), out.data_ptr() + rb * E.COLS * 8)
        return out, totals


_devs = {}


def _dev(ctx, key, A=None):
    if key not in _devs:
        _devs[key] = Dev(ctx, C.case(key)[0] if A is None else A)
    return _devs[key]


def _whole(ctx, dv, d, X, **kw):
    p = dv.plan(d, **kw)
    try:
        out, tot = dv.energy(p, dv.up(X))
        return out.cpu().numpy(), tot
    finally:
        p.close()


def _rows_and_totals(dv, d, X, kw, A, R, T, p, m, what, finite=True):
    """Tests 1 and 2 on one input and case: the rows within their bounds, the same bits on
    a second call, nothing written past the rows; the totals within theirs and bit-equal
    to the numpy restatement of the reduction applied to the device's own rows."""
    n = dv.n
    x = dv.up(X)
    plan = dv.plan(d, **kw)
    try:
        out, tot = dv.energy(plan, x)
        out2, tot2 = dv.energy(plan, x)
        none_tot = plan.energy(x.data_ptr())  # d_rows = NULL
    finally:
        plan.close()
    got, again = out.cpu().numpy(), out2.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    got, again = got[:n], again[:n]
    B = E.bounds(A, d, T, p, abs(p["gravity"]) * np.abs(m))
    worst, ok = E.ratio(got, R, B)
    terr = np.abs(tot.astype(E.LD) - R.sum(axis=0))
    tb = E.totals_bound(B, T)
    tworst = float((terr[tb > 0] / tb[tb > 0]).max()) if (tb > 0).any() else 0.0
    print(f"{what}: rows max |err| / bound = {worst:.4f}, totals {tworst:.4f}")
    if finite:
        assert np.isfinite(got).all()
    assert got.tobytes() == again.tobytes() and tot.tobytes() == tot2.tobytes()
    assert tot.tobytes() == none_tot.tobytes()
    assert ok, (what, worst)
    assert (terr <= tb).all(), (what, tworst)
    assert tot.tobytes() == E.reduce_totals(got).tobytes()
    return got, tot


# --------------------------------------------------------------------------
# 1, 2. rows and totals against the long-double reference

@pytest.mark.parametrize("dim,repel,use_weights", E.CASES, ids=E.CASE_IDS)
@pytest.mark.parametrize("n,variant", E.INPUTS, ids=E.INPUT_IDS)
def test_rows_and_totals(ctx, n, variant, dim, repel, use_weights):
    dv = _dev(ctx, n)
    R, T = E.reference(n, variant, dim, repel, use_weights)
    p = E.params(repel=repel, use_weights=use_weights)
    got, tot = _rows_and_totals(dv, dim, C.coords(n, dim, variant),
                                dict(repel=repel, use_weights=use_weights), C.case(n)[0], R, T, p,
                                C.masses(n, use_weights), f"n={n} {variant} d={dim} {repel=} w={use_weights}")
    if n == 1:
        assert not got[:, [E.REP, E.ATT, E.PAIRDIST, E.EDGELEN]].any()
    if n == 1025 and variant == "plain" and dim == 3:
        lam = ge.relative_edge_length(tot, n, len(C.case(n)[0][1]))
        print(f"relative edge length of the uniform layout: {lam:.4f}")
        assert abs(lam - 1.0) < 0.05  # a random layout: edges as long as any pair


@pytest.mark.parametrize("linlog,nohubs,delta,w", E.HUB_CASES, ids=E.HUB_IDS)
def test_rows_and_totals_on_the_hub_input(ctx, linlog, nohubs, delta, w):
    A, X = E.hub()
    dv = _dev(ctx, "hub", A)
    R, T = E.hub_reference(linlog, nohubs, delta, w)
    p = E.hub_params(linlog, nohubs, delta, w)
    kw = {k: p[k] for k in ("repel", "attract", "gravity", "delta", "use_weights", "linlog", "nohubs")}
    _rows_and_totals(dv, E.HUB_D, X, kw, A, R, T, p, E.masses(A, w),
                     f"hub {linlog=} {nohubs=} {delta=} {w=}")


# --------------------------------------------------------------------------
# 3. row cuts

@pytest.mark.parametrize("n,cuts", [(1025, [(0, 1), (1, 1024), (1024, 1025)]),
                                    (4097, [(0, 4096), (4096, 4097)])])
@pytest.mark.parametrize("d", [3, 2])
def test_row_cuts_equal_the_whole_plan(ctx, n, cuts, d):
    dv = _dev(ctx, n)
    X = C.coords(n, d, "degenerate")
    x = dv.up(X)
    want, want_tot = _whole(ctx, dv, d, X, repel=3.5)
    out = dv.torch.full((n + GUARD, E.COLS), SENTINEL, dtype=dv.torch.float64, device=dv.dev)
    done = np.zeros(n, bool)
    for rb, re in cuts:
        p = dv.plan(d, rb, re, repel=3.5, mode=ge.MODE_FAST)
        try:
            _, tot = dv.energy(p, x, rb, re, out=out)
        finally:
            p.close()
        done[rb:re] = True
        got = out.cpu().numpy()
        assert (got[n:] == SENTINEL).all() and (got[:n][~done] == SENTINEL).all(), (rb, re)
        assert got[:n][done].tobytes() == want[:n][done].tobytes(), (rb, re)
        assert tot.tobytes() == E.reduce_totals(got[rb:re]).tobytes()  # over the plan's rows
    assert done.all()
    assert want_tot.tobytes() == E.reduce_totals(want[:n]).tobytes()


# --------------------------------------------------------------------------
# 4. mode independence, and the plan is not disturbed

def test_modes_give_the_same_bits_and_steps_are_not_disturbed(ctx, monkeypatch):
    n, d = 4097, 3
    dv = _dev(ctx, n)
    t = dv.torch
    X = C.coords(n, d)
    monkeypatch.setenv("GE_FAR_MIN", "4096")
    outs = {}
    for name, mode in (("STRICT", ge.MODE_STRICT), ("FAST", ge.MODE_FAST),
                       ("FARFIELD", ge.MODE_FARFIELD)):
        x = dv.up(X)
        a, b = t.empty_like(x), t.empty_like(x)
        plain = dv.plan(d, mode=mode)
        mixed = dv.plan(d, mode=mode)
        try:
            if mode == ge.MODE_FARFIELD:
                assert mixed.far_info()["active"]
            cur, nxt = x, a
            for _ in range(3):
                plain.step(cur.data_ptr(), nxt.data_ptr())
                cur, nxt = nxt, (b if nxt is a else a)
            ctx.sync()
            want = cur.cpu().numpy()
            x2 = dv.up(X)
            a2, b2 = t.empty_like(x2), t.empty_like(x2)
            rows, tot = dv.energy(mixed, x2)
            outs[name] = (rows.cpu().numpy(), tot)
            cur, nxt = x2, a2
            for _ in range(3):
                mixed.step(cur.data_ptr(), nxt.data_ptr())
                dv.energy(mixed, nxt)
                cur, nxt = nxt, (b2 if nxt is a2 else a2)
            ctx.sync()
            assert cur.cpu().numpy().tobytes() == want.tobytes(), name
            assert np.isfinite(want).all()
        finally:
            plain.close()
            mixed.close()
    for name in ("FAST", "FARFIELD"):
        assert outs[name][0].tobytes() == outs["STRICT"][0].tobytes(), name
        assert outs[name][1].tobytes() == outs["STRICT"][1].tobytes(), name


# --------------------------------------------------------------------------
# 5. coordinates that are not finite

@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("d", [1, 3])
def test_non_finite_coordinate(ctx, d, bad):
    n, v = 257, 100
    dv = _dev(ctx, n)
    A = C.case(n)[0]
    X = C.coords(n, d)
    X[v, d // 2] = bad
    got, tot = _whole(ctx, dv, d, X)
    got = got[:n]
    nb = np.zeros(n, bool)
    nb[A[1][A[0][v]:A[0][v + 1]]] = True
    nb[v] = True
    assert np.isnan(got[v]).all()
    assert np.isnan(got[:, [E.REP, E.PAIRDIST]]).all()
    for c in (E.ATT, E.EDGELEN):
        assert np.array_equal(np.isnan(got[:, c]), nb), c
    assert np.array_equal(np.isnan(got[:, E.GRAV]), np.arange(n) == v)
    assert not np.isinf(got).any()
    assert np.isnan(tot).all()


# --------------------------------------------------------------------------
# 6. dimensions 5, 8, 16

@pytest.mark.parametrize("d", E.WIDE_DIMS)
@pytest.mark.parametrize("n", E.WIDE_SIZES)
def test_rows_and_totals_above_four_dimensions(ctx, n, d):
    dv = _dev(ctx, n)
    R, T = E.wide_reference(n, d)
    _rows_and_totals(dv, d, E.wide_coords(n, d), {}, C.case(n)[0], R, T, E.params(),
                     C.masses(n, 1), f"n={n} d={d}")


# --------------------------------------------------------------------------
# 7. the host-array form

def test_layout_energy_equals_the_plan(ctx):
    A, X = E.hub()
    dv = _dev(ctx, "hub", A)
    kw = dict(repel=3.5, attract=0.75, gravity=2.0, linlog=1, delta=0.5)
    want, want_tot = _whole(ctx, dv, E.HUB_D, X, **kw)
    rows, tot = ctx.layout_energy(A, X, **kw)
    assert rows.tobytes() == want[:dv.n].tobytes() and tot.tobytes() == want_tot.tobytes()
    none, tot2 = ctx.layout_energy(A, X, rows=False, **kw)
    assert none is None and tot2.tobytes() == tot.tobytes()
    n = 1
    rows, tot = ctx.layout_energy(C.case(n)[0], C.coords(n, 2))
    assert rows.shape == (1, E.COLS) and not rows[0, [E.REP, E.ATT, E.PAIRDIST, E.EDGELEN]].any()
    for dim in (0, 17):
        with pytest.raises(ge.GeError, match="1..16"):
            ctx.layout_energy(A, np.zeros((dv.n, dim)))


# --------------------------------------------------------------------------
# 8. two ranks

DIST_N = 1148


def _dist_inputs():
    A = G.with_hubs(G.rmat(DIST_N, 8 * DIST_N, seed=17), [(3, 600)], seed=3)
    return A, G.random_coords(DIST_N, 3, seed=4), dict(repel=1.5, gravity=2.0, linlog=1)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = ge.Context(0)
    comm = ge.Comm(ctx, world, rank, backend="transport")
    A, X, kw = _dist_inputs()
    rows, tot = comm.layout_energy(A, X, **kw)
    _, tot_only = comm.layout_energy(A, X, rows=False, **kw)
    # n = 1 on two ranks: rank 1's shard is empty
    rows1, tot1 = comm.layout_energy(C.case(1)[0], C.coords(1, 2), **kw)
    np.savez(out_path % rank, rows=rows, tot=tot, tot_only=tot_only, rows1=rows1, tot1=tot1)
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_transport_ranks_match_single_gpu(ctx, tmp_path):
    import torch.multiprocessing as mp
    A, X, kw = _dist_inputs()
    assert len(A[0]) - 1 == DIST_N
    rows, tot = ctx.layout_energy(A, X, **kw)
    assert np.isfinite(rows).all()
    rows1, tot1 = ctx.layout_energy(C.case(1)[0], C.coords(1, 2), **kw)
    out = str(tmp_path / "r%d.npz")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True,
                       start_method="spawn")
    for r in range(2):
        got = dict(np.load(out % r))
        assert got["rows"].tobytes() == rows.tobytes(), r
        assert got["tot"].tobytes() == tot.tobytes() == got["tot_only"].tobytes(), r
        assert got["rows1"].tobytes() == rows1.tobytes() and got["tot1"].tobytes() == tot1.tobytes(), r


# --------------------------------------------------------------------------
# 9. the drop-in header

def test_dropin_layout_energy(ctx, tmp_path):
    exe = str(tmp_path / "energy_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "energy_driver.cpp"), f"-L{PKG}/lib", "-lge",
                           f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    A, X = E.hub()
    paths = [str(tmp_path / f) for f in ("a.bin", "x.bin", "t.bin")]
    write_csr(paths[0], A)
    np.ascontiguousarray(X).tofile(paths[1])
    r = subprocess.run([exe, paths[0], paths[1], str(E.HUB_D), paths[2]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(paths[2], dtype=np.float64).reshape(2, E.COLS)
    assert got[0].tobytes() == ctx.layout_energy(A, X)[1].tobytes()
    want = ctx.layout_energy(A, X, repel=3.5, attract=0.75, gravity=2.0, use_weights=1, linlog=1,
                             nohubs=1, delta=0.5)[1]
    assert got[1].tobytes() == want.tobytes()
