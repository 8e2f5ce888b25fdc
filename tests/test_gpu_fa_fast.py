"""GE_MODE_FAST on the single level (fa_repulse_fast and fa_reduce_parts,
graph-embed_amd/csrc/ge_fa.hip, around fast_rep_pair, ge_pair.hpp) on the inputs of
tests/fa_fast_cases.py: sizes on every edge of the kernel's tiling (tile tails, the j-chunk
split, the row block), degenerate points and two scales.

The force-level bound, per row i and component k with u = 2^-53,
    |F_ik - F*_ik| <= 1.01 (n + 16 + 24) u sum_{j != i} |t_ijk|
against the long-double sum of include/forceatlas.hpp:148-167, clamp included; the
derivation is in tests/fa_fast_cases.py's docstring (24 u the term, n u the chunk chains,
16 u the reduce), and tests/test_fa_fast_cases.py shows on the CPU that a float64
restatement of the kernel's order meets it on every input.  The bound is not tuned to the
device.  Measured on an MI355X, largest |error| / bound over the 7 cases of an input
(each case prints its figures before it asserts), FAST / STRICT:
    n = 2, 5               0.052, 0.101 / 0.075, 0.082  (few terms: the term error dominates)
    n = 255, 256, 257      0.046, 0.082, 0.048 / 0.046, 0.064, 0.053
    n = 1 023, 1 024, 1 025   0.024, 0.020, 0.017 / 0.029, 0.049, 0.033
    n = 4 096, 4 097         0.0056, 0.0047 / 0.022, 0.021
    degenerate 257, 1 025, 4 097   0.048, 0.016, 0.0049 / 0.051, 0.034, 0.021
    n = 1 025 x1e9, x1e-300  0.017, 0.0082 / 0.044, 0.030
The worst case n u of the chains dominates the bound and random roundings use ~sqrt(n) u of
it; FAST's 16 short chains stay below STRICT's one sum per row from n ~ 1 000 up.  FAST
against STRICT after 2 iterations at n = 1 025 (test_fast_mode_tolerance): 1.3e-12 / 3.9e-13 /
1.1e-15 at d = 1 / 2 / 4.
"""
import numpy as np
import pytest

import fa_fast_cases as C
import fa_route as route
import ge_amd as ge
from faml_fast_cases import REL_TOL_FAST

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD = 3  # rows past the plan's last one in the output buffer: they keep the sentinel


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GE_MODE", "GE_WIDE_MIN_DIM", "GE_SMALL_MAX", "GE_FA_SYM", "GE_NO_GRAPH",
              "GE_STREAM_MAX", "GE_GRP_SPLIT", "GE_ROWS_TILES", "GE_REP_BLOCKS", "GE_GRP_G"):
        monkeypatch.delenv(k, raising=False)


class Dev:
    """The n-vertex graph on the device (uploaded once per size) and plans over it."""

    def __init__(self, ctx, n):
        import torch
        self.torch, self.ctx, self.n = torch, ctx, n
        self.dev = torch.device("cuda:0")
        A = C.case(n)[0]
        self.nnz = len(A[1])
        self.A = [torch.from_numpy(np.array(a)).to(self.dev) for a in A]  # case()'s are read-only
        if self.nnz == 0:  # n = 1: no entries, but the pointers must not be null
            self.A[1] = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self.A[2] = torch.zeros(1, dtype=torch.float64, device=self.dev)

    def up(self, X):
        """X on the device as the first rows of a buffer that ends in kFastJBlocks rows of
        NaN: a partner read past row n - 1 (a chunk that does not stop at n overruns by
        fewer than jb rows) turns every sum NaN, whatever its mass reads as."""
        n, d = X.shape
        buf = self.torch.full((n + C.FAST_JBLOCKS, d), float("nan"), dtype=self.torch.float64,
                              device=self.dev)
        buf[:n] = self.torch.from_numpy(np.ascontiguousarray(X, np.float64)).to(self.dev)
        return buf[:n]

    def plan(self, d, rb=0, re=None, **kw):
        re = self.n if re is None else re
        return self.ctx.fa_plan(self.n, self.nnz, *(t.data_ptr() for t in self.A), d, rb, re, **kw)

    def repulse(self, plan, x, rb=0, re=None, out=None):
        """One pass into rows [rb, re) of an (n + GUARD) x d buffer full of SENTINEL (or
        of `out`): the plan's rows land at their own place."""
        re = self.n if re is None else re
        d = x.shape[1]
        if out is None:
            out = self.torch.full((self.n + GUARD, d), SENTINEL, dtype=self.torch.float64,
                                  device=self.dev)
        self.torch.cuda.synchronize()
        plan.repulse(x.data_ptr(), out.data_ptr() + rb * d * 8)
        return out


_devs = {}


def _dev(ctx, n):
    if n not in _devs:
        _devs[n] = Dev(ctx, n)
    return _devs[n]


def _fast_whole(ctx, n, d, X, **kw):
    dv = _dev(ctx, n)
    p = dv.plan(d, mode=ge.MODE_FAST, **kw)
    try:
        return dv.repulse(p, dv.up(X)).cpu().numpy()[:n]
    finally:
        p.close()


# --------------------------------------------------------------------------
# 1. force level, derived bound

@pytest.mark.parametrize("dim,repel,use_weights", C.CASES, ids=C.CASE_IDS)
@pytest.mark.parametrize("n,variant", C.INPUTS, ids=C.INPUT_IDS)
def test_force_bound(ctx, n, variant, dim, repel, use_weights):
    """FaPlan.repulse under FAST, and under STRICT for a figure to compare with, against
    the long-double reference and the bound of the module docstring."""
    dv = _dev(ctx, n)
    X = C.coords(n, dim, variant)
    Fr, T = C.reference(n, variant, dim, repel, use_weights)
    x = dv.up(X)
    assert route.repulse_kernel(n, dim, mode=ge.MODE_FAST, repel=repel,
                                use_weights=use_weights) == "fa_repulse_fast"
    for name, mode in (("FAST", ge.MODE_FAST), ("STRICT", ge.MODE_STRICT)):
        plan = dv.plan(dim, mode=mode, repel=repel, use_weights=use_weights)
        try:
            got = dv.repulse(plan, x).cpu().numpy()
            again = dv.repulse(plan, x).cpu().numpy()
        finally:
            plan.close()
        assert (got[n:] == SENTINEL).all()  # nothing written past the plan's rows
        got, again = got[:n], again[:n]
        assert np.isfinite(got).all()
        assert got.tobytes() == again.tobytes()
        worst, ok = C.ratio(got, n, Fr, T)
        print(f"{name} n={n} {variant} {dim=} {repel=} {use_weights=}: "
              f"max |F - F*| / bound = {worst:.4f}")
        if n == 1:
            assert not got.any()  # the only rows with sum |t| = 0
        assert ok, (name, worst)


# --------------------------------------------------------------------------
# 2. cut independence, bit for bit

def _shards(n):
    """Row shards that cut inside the first row block, across the block edge and (at
    n = 4 097) leave a last shard of several blocks, and an empty one.  1 026 is clipped
    to n: at n = 1 025 the middle shard is exactly one row block and the last is empty."""
    cut = min(1026, n)
    return [(0, 1), (1, cut), (cut, n), (5, 5)]


@pytest.mark.parametrize("d", [3, 1])
@pytest.mark.parametrize("n", [4097, 1025])
def test_row_shards_equal_the_whole_plan(ctx, n, d):
    """A row's chunking depends on n alone, so every row shard computes the whole plan's
    bits (what GE_MODE_FARFIELD's row-shard fall-back relies on)."""
    dv = _dev(ctx, n)
    X = C.coords(n, d, "degenerate")
    x = dv.up(X)
    want = _fast_whole(ctx, n, d, X, repel=3.5)
    out = dv.torch.full((n + GUARD, d), SENTINEL, dtype=dv.torch.float64, device=dv.dev)
    done = np.zeros(n, bool)
    for rb, re in _shards(n):
        assert route.repulse_kernel(n, d, rb=rb, re=re, mode=ge.MODE_FAST,
                                    repel=3.5) == "fa_repulse_fast"
        p = dv.plan(d, rb, re, mode=ge.MODE_FAST, repel=3.5)
        try:
            dv.repulse(p, x, rb, re, out=out)
        finally:
            p.close()
        done[rb:re] = True
        got = out.cpu().numpy()
        # rows outside the shards run so far keep the sentinel (an empty shard: all of them)
        assert (got[n:] == SENTINEL).all() and (got[:n][~done] == SENTINEL).all(), (rb, re)
        assert got[:n][done].tobytes() == want[done].tobytes(), (rb, re)
    assert done.all()


# --------------------------------------------------------------------------
# 3. a FAST step is FAST repulsion plus the STRICT row pass

@pytest.mark.parametrize("n,d", [(1025, 2), (4097, 4)])
def test_step_is_fast_repulsion_plus_strict_rows(ctx, monkeypatch, n, d):
    dv = _dev(ctx, n)
    t = dv.torch
    x = dv.up(C.coords(n, d))
    y, y2, f = t.full_like(x, SENTINEL), t.full_like(x, SENTINEL), t.full_like(x, SENTINEL)
    kw = dict(repel=3.5, use_weights=1)
    assert route.step_kernel(n, d, mode=ge.MODE_FAST, **kw) == "fa_repulse_fast+rows"
    stepper = dv.plan(d, mode=ge.MODE_FAST, **kw)
    repulser = dv.plan(d, mode=ge.MODE_FAST, **kw)
    monkeypatch.setenv("GE_FA_SYM", "0")  # no sweep tables on the STRICT plan
    rows = dv.plan(d, mode=ge.MODE_STRICT, **kw)
    try:
        stepper.step(x.data_ptr(), y.data_ptr())
        repulser.repulse(x.data_ptr(), f.data_ptr())
        rows.attract(x.data_ptr(), f.data_ptr(), y2.data_ptr())
        ctx.sync()
    finally:
        for p in (stepper, repulser, rows):
            p.close()
    a, b = y.cpu().numpy(), y2.cpu().numpy()
    assert np.isfinite(a).all() and not (a == SENTINEL).all(axis=1).any()
    assert a.tobytes() == b.tobytes()
    assert not np.array_equal(a, x.cpu().numpy())


# --------------------------------------------------------------------------
# 4. ge_force_atlas under FAST equals a hand-stepped plan, graph replay included

def _hand_stepped(ctx, n, d, X, iterations):
    dv = _dev(ctx, n)
    x = dv.up(X)
    y = dv.torch.empty_like(x)
    p = dv.plan(d, mode=ge.MODE_FAST)
    try:
        for _ in range(iterations):
            p.step(x.data_ptr(), y.data_ptr())
            x, y = y, x
        ctx.sync()
    finally:
        p.close()
    return x.cpu().numpy()


def test_force_atlas_equals_hand_stepped_plan(ctx, monkeypatch):
    """2 iterations; 130 = four replays of the captured 32-step graph plus 2 plain steps
    (even / odd buffer swap), and the same bytes with GE_NO_GRAPH=1; n = 5 runs the plan
    path (FAST skips the one-workgroup kernel)."""
    n, d = 257, 3
    A, X = C.case(n)[0], C.coords(n, d)
    for iterations in (2, 130):
        want = _hand_stepped(ctx, n, d, X, iterations)
        assert np.isfinite(want).all()
        assert route.run_kernel(A, d, iterations, mode=ge.MODE_FAST) == "fa_repulse_fast+rows"
        assert route.schedule(n, d, iterations=iterations, mode=ge.MODE_FAST)["graph"] == (iterations == 130)
        got = ctx.force_atlas(A, d, coords=X, iterations=iterations, mode=ge.MODE_FAST)
        assert got.tobytes() == want.tobytes(), iterations
    monkeypatch.setenv("GE_NO_GRAPH", "1")
    assert not route.schedule(n, d, iterations=130, mode=ge.MODE_FAST)["graph"]
    got = ctx.force_atlas(A, d, coords=X, iterations=130, mode=ge.MODE_FAST)
    assert got.tobytes() == want.tobytes()
    monkeypatch.delenv("GE_NO_GRAPH")
    n, d = 5, 2
    A, X = C.case(n)[0], C.coords(n, d)
    assert route.run_kernel(A, d, 3, mode=ge.MODE_FAST) == "fa_repulse_fast+rows"
    got = ctx.force_atlas(A, d, coords=X, iterations=3, mode=ge.MODE_FAST)
    assert got.tobytes() == _hand_stepped(ctx, n, d, X, 3).tobytes()
    strict = ctx.force_atlas(A, d, coords=X, iterations=3)
    assert np.allclose(got, strict, rtol=1e-9, atol=1e-12)


# --------------------------------------------------------------------------
# 5. NaN

@pytest.mark.parametrize("d", [1, 3])
def test_nan_coordinate(ctx, d):
    """One NaN coordinate: NaN where the long-double reference has NaN (every component of
    every row: each row meets the vertex, and a NaN distance makes the whole term NaN, as
    in include/forceatlas.hpp), and nowhere else."""
    n, v = 257, 100
    X = C.coords(n, d)
    X[v, d // 2] = np.nan
    with np.errstate(invalid="ignore"):
        Fr, _ = C.FAR.exact_rows(X, C.masses(n, 1), 1.0, np.arange(n))
    assert np.isnan(Fr).all()
    got = _fast_whole(ctx, n, d, X)
    assert np.array_equal(np.isnan(got), np.isnan(Fr))
    assert not np.isinf(got).any()


# --------------------------------------------------------------------------
# 6. the 1e-5 bar at every dimension

@pytest.mark.parametrize("d", [1, 2, 4])
def test_fast_mode_tolerance(ctx, d):
    """tests/test_gpu_parity.py's test_fa_fast_mode_tolerance (d = 3) at the other
    dimensions: the coordinates after 2 iterations against STRICT."""
    n = 1025
    A, X = C.case(n)[0], C.coords(n, d)
    strict = ctx.force_atlas(A, d, coords=X, iterations=2)
    fast = ctx.force_atlas(A, d, coords=X, iterations=2, mode=ge.MODE_FAST)
    rel = float(np.max(np.abs(fast - strict)) / np.max(np.abs(strict)))
    print(f"FAST against STRICT after 2 iterations, {d=}: {rel:.3e}")
    assert np.isfinite(fast).all()
    assert rel < REL_TOL_FAST
