"""ge_force_atlas_batch and ge_embed_via_force_atlas_ml on the device.

The contract (include/ge.h): every graph of a batch has the bits of ge_force_atlas on it
alone.  Expected values come from the oracle and from ctx.force_atlas per graph, never
from the batch; each test asserts its class counts, so none passes by running serial.
The oracle is bit-exact for the default attraction only: linlog / delta != 1 go through
the device's log / pow (include/ge.h), so those two options are compared with
ctx.force_atlas alone.  300 iterations unless said.
"""
import functools

import numpy as np
import pytest

import fa_batch_cases as C
import ge_amd as ge
import oracle_lib as O

pytestmark = pytest.mark.gpu

IT = C.ITERATIONS


def _key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _oracle(dim, key=()):
    kw = dict(key)
    kw.pop("mode", None)
    O.build()
    gs = C.cases()
    return [O.force_atlas(A, dim, coords=X0, iterations=IT, **kw)
            for A, X0 in zip(gs, C.start(gs, dim))]


def _alone(ctx, graphs, dim, coords, iterations=IT, **kw):
    return [ctx.force_atlas(A, dim, coords=X0, iterations=iterations, **kw)
            for A, X0 in zip(graphs, coords)]


def _assert_each(got, want, what, nan_where=None):
    """Bit-equal per graph; NaNs only where nan_where (default: want) has them."""
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        ref = b if nan_where is None else nan_where[g]
        nan_ok = bool(np.isnan(ref).any())
        assert C.same(a, b, nan_ok=nan_ok), f"{what}: graph {g} (n = {len(b)}) differs"


def _totals(graphs, dim, **kw):
    s = ge.fa_batch_schedule(*C.sizes_entries(graphs), dim, **kw)
    return {k: s[k] for k in ge.FA_BATCH_TOTALS}


@pytest.mark.parametrize("dim", [1, 2, 3, 4, 5, 8, 16])
def test_all_sizes_in_one_batch(ctx, dim):
    gs = C.cases()
    X0 = C.start(gs, dim)
    got, info = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=IT, info=True)
    assert info == _totals(gs, dim)
    assert info["waves"] > 0 and info["blocks"] > 0 and info["serials"] > 0
    want = _oracle(dim)
    _assert_each(got, want, f"d = {dim} against the oracle")
    _assert_each(got, _alone(ctx, gs, dim, X0), f"d = {dim} against ge_force_atlas alone",
                 nan_where=want)


EXACT_OPTIONS = {"unweighted": dict(use_weights=0), "nohubs": dict(nohubs=1),
                 "repel2": dict(repel=2.0), "normalize": dict(normalize=1)}
LOG_POW_OPTIONS = {"linlog": dict(linlog=1), "delta0.5": dict(delta=0.5)}


@pytest.mark.parametrize("name", list(EXACT_OPTIONS) + list(LOG_POW_OPTIONS))
def test_options(ctx, name):
    kw = {**EXACT_OPTIONS, **LOG_POW_OPTIONS}[name]
    gs, dim = C.cases(), 3
    X0 = C.start(gs, dim)
    got, info = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=IT, info=True, **kw)
    assert info == _totals(gs, dim, **kw) and info["waves"] == 15 and info["blocks"] == 5
    alone = _alone(ctx, gs, dim, X0, **kw)
    if name in EXACT_OPTIONS:
        want = _oracle(dim, _key(kw))
        _assert_each(got, want, f"{name} against the oracle")
        _assert_each(got, alone, f"{name} against ge_force_atlas alone", nan_where=want)
    else:
        assert all(np.isfinite(x).all() for x in alone)
        _assert_each(got, alone, f"{name} against ge_force_atlas alone")


@pytest.mark.parametrize("seeds", [None, "distinct"])
def test_init_random(ctx, seeds):
    gs, dim = C.cases(), 3
    sd = None if seeds is None else [1000 + 7 * g for g in range(len(gs))]
    got, info = ctx.force_atlas_batch(gs, dim, iterations=IT, seeds=sd, info=True, seed=77)
    assert info["waves"] == 15 and info["blocks"] == 5 and info["serials"] == 1
    per = [77] * len(gs) if sd is None else sd
    want = [O.force_atlas(A, dim, iterations=IT, seed=s) for A, s in zip(gs, per)]
    _assert_each(got, want, "random start against the oracle")
    alone = [ctx.force_atlas(A, dim, iterations=IT, seed=s) for A, s in zip(gs, per)]
    _assert_each(got, alone, "random start against ge_force_atlas alone", nan_where=want)
    if sd is None:  # every graph drew from the start of the one stream
        assert np.array_equal(O.uniform_stream(77, 8 * dim).reshape(8, dim),
                              ctx.force_atlas_batch(gs[6:7], dim, iterations=0, seed=77)[0])


BAD = {"1e200": 1e200, "subnormal": 5e-324, "inf": np.inf, "nan": np.nan}


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("cls", ["wave", "block"])
def test_isolation(ctx, cls, bad):
    """One graph starts outside the exact-division domain; every graph, that one
    included, still equals its separate call."""
    pick = (5, 8, 17, 33, 64) if cls == "wave" else (65, 127, 256)
    gs = [A for A in C.cases() if len(A[0]) - 1 in pick]
    dim, victim = 3, 2 if cls == "wave" else 1
    X0 = C.start(gs, dim, seed=9)
    X0[victim][1, 0] = BAD[bad]
    got, info = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=IT, info=True)
    assert info["waves" if cls == "wave" else "blocks"] == len(gs) and info["serials"] == 0
    want = _alone(ctx, gs, dim, X0)
    for g in range(len(gs)):
        assert g == victim or np.isfinite(want[g]).all()
    _assert_each(got, want, f"{cls} class, {bad}")
    # the oracle on the same start (bit for bit where it stays finite)
    worc = [O.force_atlas(A, dim, coords=X, iterations=IT) for A, X in zip(gs, X0)]
    _assert_each(got, worc, f"{cls} class, {bad}, against the oracle")


def test_reversed_and_cut_in_two(ctx):
    gs, dim = list(C.cases()), 3
    X0 = C.start(gs, dim)
    whole = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=IT)
    _assert_each(whole, _oracle(dim), "the whole batch")
    rev, info = ctx.force_atlas_batch(gs[::-1], dim, coords=X0[::-1], iterations=IT, info=True)
    assert (info["waves"], info["blocks"], info["serials"]) == (15, 5, 1)
    _assert_each(rev[::-1], _oracle(dim), "the batch reversed")
    cut = 10
    a, ia = ctx.force_atlas_batch(gs[:cut], dim, coords=X0[:cut], iterations=IT, info=True)
    b, ib = ctx.force_atlas_batch(gs[cut:], dim, coords=X0[cut:], iterations=IT, info=True)
    assert ia["waves"] == 10 and ib["waves"] == 5 and ib["blocks"] == 5
    _assert_each(a + b, _oracle(dim), "the batch cut in two")


def test_many_copies(ctx):
    """More waves than a workgroup holds, more workgroups than the device has CUs in both
    launches: all copies are equal, and equal to the graph alone."""
    by_n = {len(A[0]) - 1: A for A in C.cases()}
    small, mid, dim = by_n[9], by_n[65], 3
    Xs, Xm = C.start([small, mid], dim, seed=13)
    gs = [small] * 1100 + [mid] * 300
    got, info = ctx.force_atlas_batch(gs, dim, coords=[Xs] * 1100 + [Xm] * 300, iterations=IT,
                                      info=True)
    assert info == dict(waves=1100, blocks=300, serials=0, wave_workgroups=275)
    ws = O.force_atlas(small, dim, coords=Xs, iterations=IT)
    wm = O.force_atlas(mid, dim, coords=Xm, iterations=IT)
    assert all(C.same(x, ws) for x in got[:1100]) and all(C.same(x, wm) for x in got[1100:])
    assert C.same(ctx.force_atlas(small, dim, coords=Xs, iterations=IT), ws)


def test_horizon(ctx):
    """Six graphs of 5..64 vertices over the reference's 100 000 iterations."""
    pick = (5, 9, 17, 33, 63, 64)
    gs = [A for A in C.cases() if len(A[0]) - 1 in pick]
    dim = 3
    X0 = C.start(gs, dim, seed=17)
    got, info = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=100000, info=True)
    assert info["waves"] == 6 and info["blocks"] == 0 and info["serials"] == 0
    want = _alone(ctx, gs, dim, X0, iterations=100000)
    assert all(np.isfinite(x).all() for x in want)
    _assert_each(got, want, "100 000 iterations")


def test_fast_mode_is_serial_below_the_wide_schedule(ctx):
    gs, dim = C.cases(), 3
    X0 = C.start(gs, dim)
    got, info = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=IT, info=True,
                                      mode=ge.MODE_FAST)
    assert info == dict(waves=0, blocks=0, serials=len(gs), wave_workgroups=0)
    want = _alone(ctx, gs, dim, X0, mode=ge.MODE_FAST)
    assert all(np.isfinite(x).all() for x in want)
    _assert_each(got, want, "FAST, d = 3")


def test_fast_mode_on_the_wide_schedule(ctx):
    gs, dim = C.cases(), 8
    X0 = C.start(gs, dim)
    got, info = ctx.force_atlas_batch(gs, dim, coords=X0, iterations=IT, info=True,
                                      mode=ge.MODE_FAST)
    assert info == _totals(gs, dim) and info["waves"] == 15 and info["blocks"] == 3
    _assert_each(got, _oracle(dim), "FAST, d = 8, against the oracle")
    _assert_each(got, _alone(ctx, gs, dim, X0, mode=ge.MODE_FAST), "FAST, d = 8")


@pytest.mark.parametrize("dim", [2, 3, 8])
def test_multilevel_form(ctx, dim):
    lv = C.ml_level()
    sizes = np.diff(lv["PT"][0])
    assert sizes.min() == 1 and sizes.max() == 70 and len(C.sub_matrix(
        lv["A"], lv["PT"], lv["vA"], lv["bare"])[1]) == 0
    got, info = ctx.embed_via_force_atlas_ml(lv["A"], lv["PT"], lv["vA"], lv["cA"][dim], lv["rA"],
                                             dim, iterations=200, seed=7, info=True)
    assert info["waves"] == int((sizes <= 64).sum()) and info["blocks"] == 2
    assert info["serials"] == 0
    orc = C.ml_compose(lv["A"], lv["PT"], lv["vA"], lv["cA"][dim], lv["rA"], dim,
                       lambda S, d: O.force_atlas(S, d, iterations=200, seed=7))
    assert np.isfinite(orc).all()  # the single member too: its layout is one point off 0
    assert C.same(got, orc)
    own = C.ml_compose(lv["A"], lv["PT"], lv["vA"], lv["cA"][dim], lv["rA"], dim,
                       lambda S, d: ctx.force_atlas(S, d, iterations=200, seed=7))
    assert C.same(got, own)


def test_errors_with_a_context(ctx):
    off = np.array([0, 2, 4], dtype=np.int32)
    ip = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    ix = np.array([1, 0, 3, 2], dtype=np.int32)
    dx = np.ones(4)

    def run(off=off, ix=ix, dim=3):
        X = np.random.RandomState(1).uniform(-1.0, 1.0, size=(4, max(dim, 1)))
        return ge._force_atlas_batch_raw(ctx, off, ip, ix, dx, dim, X, False, None, 1, {})

    assert run().shape == (4, 3)
    with pytest.raises(ge.GeError, match=r"graph 1: .*outside"):
        run(ix=np.array([1, 0, 1, 2], dtype=np.int32))
    with pytest.raises(ge.GeError, match=r"graph 1: .*offsets"):
        run(off=np.array([0, 3, 2, 4], dtype=np.int32))
    for dim in (0, 17):
        with pytest.raises(ge.GeError, match="1..16"):
            run(dim=dim)
    # the context still works
    assert np.isfinite(run()).all()
