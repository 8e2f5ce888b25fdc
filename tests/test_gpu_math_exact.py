"""The strict kernels' hand-built arithmetic against exact math on hard-to-round
operands (tests/math_cases.py; tests/test_math_cases.py checks the cases and the
reference on the CPU).

Helper level: ge_math_cases runs sqrt_normal, recip_of + div_by, pair_den +
div_by_nz and rep_term on every case, one thread each, and returns the bits; they
must equal the correctly rounded reference.  The compiler's own `/` and sqrt come
back beside them, so a failure says which layer missed.  The one allowance is the
documented one: a +-0 term of div_by_nz may differ in sign (ge_math.hpp).

Kernel level: layouts that hold the hard pairs (two points whose distance is a
hard denominator exactly, each at norm T/2) run through every repulsion schedule
of forceAtlas and forceAtlasMultilevel, one and three iterations, against the
oracle bit for bit.  A one-ulp error of one term is usually absorbed by its row's
sum, so one all-ones pair per binade is joined by a heavy edge
(math_cases.HEAVY_PAIRS): its mutual term dominates the row and a wrong last bit
reaches the coordinates.

Measured on an MI355X before pair_den corrected its reciprocal for all-ones
distances: SQRT 0 of 1 612, DIV 0 of 599 375, PAIR dis 0, n/dis 1 098 and c/dis^2 0
of 144 447 (the nine all-ones distances times the 122 power-of-two numerators), REP
36 of 576 first components at d = 2, 3, 4 and 0 of 296 at d = 1; the compiler's `/`
and sqrt differed nowhere.  With the correction every count is 0.
"""
import functools

import numpy as np
import pytest

import graphs as G
import math_cases as M
import ref_cases as C
from faml_plan import assert_census, assert_schedule, run_plan

pytestmark = pytest.mark.gpu

SHOWN = 8  # failing cases listed in an assertion message


def _differs(got_bits, want, zero_sign_free=False):
    """Per element: the device's bits differ from the reference's."""
    bad = np.asarray(got_bits, np.uint64) != M.bits(want).reshape(np.shape(got_bits))
    if zero_sign_free:
        got = np.asarray(got_bits, np.uint64).view(np.float64)
        bad &= ~((got == 0.0) & (np.asarray(want) == 0.0))
    return bad


def _hex(v):
    return np.asarray(v, np.uint64).reshape(1).view(np.float64)[0].hex()


class Checks:
    """Collects the comparisons of one test, so that a failure reports every one of them."""

    def __init__(self):
        self.failed = []

    def add(self, name, operands, labels, helper, want, compiler, zero_sign_free=False):
        """helper / compiler: the bits of the project's helper and of the compiler's own
        operation, case by case; want: the exact result.  Prints the counts and keeps, for
        a failure, the first failing operands in hex with what the compiler's form did."""
        bad_h = _differs(helper, want, zero_sign_free)
        bad_c = _differs(compiler, want)
        print(f"{name}: {len(want)} cases, helper differs at {int(bad_h.sum())}, "
              f"the compiler's own operation at {int(bad_c.sum())}")
        if not (bad_h.any() or bad_c.any()):
            return
        lines = [f"{name}: {int(bad_h.sum())} of {len(want)} helper results and "
                 f"{int(bad_c.sum())} of the compiler's own differ from the exact value; first:"]
        for i in np.flatnonzero(bad_h | bad_c)[:SHOWN]:
            ops = ", ".join(f"{l} = {float(v).hex()}"
                            for l, v in zip(labels, np.atleast_1d(operands[i])))
            lines.append(f"  {ops}: exact {float(want[i]).hex()}, helper {_hex(helper[i])}"
                         f"{' WRONG' if bad_h[i] else ''}, compiler {_hex(compiler[i])}"
                         f"{' WRONG' if bad_c[i] else ''}")
        self.failed.append("\n".join(lines))

    def done(self):
        assert not self.failed, "\n".join(self.failed)


# --------------------------------------------------------------------------
# helper level

def test_sqrt_normal_is_correctly_rounded(ctx):
    out = ctx.math_cases("sqrt", M.SQRT_S)
    assert out.shape == (M.N_SQRT, 2)
    ck = Checks()
    ck.add("SQRT", M.SQRT_S, ["s"], out[:, 0], M.sqrt_reference(), out[:, 1])
    ck.done()


def test_shared_reciprocal_quotient_is_correctly_rounded(ctx):
    out = ctx.math_cases("div", np.stack([M.DIV_N, M.DIV_D], axis=1))
    assert out.shape == (M.N_DIV, 2)
    ck = Checks()
    ck.add("DIV", np.stack([M.DIV_N, M.DIV_D], axis=1), ["n", "d"], out[:, 0], M.div_reference(),
           out[:, 1])
    ck.done()


def test_pair_den_is_correctly_rounded(ctx):
    rows = np.stack([M.PAIR_S, M.PAIR_N, M.PAIR_C], axis=1)
    out = ctx.math_cases("pair", rows)
    assert out.shape == (M.N_PAIR, 5)
    want = M.pair_reference()
    dis = out[:, 0].view(np.float64)
    ck = Checks()
    ck.add("PAIR dis", rows, ["s", "n", "c"], out[:, 0], want[:, 0], out[:, 0])
    ops = np.stack([M.PAIR_S, M.PAIR_N, M.PAIR_C, dis], axis=1)
    ck.add("PAIR n/dis", ops, ["s", "n", "c", "dis"], out[:, 1], want[:, 1], out[:, 3],
           zero_sign_free=True)
    ck.add("PAIR c/dis^2", ops, ["s", "n", "c", "dis"], out[:, 2], want[:, 2], out[:, 4])
    ck.done()


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_rep_term_is_exact(ctx, dim):
    rows = M.rep_cases(dim)
    out = ctx.math_cases("rep", rows, dim=dim)
    assert out.shape == (M.N_REP[dim], 2 * dim)
    want = M.rep_reference(rows, dim)
    labels = ([f"xi{k}" for k in range(dim)] + [f"xj{k}" for k in range(dim)]
              + ["deg_i+1", "deg_j+1", "repel"])
    ck = Checks()
    for k in range(dim):
        ck.add(f"REP d={dim} term {k}", rows, labels, out[:, k], want[:, k], out[:, dim + k],
               zero_sign_free=True)
    ck.done()


# --------------------------------------------------------------------------
# kernel level, single-level forceAtlas

SYM = {"GE_STREAM_MAX": "0", "GE_FA_SYM": "1"}
FA_PATHS = {
    # name: (n, dim, environment)
    "one-workgroup-d2": (400, 2, {"GE_SMALL_MAX": "512"}),
    "one-workgroup-d3": (400, 3, {"GE_SMALL_MAX": "512"}),
    "grouped-d2": (600, 2, {"GE_SMALL_MAX": "0"}),
    "grouped-d3": (600, 3, {"GE_SMALL_MAX": "0"}),
    "grouped-d4": (600, 4, {"GE_SMALL_MAX": "0"}),
    "grouped-tiles-d3": (3300, 3, {"GE_SMALL_MAX": "0"}),  # above grouped_cap(3): fa_grouped_stream
    "ordered-pairs-d2": (1100, 2, {"GE_STREAM_MAX": "0", "GE_FA_SYM": "0"}),
    "ordered-pairs-d3": (1100, 3, {"GE_STREAM_MAX": "0", "GE_FA_SYM": "0"}),
    "sweeps-d2": (1100, 2, SYM),
    "sweeps-d3": (1100, 3, SYM),
    "sweeps-d4": (1100, 4, SYM),
    "wide-d5": (600, 5, {}),
}


@functools.lru_cache(maxsize=None)
def _fa_want(n, dim, iterations):
    import oracle_lib
    oracle_lib.build()
    A, X0 = M.crafted_fa_case(n, dim)
    x = oracle_lib.force_atlas(A, dim, coords=X0, iterations=iterations)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("path", list(FA_PATHS))
def test_fa_paths_on_hard_pairs(ctx, monkeypatch, path):
    """forceAtlas from a layout whose first 180 points are the hard pairs: the first
    iteration divides by the hard distances in the repulsion, along the joined pairs in
    the attraction, and by the hard norms T/2 in the gravity term.  The environment is
    what selects each schedule (GE_FA_SYM=1 needs GE_STREAM_MAX=0 below 65 536 rows)."""
    n, dim, env = FA_PATHS[path]
    for k in ("GE_SMALL_MAX", "GE_STREAM_MAX", "GE_FA_SYM", "GE_WIDE_MIN_DIM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A, X0 = M.crafted_fa_case(n, dim)
    for it in (1, 3):
        got = ctx.force_atlas(A, dim, coords=X0, iterations=it)
        want = _fa_want(n, dim, it)
        bad = np.flatnonzero((M.bits(got) != M.bits(want)).reshape(n, dim).any(axis=1))
        assert len(bad) == 0, (
            f"{path}, {it} iteration(s): {len(bad)} of {n} rows differ; first rows {bad[:SHOWN]} "
            f"(rows below {2 * len(M.HARD_PAIRS)} are hard pairs): got "
            f"{[v.hex() for v in got[bad[0]]]}, want {[v.hex() for v in want[bad[0]]]}")


# --------------------------------------------------------------------------
# kernel level, forceAtlasMultilevel

ML_SIZES = [321, 257, 100, 40]
ML_PATHS = {
    # name: (GE_FAML_RES_CAP, mode of test_gpu_faml_paths.MODES)
    "resident": ("4096", None),
    "sweeps": ("256", {"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"}),
}
ML_PT_SEED = 3


@functools.lru_cache(maxsize=None)
def _ml_case(dim, repel):
    """Aggregates whose first members (in P_T storage order) are hard pairs, every third
    pair joined by an edge, math_cases.HEAVY_PAIRS by heavy ones; the start is supplied
    (init) in storage order."""
    n = sum(ML_SIZES)
    PT = C.block_partition(n, ML_SIZES, seed=ML_PT_SEED)
    init = np.random.RandomState(17).uniform(-1.0, 1.0, size=(n, dim))
    src, dst, heavy = [], [], []
    for a, s in enumerate(ML_SIZES):
        base = int(PT[0][a])
        npairs = min(len(M.HARD_PAIRS), s // 2 - 5)
        for q in range(npairs):
            init[base + 2 * q], init[base + 2 * q + 1] = M.antipodal(M.HARD_PAIRS[q], dim)
            if q % 3 == 0:
                src.append(int(PT[1][base + 2 * q]))
                dst.append(int(PT[1][base + 2 * q + 1]))
            if q in M.HEAVY_PAIRS:
                heavy.append((src[-1], dst[-1], M.HEAVY_PAIRS[q]))
    R = G.rmat(n, 6 * n, seed=9)
    rows = np.repeat(np.arange(n), np.diff(R[0]))
    A = G.csr_from_edges(n, np.concatenate([rows, np.array(src, np.int64)]),
                         np.concatenate([R[1].astype(np.int64), np.array(dst, np.int64)]))
    A = C.symmetric_weights(A)
    for a, b, w in heavy:
        A = M.with_pair_weights(A, {0: w}, src_of=lambda p: (a, b))
    assert len(heavy) == 3 + 3 + 3 + 1
    case = C._ml(A, ML_SIZES, ML_PT_SEED, dim, 3, 19, repel=repel)
    assert np.array_equal(case["PT"][1], PT[1])
    assert all(case["vA"][a] == case["vA"][b] for a, b in zip(src, dst)) and len(src) >= 60
    assert np.abs(init).max(axis=1).min() > 0.0
    init.setflags(write=False)
    return case, init


@functools.lru_cache(maxsize=None)
def _ml_want(dim, repel, iterations):
    import oracle_lib
    oracle_lib.build()
    case, init = _ml_case(dim, repel)
    x = oracle_lib.force_atlas_ml(case["A"], case["PT"], case["vA"], case["cA"], case["rA"], dim,
                                  iterations=iterations, seed=case["seed"], init=init,
                                  **case["kw"])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("repel", [1.0, 2.0 ** 70], ids=["shared", "slash-forms"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("path", list(ML_PATHS))
def test_faml_paths_on_hard_pairs(ctx, monkeypatch, path, dim, repel):
    """forceAtlasMultilevel with hard pairs among the members of every aggregate: the
    resident kernels of every class and the streamed symmetric sweeps, with the
    shared reciprocals and (repel = 2^70: c_ij leaves weight_ok) the `/` forms."""
    knob, mode = ML_PATHS[path]
    monkeypatch.setenv("GE_FAML_RES_CAP", knob)
    for k, v in (mode or {}).items():
        monkeypatch.setenv(k, v)
    case, init = _ml_case(dim, repel)
    for it in (1, 3):
        got, cls, sched = run_plan(ctx, dict(case, iterations=it), init=init)
        want_cls = assert_census(cls, ML_SIZES, dim, knob)
        if path == "resident":
            assert want_cls["large"] == [321, 257] and not want_cls["streamed"]
            assert cls["small"] == 1 and cls["mid"] == 1
        else:
            assert want_cls["streamed"] == [321, 257] and not want_cls["large"]
        assert_schedule(sched, cls, want_cls["streamed"], "sweeps" if mode else None)
        want = _ml_want(dim, repel, it)
        assert np.isfinite(want).all()
        bad = np.flatnonzero((M.bits(got) != M.bits(want)).reshape(got.shape).any(axis=1))
        assert len(bad) == 0, (
            f"{path} d={dim} repel={repel}, {it} iteration(s): {len(bad)} of {len(got)} rows "
            f"differ; first {bad[:SHOWN]}: got {[v.hex() for v in got[bad[0]]]}, "
            f"want {[v.hex() for v in want[bad[0]]]}")
