"""The sweeps' record ring at the edges of its schedule (ge_sym.hpp: the 16-byte halves,
the mirror, tile_steps' read one step ahead, the drain's zeroing): one
forceAtlasMultilevel call over tests/sym_ring_cases.py, every aggregate streamed as
symmetric sweeps, bit for bit against the oracle.
"""
import numpy as np
import pytest

import sym_ring_cases as R
from faml_plan import assert_census, assert_schedule, run_plan

pytestmark = pytest.mark.gpu

SWEEPS = {"GE_FAML_RES_CAP": "256", "GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"}


def _check(ctx, oracle, monkeypatch, case, init):
    for k, v in SWEEPS.items():
        monkeypatch.setenv(k, v)
    got, cls, sched = run_plan(ctx, case, init=init)
    want = assert_census(cls, R.SIZES, case["dim"], "256")
    assert want["streamed"] == R.SIZES
    assert_schedule(sched, cls, want["streamed"], "sweeps")
    ref = oracle.force_atlas_ml(case["A"], case["PT"], case["vA"], case["cA"], case["rA"],
                                case["dim"], iterations=case["iterations"], seed=case["seed"],
                                init=init, **case["kw"])
    assert np.isfinite(ref).all()
    bad = np.flatnonzero((got.view(np.uint64) != ref.view(np.uint64)).any(axis=1))
    # rows are in vertex order: name the aggregates of the rows that differ
    assert len(bad) == 0, (f"{len(bad)} rows differ, in aggregates of sizes "
                           f"{sorted({R.SIZES[a] for a in case['vA'][bad]})}")
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("iterations", R.ITERATIONS)
@pytest.mark.parametrize("repel", R.REPELS, ids=["repel-one", "general", "slash-forms"])
@pytest.mark.parametrize("dim", R.DIMS)
def test_ring_edges(ctx, oracle, monkeypatch, dim, repel, iterations):
    case, init = R.case(dim, repel, iterations)
    _check(ctx, oracle, monkeypatch, case, init)


@pytest.mark.parametrize("dim", R.DIMS)
def test_member_at_the_origin_in_the_last_tile(ctx, oracle, monkeypatch, dim):
    """The last member of every aggregate has the coordinates of a short last tile's padding
    (the origin) and the deg+1 the plan builds for it: its record must not be taken for,
    or overwritten by, the inert ones staged beside it."""
    case, init = R.case(dim, 1.0, 1, origin_last=True)
    _check(ctx, oracle, monkeypatch, case, init)
