"""The sweeps' issue-priority hints (ge_sym.hpp sweep_prio): the bits stay the oracle's
at every tile count at which a hint's index is clamped, and the hints do fire.

A sweep steers its own issue priority from two hints read off the hand-over
counters: `spun` (its wait found the flag unset) and `lead` (the predecessor has
handed over the tile K_LOOK tiles ahead: an index clamped to the aggregate's last
counter).  Neither may change a bit, and the look-ahead may not leave the aggregate's
counters, so the layouts put the tile counts around K_LOOK next to each other and the
shortest aggregate at the very end of the allocation.  (The variant that also kept a
`want` word per counter for a waiting follower was measured and not shipped, so there
are no such words to test.)  Every run returning at all shows the plan's error word clear
(a hand-over wait that times out fails the call with GE_ERR_STATE).
"""
import numpy as np
import pytest

import graphs as G
import ref_cases as C
from faml_plan import assert_census, assert_schedule, run_plan

pytestmark = pytest.mark.gpu

K_LOOK = 16  # ge_sym.hpp kLook
K_STAMP_WORDS = 8  # ge_sym.hpp kStampWords
SWEEPS = {"GE_FAML_RES_CAP": "256", "GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"}

# All streamed under GE_FAML_RES_CAP=256 (more than 256 members); 257 has the fewest
# tiles (5, with 320) and is last in the progress counters.
EDGE_SIZES = [2600, 321, 64 * K_LOOK, 64 * K_LOOK + 1, 64 * (K_LOOK + 1) + 1, 320, 257]
ALONE_SIZES = [257]

_cases = {}
_wants = {}


def _case(sizes, dim, repel=1.0):
    key = (tuple(sizes), dim, repel)
    if key not in _cases:
        n = sum(sizes)
        A = C.symmetric_weights(G.rmat(n, 8 * n, seed=len(sizes) + dim))
        _cases[key] = C._ml(A, sizes, 13, dim, 6, 29, repel=repel)
    return key, _cases[key]


def _want(oracle, key, case):
    if key not in _wants:
        x = C.run_ml(oracle.force_atlas_ml, case)
        x.setflags(write=False)
        _wants[key] = x
    return _wants[key]


def _run(ctx, monkeypatch, sizes, case):
    for k, v in SWEEPS.items():
        monkeypatch.setenv(k, v)
    got, cls, sched = run_plan(ctx, case)
    want = assert_census(cls, sizes, case["dim"], "256")
    assert want["streamed"] == [s for s in sizes if s > 256]
    assert_schedule(sched, cls, want["streamed"], "sweeps")
    return got


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_look_ahead_tile_edges(ctx, oracle, monkeypatch, dim):
    """5, 6, K_LOOK, K_LOOK + 1, K_LOOK + 2 and 41 tiles in one launch, the shortest last."""
    key, case = _case(EDGE_SIZES, dim)
    assert np.array_equal(_run(ctx, monkeypatch, EDGE_SIZES, case), _want(oracle, key, case))


def test_look_ahead_tile_edges_division_path(ctx, oracle, monkeypatch):
    """repel = 2^70 is outside weight_ok: every tile takes the `/` forms (col_steps)."""
    key, case = _case(EDGE_SIZES, 3, repel=2.0 ** 70)
    assert np.array_equal(_run(ctx, monkeypatch, EDGE_SIZES, case), _want(oracle, key, case))


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_single_short_aggregate_at_allocation_end(ctx, oracle, monkeypatch, dim):
    """One streamed aggregate of 5 tiles alone: every look-ahead index is clamped to the
    allocation's last word."""
    key, case = _case(ALONE_SIZES, dim)
    assert np.array_equal(_run(ctx, monkeypatch, ALONE_SIZES, case), _want(oracle, key, case))


@pytest.mark.parametrize("k", [2, K_LOOK + 2])
@pytest.mark.parametrize("dim", [2, 3])
def test_single_level_below_and_above_look_ahead(ctx, oracle, monkeypatch, k, dim):
    """forceAtlas through the symmetric kernel as one aggregate of k + 1 row tiles
    (n = 64 k + 1): fewer tiles than the look-ahead and more."""
    monkeypatch.setenv("GE_STREAM_MAX", "0")
    monkeypatch.setenv("GE_FA_SYM", "1")
    n = 64 * k + 1
    A = G.rmat(n, 6 * n, seed=n + dim)
    m = len(A[0]) - 1
    assert m == n
    X0 = G.random_coords(m, dim, seed=dim)
    want = oracle.force_atlas(A, dim, coords=X0, iterations=3)
    assert np.array_equal(ctx.force_atlas(A, dim, coords=X0, iterations=3), want)


def _read_stamps(path):
    raw = open(path, "rb").read()
    nunits, words, blocks, threads = (int(v) for v in np.frombuffer(raw[:16], dtype=np.int32))
    assert words == K_STAMP_WORDS and len(raw) == 16 + 16 * nunits + 8 * words * nunits
    units = np.frombuffer(raw[16:16 + 16 * nunits], dtype=np.int32).reshape(nunits, 4)
    st = np.frombuffer(raw[16 + 16 * nunits:], dtype=np.int64).reshape(nunits, words)
    return units, st


def test_hints_fire(ctx, oracle, monkeypatch, tmp_path):
    """The stamping instantiation on the edge layout: same bits, and the launch's
    timeline counts at least one wait that spun and one tile run at raised priority.
    All the sweeps are resident at once (fewer than the grid's waves), so every sweep
    A > 0 finds its first tile's flag unset (spun), and sweep 0 of every aggregate
    never waits (raised)."""
    dump = tmp_path / "stamps.bin"
    monkeypatch.setenv("GE_SYM_STAMPS", str(dump))
    key, case = _case(EDGE_SIZES, 3)
    assert np.array_equal(_run(ctx, monkeypatch, EDGE_SIZES, case), _want(oracle, key, case))
    units, st = _read_stamps(dump)
    tiles = sum((s + 63) // 64 for s in EDGE_SIZES if s > 256)
    assert len(units) == tiles
    assert (st[:, 2] >= st[:, 0]).all()
    raised, spun = st[:, 6], st[:, 7]
    print("raised tiles", int(raised.sum()), "spun waits", int(spun.sum()), "units", tiles)
    assert (spun >= 0).all() and (raised >= 0).all()
    assert spun.max() >= 1
    assert raised.max() >= 1
    # a sweep runs at most its own column tiles raised and waits once per tile
    rem = np.array([((np.diff(case["PT"][0])[a] + 63) // 64) - A for a, A in units[:, :2]])
    assert (raised <= rem).all() and (spun <= rem).all()
    assert (spun[units[:, 1] == 0] == 0).all()
