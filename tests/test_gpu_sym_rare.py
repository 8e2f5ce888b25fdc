"""The sweeps' bulk loop on the rare inputs of its detect-then-fix denominators
(ge_pair.hpp pair_den_detect, ge_sym.hpp tile_steps): one forceAtlasMultilevel
iteration over tests/sym_rare_cases.py, streamed as symmetric sweeps, bit for bit
against the oracle; and the stamped instantiation's count of the steps that took the
fix-up -- above zero on the directed inputs, zero on a layout with nothing to flag.
"""
import numpy as np
import pytest

import sym_rare_cases as R
from faml_plan import assert_census, assert_schedule, run_plan

pytestmark = pytest.mark.gpu

SWEEPS = {"GE_FAML_RES_CAP": "256", "GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"}

_wants = {}


def _want(oracle, key, case, init):
    if key not in _wants:
        x = oracle.force_atlas_ml(case["A"], case["PT"], case["vA"], case["cA"], case["rA"],
                                  case["dim"], iterations=case["iterations"], seed=case["seed"],
                                  init=init, **case["kw"])
        x.setflags(write=False)
        _wants[key] = x
    return _wants[key]


def _run(ctx, monkeypatch, case, init):
    for k, v in SWEEPS.items():
        monkeypatch.setenv(k, v)
    got, cls, sched = run_plan(ctx, case, init=init)
    want = assert_census(cls, R.SIZES, case["dim"], "256")
    assert want["streamed"] == R.SIZES
    assert_schedule(sched, cls, want["streamed"], "sweeps")
    return got


def _differing(got, want, pairs):
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    return [(k, a, i, j) for k, a, i, j, ci, cj in pairs if ci in bad or cj in bad], bad


@pytest.mark.parametrize("repel", R.REPELS, ids=["shared", "slash-forms"])
@pytest.mark.parametrize("dim", R.DIMS)
def test_directed_pairs(ctx, oracle, monkeypatch, dim, repel):
    """Every rare case in tile_steps' steps at once (repel = 2^70: the `/` forms, where
    the detect-then-fix form is never entered)."""
    case, init, pairs = R.directed(dim, repel)
    got = _run(ctx, monkeypatch, case, init)
    want = _want(oracle, ("directed", dim, repel), case, init)
    assert np.isfinite(want).all()
    # rows are in vertex order: storage position c holds vertex PT[1][c]
    vs = [(k, a, i, j, case["PT"][1][ci], case["PT"][1][cj]) for k, a, i, j, ci, cj in pairs]
    hit, bad = _differing(got, want, vs)
    assert len(bad) == 0, f"d={dim} repel={repel}: {len(bad)} rows differ; directed pairs among them: {hit}"
    assert np.array_equal(got, want)


def _fixups(path):
    raw = open(path, "rb").read()
    nunits, words, _, _ = (int(v) for v in np.frombuffer(raw[:16], dtype=np.int32))
    assert len(raw) == 16 + 16 * nunits + 8 * words * nunits
    units = np.frombuffer(raw[16:16 + 16 * nunits], dtype=np.int32).reshape(nunits, 4)
    st = np.frombuffer(raw[16 + 16 * nunits:], dtype=np.int64).reshape(nunits, words)
    # ge_sym.hpp stamp_unit: the upper half of the XCC_ID word
    return units, st[:, 5] >> 32


def test_fixup_is_taken_on_directed_pairs_only(ctx, oracle, monkeypatch, tmp_path):
    """The stamped instantiation counts the steps whose wave took the fix-up: the
    directed pairs' sweeps do, and a layout with no distance near eps and no all-ones
    low word (tests/test_sym_rare_cases.py) never does."""
    monkeypatch.setenv("GE_SYM_STAMPS", str(tmp_path / "stamps.bin"))
    case, init, pairs = R.directed(3)
    got = _run(ctx, monkeypatch, case, init)
    assert np.array_equal(got, _want(oracle, ("directed", 3, 1.0), case, init))
    units, fix = _fixups(tmp_path / "stamps.bin")
    tiles = sum((s + 63) // 64 for s in R.SIZES)
    assert len(units) == tiles
    print("fix-up steps by unit (aggregate, row tile):",
          {(int(a), int(A)): int(f) for (a, A), f in zip(units[:, :2], fix) if f})
    # every sweep that holds a directed pair took it at least once, at most once per step
    for a, A in {(a, i // 64) for _, a, i, _, _, _ in pairs}:
        f = fix[(units[:, 0] == a) & (units[:, 1] == A)]
        assert len(f) == 1 and 1 <= f[0] <= 64 * ((R.SIZES[a] + 63) // 64 - A)
    pcase, pinit = R.plain(3)
    got = _run(ctx, monkeypatch, pcase, pinit)
    assert np.array_equal(got, _want(oracle, ("plain", 3), pcase, pinit))
    units, fix = _fixups(tmp_path / "stamps.bin")
    assert len(units) == tiles and (fix == 0).all(), fix
