"""The multilevel plan's schedule (graph-embed_amd/csrc/ge_faml_sched.hpp) on the host:
every case of tests/golden/faml_sched.json, recorded from the plan build before the
scheduler was split out of it, comes out of ge_amd.faml_schedule scalar for scalar and
table for table (length and sha256).

The schedule changes no result bit, so no oracle comparison can see a mistake in it;
this pins it.  Each case also asserts, on the golden itself, the property it was
recorded for, so that a change of the schedule's constants has to record the golden
again deliberately (tests/golden/make_faml_sched.py).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import ge_amd as ge

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "faml_sched.json")) as _f:
    GOLDEN = {c["name"]: c for c in json.load(_f)["cases"]}
KNOBS = ("GE_FAML_RES_CAP", "GE_FAML_R", "GE_FAML_U", "GE_FAML_SYM", "GE_FAML_SYM_CHAIN")
SWEEP, ROWS = 0, 1  # ge_sym.hpp kUnitSweep, kUnitRows


def _sizes(c):
    return [s for s, k in c["sizes"] for _ in range(k)]


def _schedule(c, monkeypatch):
    for k in KNOBS + ("GE_WIDE_MIN_DIM",):
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    pip = np.concatenate([[0], np.cumsum(_sizes(c))]).astype(np.int32)
    return ge.faml_schedule(pip, c["dim"], c["cus"], c["sym_occ"], aggs=c["aggs"],
                            split=c["split"], rank=c["rank"], nranks=c["nranks"], mode=c["mode"])


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_schedule_equals_recorded(name, monkeypatch):
    c = GOLDEN[name]
    got = _schedule(c, monkeypatch)
    for k, v in c["scalars"].items():
        assert got[k] == v, (k, got[k], v)
    assert got["streamed_pairs"] == c["streamed_pairs"]
    assert sorted(c["tables"]) == sorted(ge.FAML_SCHED_TABLES)
    for k, want in c["tables"].items():
        t = np.ascontiguousarray(got[k], dtype="<i4")
        assert len(t) == want["len"], (k, len(t), want["len"])
        assert hashlib.sha256(t.tobytes()).hexdigest() == want["sha256"], k


def _units(c, monkeypatch):
    return _schedule(c, monkeypatch)["units"].reshape(-1, 4)


def _streamed(c, cap=256):
    return [s for s in _sizes(c) if s > cap]


def _tiles(sizes):
    return sum((s + 63) // 64 for s in sizes)


def test_golden_device_is_the_one_the_expectations_assume():
    """The expectations below were derived for 256 CUs and four resident sweep blocks."""
    for c in GOLDEN.values():
        assert c["cus"] == 256 and (c["sym_occ"] >= 3 or c["dim"] > 4), c["name"]


def test_case_a_mixed_with_every_class_at_this_cap():
    s = GOLDEN["a"]["scalars"]
    assert (s["sweeps"], s["row_blocks"], s["streamed"]) == (3, 4, 7)
    # a cap of 256 leaves the large-resident class (256 < s <= cap) empty: case s has it
    assert (s["small"], s["mid"], s["large"]) == (2, 2, 0)
    t = GOLDEN["s"]["scalars"]
    assert min(t["small"], t["mid"], t["large"], t["streamed"]) >= 1 and t["res_cap"] == 1100
    assert t["blocks_large"] == t["large"] == 6


def test_case_b_one_row_block_aggregate(monkeypatch):
    s = GOLDEN["b"]["scalars"]
    assert (s["row_blocks"], s["sweeps"]) == (1, 30)
    u = _units(GOLDEN["b"], monkeypatch)
    assert (u[:200, 3] == ROWS).all() and (u[:200, 0] == 0).all() and (u[200:, 3] == SWEEP).all()


def test_case_c_work_bound_all_swept():
    c = GOLDEN["c"]
    s = c["scalars"]
    assert (s["sweeps"], s["row_blocks"], s["res_cap"]) == (400, 0, 1600)
    # work / waves exceeds the longest chain: the C4 regime
    T, waves = 40, s["sym_blocks"] * 4
    assert 400 * (0.5 * T * T + T) / waves > 2.5 * T
    assert c["tables"]["units"]["len"] == 4 * 400 * T and s["ntiles"] == 400 * T


def test_case_d_row_blocks_first_in_queue(monkeypatch):
    s = GOLDEN["d"]["scalars"]
    assert (s["row_blocks"], s["sweeps"]) == (1, 600)
    u = _units(GOLDEN["d"], monkeypatch)
    assert (u[:300, 3] == ROWS).all() and (u[:300, 0] == 0).all()
    assert (u[:300, 1] == np.arange(300)).all() and (u[:300, 2] == 75).all()  # 300 / 4 levels
    assert (u[300:, 3] == SWEEP).all() and len(u) == 300 + 600 * 40


def test_case_e_all_row_blocks():
    s = GOLDEN["e"]["scalars"]
    assert (s["row_blocks"], s["sweeps"], s["ntiles"]) == (2, 0, 0)


def test_cases_f_g_h_knobs():
    tiles = _tiles(_streamed(GOLDEN["a"]))
    f, g, h = (GOLDEN[k] for k in "fgh")
    assert (f["scalars"]["sweeps"], f["scalars"]["row_blocks"]) == (7, 0)
    assert f["scalars"]["ntiles"] == tiles
    assert (g["scalars"]["sweeps"], g["scalars"]["row_blocks"], g["scalars"]["ntiles"]) == (0, 7, 0)
    assert f["tables"]["units"]["len"] == g["tables"]["units"]["len"] == 4 * tiles
    assert h["scalars"]["sym"] == 0 and h["tables"]["units"]["len"] == 0
    assert h["tables"]["items"]["len"] == 2 * tiles  # R = 1: one item per row tile


def test_cases_i_j_variants(monkeypatch):
    i, j = GOLDEN["i"]["scalars"], GOLDEN["j"]["scalars"]
    assert (i["R"], i["U"], i["code"]) == (4, 1, 33)
    assert (j["R"], j["U"], j["code"]) == (1, 1, 9)  # R = 3 is not compiled
    items = _schedule(GOLDEN["i"], monkeypatch)["items"].reshape(-1, 2)
    assert len(items) == sum((s + 255) // 256 for s in _streamed(GOLDEN["i"]))
    assert (items[:, 1] % 256 == 0).all()


def test_cases_k_l_m_wide_and_fast(monkeypatch):
    k, l, m = (GOLDEN[x] for x in "klm")
    assert k["scalars"]["wide"] == 1 and k["scalars"]["sym"] == 0
    assert (k["scalars"]["R"], k["scalars"]["U"]) == (1, 1) and k["tables"]["units"]["len"] == 0
    assert l["scalars"]["fast"] == 1 and l["scalars"]["sym"] == 0
    assert l["tables"]["units"]["len"] == 0
    fi = _schedule(l, monkeypatch)["fitems"].reshape(-1, 4)
    assert len(fi) == sum((s + 255) // 256 for s in _streamed(l))
    assert (fi[:, 1] % 256 == 0).all() and (fi[:, 2] - fi[:, 1] <= 256).all()
    assert m["scalars"]["fast"] == 0 and m["tables"]["fitems"]["len"] == 0


def test_case_n_owns_tiles_of_both_split_aggregates(monkeypatch):
    for name in ("n_strict", "n_fast"):
        c = GOLDEN[name]
        got = _schedule(c, monkeypatch)
        # rank 1 of 4: tiles [10, 20) of the 41 and [1, 3) of the 6
        assert len(got["rows"]) == 640 + 128 and len(got["xrows"]) == 2600 + 321
        assert list(got["xcounts"]) == [640 + 64, 640 + 128, 640 + 64, 680 + 65]
        assert c["scalars"]["R"] == 1 and c["scalars"]["streamed"] == 2
    assert GOLDEN["n_strict"]["tables"]["units"]["len"] == 4 * 12
    assert GOLDEN["n_fast"]["scalars"]["fast"] == 1
    assert GOLDEN["n_fast"]["tables"]["fitems"]["len"] == 4 * (3 + 1)


def test_cases_o_p_split_alone(monkeypatch):
    """257 members are 5 tiles: rank 3 of 4 owns [3, 5) and rank 0 [0, 1), so both force
    R = 1.  Three tiles (o_r4, p_r4, under GE_FAML_R=4) leave rank 0 none: R stays 4."""
    o, p = _schedule(GOLDEN["o"], monkeypatch), _schedule(GOLDEN["p"], monkeypatch)
    assert len(o["rows"]) == 1025 + 65 and len(p["rows"]) == 1025 + 64
    assert len(o["units"]) == 4 * (17 + 2) and len(p["units"]) == 4 * (17 + 1)
    o4, p4 = GOLDEN["o_r4"], GOLDEN["p_r4"]
    assert o4["scalars"]["R"] == 1 and o4["tables"]["rows"]["len"] == 1025 + 1
    assert p4["scalars"]["R"] == 4 and p4["tables"]["rows"]["len"] == 1025
    assert p4["tables"]["items"]["len"] == 2 * 5  # 1025 rows in steps of 256


def test_cases_q_r_empty_and_zero_sized():
    q, r = GOLDEN["q"], GOLDEN["r"]
    for k, t in q["tables"].items():
        assert t["len"] == (3 if k == "beg" else 1 if k == "xcounts" else 0), k
    assert q["streamed_pairs"] == 0.0
    s = r["scalars"]
    assert (s["small"], s["mid"], s["large"], s["streamed"]) == (0, 1, 0, 1)
    assert r["tables"]["order"]["len"] == 1 and r["tables"]["huge"]["len"] == 1


def test_bad_lists_are_refused():
    pip = np.array([0, 300, 600], dtype=np.int32)
    with pytest.raises(ge.GeError, match="strictly increasing"):
        ge.faml_schedule(pip, 3, 256, 4, aggs=[1, 0])
    with pytest.raises(ge.GeError, match="rank"):
        ge.faml_schedule(pip, 3, 256, 4, rank=2, nranks=2)
