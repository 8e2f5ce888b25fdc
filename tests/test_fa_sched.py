"""The single-level plan's schedule (graph-embed_amd/csrc/ge_fa_sched.hpp) on the host.

The schedule changes no result bit, so no oracle comparison can see a mistake in it;
this pins it.  Every expectation below was written by hand from the rules of the build
before the scheduler was split out of ge_fa.hip (plan_init, plan_step, the launch
helpers and fa_run_device there), and each case names the rule it pins.  Unless a case
says otherwise: 256 CUs, d = 3, STRICT, the whole level, no knobs.
"""
import pytest

import ge_amd as ge

KNOBS = ("GE_SMALL_MAX", "GE_SMALL_G", "GE_SMALL_HANDOVER", "GE_SMALL_GENERAL_ONLY",
         "GE_STREAM_MAX", "GE_GRP_G", "GE_GRP_SPLIT", "GE_REP_BLOCKS", "GE_REP_R", "GE_FA_SYM",
         "GE_FAR_MIN", "GE_FAR_R", "GE_NO_PERSIST", "GE_NO_GRAPH", "GE_FA_PACKED",
         "GE_FA_PACK_ROWS", "GE_PERSIST_REQUIRE", "GE_WIDE_MIN_DIM")
STREAM_MAX = 65536  # kStreamMax
FAST, FARFIELD = ge.MODE_FAST, ge.MODE_FARFIELD


@pytest.fixture
def sched(monkeypatch):
    def run(n, dim=3, cus=256, env=None, **kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        return ge.fa_schedule(n, dim, cus, **kw)
    return run


def test_names_cover_the_header():
    assert ge.FA_SCHED_SCALARS == ge.FA_SCHED_PLAN_SCALARS + ge.FA_SCHED_RUN_SCALARS
    assert len(ge.FA_SCHED_SCALARS) == ge.FA_SCHED_COUNT
    for name in ("ge_fa_sched_query", "ge_fa_plan_schedule"):
        assert name in ge.header_symbols() and name in ge._SIGS


# ---- the one-workgroup run: n <= small_max (64; GE_SMALL_MAX, at most kSmallMax = 512;
# wide: at most 256) and STRICT or wide (fa_run_device)
@pytest.mark.parametrize("n,dim,mode,env,small", [
    (64, 3, 0, {}, True), (65, 3, 0, {}, False),
    (512, 3, 0, {"GE_SMALL_MAX": "9999"}, True), (513, 3, 0, {"GE_SMALL_MAX": "9999"}, False),
    (10, 3, FAST, {}, False),  # FAST has no one-workgroup kernel
    (10, 5, FAST, {}, True),   # wide turns FAST into STRICT
    (256, 16, 0, {"GE_SMALL_MAX": "512"}, True), (257, 16, 0, {"GE_SMALL_MAX": "512"}, False),
])
def test_one_workgroup_run(sched, n, dim, mode, env, small):
    s = sched(n, dim, env=env, mode=mode, iterations=1000, nnz=4 * n)
    assert s["small"] is small
    if small:
        assert not s["persist"] and not s["graph"]


def test_one_workgroup_lanes_staging_and_handover(sched):
    # small_group: the knob-free G doubles while n G 2 <= T (at most 16); T = 1024 for the
    # domain-only kernel, 512 for the general one
    s = sched(64, iterations=1000, nnz=6144)
    assert (s["small_g_domain"], s["small_g_general"]) == (16, 8)
    assert s["small_staged"] and s["small_handover"] == 1000
    assert not sched(64, iterations=1000, nnz=6145)["small_staged"]  # kSmallNnz
    assert sched(64, 4, iterations=9, nnz=4096)["small_staged"]  # small_nnz_cap(4)
    assert not sched(64, 4, iterations=9, nnz=4097)["small_staged"]
    s = sched(500, env={"GE_SMALL_MAX": "512"}, iterations=9)
    assert (s["small_g_domain"], s["small_g_general"]) == (2, 1)
    # GE_SMALL_G where n g <= T; the domain-only kernel only for the linear attraction
    s = sched(40, env={"GE_SMALL_G": "4"}, iterations=9, linlog=1)
    assert (s["small_g_domain"], s["small_g_general"]) == (0, 4)
    s = sched(40, env={"GE_SMALL_G": "16"}, iterations=9, delta=2.0)
    assert (s["small_g_domain"], s["small_g_general"]) == (0, 8)  # 40 x 16 > 512: ignored
    assert sched(40, env={"GE_SMALL_G": "3"}, iterations=9)["small_g_general"] == 8  # invalid
    s = sched(40, env={"GE_SMALL_GENERAL_ONLY": "1", "GE_SMALL_HANDOVER": "37"}, iterations=99)
    assert (s["small_g_domain"], s["small_handover"]) == (0, 37)
    # wide: the general kernel from iteration 0, 256 threads, small_group mapped to 8 / 2 / 1
    for n, g in ((32, 8), (33, 2), (128, 2), (129, 1)):
        s = sched(n, 8, env={"GE_SMALL_MAX": "512"}, iterations=50)
        assert (s["small_g_domain"], s["small_g_general"], s["small_handover"]) == (0, g, 50)


# ---- the step: STRICT, n <= stream_max and no GE_GRP_SPLIT take the fused kernels, the
# stream above grouped_cap(d) (plan_step, launch_grouped_variant)
@pytest.mark.parametrize("n,dim,step", [
    (3072, 3, "fused"), (3073, 3, "stream"), (1536, 4, "fused"), (1537, 4, "stream"),
    (1228, 8, "fused"), (1229, 8, "stream"), (675, 16, "fused"), (676, 16, "stream"),
    (STREAM_MAX, 3, "stream"), (STREAM_MAX + 1, 3, "split"),
])
def test_step_kind(sched, n, dim, step):
    assert sched(n, dim)["step"] == step


def test_split_step_repulsion(sched):
    s = sched(STREAM_MAX + 1)  # past the stream: the whole level sweeps (plan_init)
    assert (s["step"], s["rep"], s["sym"]) == ("split", "sweeps", True)
    s = sched(STREAM_MAX + 1, rb=64)  # a row shard keeps the ordered-pair kernel
    assert (s["step"], s["rep"], s["sym"]) == ("split", "ordered", False)
    s = sched(300, env={"GE_GRP_SPLIT": "1"})  # n <= grouped_cap: fa_repulse_grouped
    assert (s["step"], s["rep"], s["lanes"], s["sym"]) == ("split", "grouped", 64, False)
    s = sched(300, mode=FAST)  # FAST is never fused
    assert (s["step"], s["rep"], s["mode"]) == ("split", "fast", FAST)
    # what ge_fa_plan_repulse runs on a fused plan: grouped up to grouped_cap, else ordered
    assert sched(3072)["rep"] == "grouped" and sched(3073)["rep"] == "ordered"
    # wide: the ordered-pair kernel at every size, general body, one row slot
    s = sched(700, 16)
    assert (s["rep"], s["R"], s["repel_one"], s["linear"], s["wide"]) == (
        "ordered_wide", 1, False, False, True)
    s = sched(700, 3, env={"GE_WIDE_MIN_DIM": "3", "GE_REP_R": "8"})
    assert (s["rep"], s["R"], s["repel_one"], s["linear"], s["wide"]) == (
        "ordered_wide", 1, False, False, True)


def test_body_flags(sched):
    # REPEL_ONE: repel == 1; LINEAR: !linlog && delta == 1 (launch_grouped_step_narrow)
    for kw, want in (({}, (True, True)), ({"repel": 2.0}, (False, True)),
                     ({"linlog": 1}, (True, False)), ({"repel": 0.5, "delta": 2.0}, (False, False))):
        s = sched(300, **kw)
        assert (s["repel_one"], s["linear"]) == want, kw


# ---- lanes per row: G doubles while rows G < 131072, at most 64, by the plan's rows
# (grouped_lanes); GE_STREAM_MAX keeps the larger levels on the fused stream here
@pytest.mark.parametrize("rows,G", [(2049, 64), (4096, 32), (8191, 32), (8192, 16),
                                    (131071, 2), (131072, 1)])
def test_lanes_per_row(sched, rows, G):
    s = sched(rows, env={"GE_STREAM_MAX": "200000"})
    assert (s["step"], s["lanes"]) == ("fused" if rows <= 3072 else "stream", G)
    assert sched(200000, rb=1000, re=1000 + rows, env={"GE_STREAM_MAX": "200000"})["lanes"] == G


def test_lanes_knobs_shards_and_wide(sched):
    assert sched(3000, rb=1500, re=3000)["lanes"] == 64
    assert sched(6000, rb=1500, re=3000)["lanes"] == 64 and sched(6000)["lanes"] == 32
    assert sched(300, env={"GE_GRP_G": "8"})["lanes"] == 8
    assert sched(300, env={"GE_GRP_G": "3"})["lanes"] == 64  # not a power of two: ignored
    assert sched(300, env={"GE_GRP_G": "128"})["lanes"] == 64
    # wide: a wave per row while grouped_lanes gives 32 or 64, else 8 (launch_grouped_step)
    assert sched(8191, 8)["lanes"] == 64 and sched(8192, 8)["lanes"] == 8
    assert sched(700, 8, env={"GE_GRP_G": "16"})["lanes"] == 8


# ---- fa_repulse_strict's grid (rep_grid): min(CUs or GE_REP_BLOCKS, 64-row slots) blocks,
# rows per block rounded up to 64; R = 8 above 1024 rows per block, else 1
@pytest.mark.parametrize("rows,env,per,nb,R", [
    (9088, {"GE_REP_BLOCKS": "2"}, 4544, 2, 8), (250000, {}, 1024, 245, 1),
    (500000, {}, 1984, 253, 8), (100, {}, 64, 2, 1),
])
def test_ordered_pair_grid(sched, rows, env, per, nb, R):
    env = dict(env, GE_FA_SYM="0")
    whole = sched(max(rows, 4000), re=rows, env=env)  # rows [0, rows) of a level past grouped_cap
    assert whole["rep"] == "ordered"
    assert (whole["per"], whole["nb"], whole["R"]) == (per, nb, R)
    s = sched(600000, rb=17, re=17 + rows, env=env)
    assert (s["rep"], s["per"], s["nb"], s["R"]) == ("ordered", per, nb, R)


def test_empty_shard_has_no_grid(sched):
    # rows == 0: the launch helpers return before any kernel (launch_repulsion), so the
    # schedule holds no grid, whatever the route
    for kw in ({}, {"mode": FAST}, {"dim": 8}):
        s = sched(70000, rb=5, re=5, **kw)
        assert (s["per"], s["nb"], s["fast_blocks"]) == (0, 0, 0), kw
    assert sched(300, rb=300, re=300)["lanes"] == 64


def test_ordered_pair_row_slots_knob(sched):
    assert sched(250000, env={"GE_REP_R": "4"})["R"] == 4
    assert sched(250000, env={"GE_REP_R": "3"})["R"] == 1  # not 1, 2, 4 or 8: ignored
    assert sched(500000, env={"GE_REP_R": "3"})["R"] == 8
    assert sched(250000, 8, env={"GE_REP_R": "4"})["R"] == 1  # wide
    assert (sched(250000, cus=304)["per"], sched(250000, cus=304)["nb"]) == (832, 301)
    assert (sched(250000, cus=8)["per"], sched(250000, cus=8)["nb"]) == (31296, 8)


# ---- sym: STRICT, narrow, the whole level, past stream_max or forced (plan_init)
def test_sym(sched):
    assert sched(STREAM_MAX + 1)["sym"] and not sched(STREAM_MAX)["sym"]
    s = sched(STREAM_MAX + 1, env={"GE_FA_SYM": "0"})
    assert (s["sym"], s["rep"]) == (False, "ordered")
    # GE_FA_SYM=1 up to stream_max: the plan holds the sweeps, its step is still the fused
    # one; only ge_fa_plan_repulse (or GE_GRP_SPLIT, GE_STREAM_MAX) reaches them
    s = sched(300, env={"GE_FA_SYM": "1"})
    assert (s["sym"], s["step"], s["rep"]) == (True, "fused", "sweeps")
    s = sched(300, env={"GE_FA_SYM": "1", "GE_GRP_SPLIT": "1"})
    assert (s["sym"], s["step"], s["rep"]) == (True, "split", "sweeps")
    s = sched(300, env={"GE_STREAM_MAX": "0"})
    assert (s["sym"], s["step"], s["rep"]) == (True, "split", "sweeps")
    for kw in ({"rb": 64}, {"mode": FAST}, {"dim": 8}):
        s = sched(STREAM_MAX + 1, env={"GE_FA_SYM": "1"}, **kw)
        assert not s["sym"] and s["rep"] != "sweeps", kw


# ---- FAST: blocks of 256 x 4 rows, min(16, ceil(n / 256)) j blocks (launch_repulsion_narrow)
def test_fast_grid(sched):
    s = sched(5000, mode=FAST)
    assert (s["rep"], s["fast_blocks"], s["fast_jb"], s["fpart"]) == ("fast", 5, 16, True)
    s = sched(1000, mode=FAST)
    assert (s["fast_blocks"], s["fast_jb"]) == (1, 4)
    s = sched(5000, rb=1024, re=2049, mode=FAST)  # the rows of the shard, the j range of n
    assert (s["fast_blocks"], s["fast_jb"]) == (2, 16)


# ---- FARFIELD: the reason in the order DIM, ROW_SHARD, MASS, SMALL, ACTIVE (plan_init)
def test_farfield(sched):
    s = sched(200000, 5, mode=FARFIELD)
    assert (s["far_reason"], s["mode"], s["rep"], s["fpart"]) == ("dim", 0, "ordered_wide", False)
    s = sched(200000, rb=64, mode=FARFIELD)
    assert (s["far_reason"], s["mode"], s["rep"], s["fpart"]) == ("row_shard", FAST, "fast", True)
    s = sched(131071, mode=FARFIELD)
    assert (s["far_reason"], s["mode"], s["rep"], s["fpart"]) == ("small", FAST, "fast", True)
    s = sched(131072, mode=FARFIELD)
    assert (s["far_reason"], s["mode"], s["step"], s["rep"], s["fpart"]) == (
        "active", FARFIELD, "split", "farfield", True)
    assert (s["fast_blocks"], s["fast_jb"]) == (128, 16)  # a non-finite box runs FAST
    s = sched(100, env={"GE_FAR_MIN": "100"}, mode=FARFIELD)
    assert (s["far_reason"], s["rep"]) == ("active", "farfield")
    assert sched(99, env={"GE_FAR_MIN": "100"}, mode=FARFIELD)["far_reason"] == "small"
    # the masses come before the size, after the dimension and the shard
    assert sched(131072, mode=FARFIELD, masses_ok=False)["far_reason"] == "mass"
    assert sched(100, mode=FARFIELD, masses_ok=False)["far_reason"] == "mass"
    assert sched(131072, rb=64, mode=FARFIELD, masses_ok=False)["far_reason"] == "row_shard"
    assert sched(131072, 5, rb=64, mode=FARFIELD, masses_ok=False)["far_reason"] == "dim"
    s = sched(131072, mode=FARFIELD, masses_ok=False)
    assert (s["mode"], s["rep"], s["fpart"]) == (FAST, "fast", True)
    assert sched(131072)["far_reason"] == "not_requested" and not sched(131072)["fpart"]
    for r, rows in (("1", 64), ("4", 256), ("7", 64)):
        assert sched(131072, env={"GE_FAR_R": r}, mode=FARFIELD)["far_item_rows"] == rows
    assert sched(131072, mode=FARFIELD)["far_item_rows"] == 64


# ---- the run (fa_run_device, launch_persistent)
def test_persistent_kernel_is_tried(sched):
    assert sched(300, iterations=128)["persist"] and not sched(300, iterations=127)["persist"]
    s = sched(300, iterations=128)
    assert (s["persist_g"], s["packed"], s["pack_rows"]) == (64, True, 0)
    assert sched(3072, iterations=128)["persist"] and not sched(3073, iterations=128)["persist"]
    assert sched(1536, 4, iterations=128)["persist"] and not sched(1537, 4, iterations=128)["persist"]
    assert not sched(300, iterations=128, mode=FAST)["persist"]
    assert not sched(300, 8, iterations=128)["persist"]  # wide
    assert not sched(300, env={"GE_WIDE_MIN_DIM": "3"}, iterations=128)["persist"]
    assert not sched(300, env={"GE_NO_PERSIST": "1"}, iterations=128)["persist"]
    assert not sched(64, iterations=128)["persist"]  # the one-workgroup run
    s = sched(3000, 2, env={"GE_GRP_G": "16", "GE_FA_PACK_ROWS": "6"}, iterations=128)
    assert (s["persist"], s["persist_g"], s["pack_rows"]) == (True, 16, 6)
    s = sched(300, env={"GE_FA_PACKED": "0", "GE_FA_PACK_ROWS": "6"}, iterations=128)
    assert (s["persist"], s["packed"], s["pack_rows"]) == (True, False, 0)
    assert sched(300, env={"GE_FA_PACK_ROWS": "5"}, iterations=128)["pack_rows"] == 4


def test_graph_replay(sched):
    assert sched(3100, iterations=128)["graph"] and not sched(3100, iterations=127)["graph"]
    assert not sched(3100, env={"GE_NO_GRAPH": "1"}, iterations=128)["graph"]
    assert sched(131071, iterations=128, mode=FARFIELD)["graph"]  # a FAST plan
    assert not sched(131072, iterations=128, mode=FARFIELD)["graph"]  # the far engine
    assert sched(131072, iterations=128, mode=FARFIELD, masses_ok=False)["graph"]
    assert sched(70000, iterations=128)["graph"]  # sweeps replay too


def test_bad_arguments(sched):
    for kw in ({"n": 0}, {"n": 10, "dim": 17}, {"n": 10, "rb": 5, "re": 4}, {"n": 10, "re": 11}):
        with pytest.raises(ge.GeError):
            sched(**kw)
