"""GPU parity against the reference itself: the device paths through the C ABI
against fixtures recorded from the reference's own translation units
(tests/golden/ref_*.npz, written by tests/golden/make_ref_fixtures.py from
oracle/_ref/ge_ref) -- no oracle in the chain.  Bit-identical (np.array_equal)
everywhere except F8, where device log / pow (ocml) meet glibc's.

The shapes are the smallest at which each device path is still selected; the
inputs are rebuilt from tests/ref_cases.py and their sha256 is asserted first, so
a drifted generator reads as a hash mismatch and not as a kernel bug.
"""
import numpy as np
import pytest

import ref_cases as C
from faml_plan import assert_census, assert_schedule, run_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def man():
    return C.manifest()


def _fa(ctx, man, golden, name):
    case = C.fa_case(name)
    assert C.input_hashes(case) == man["cases"][name]["inputs"]
    return C.run_fa(ctx.force_atlas, case), golden("ref_" + name)["x"]


def _ml(ctx, man, golden, name):
    case = C.ml_case(name)
    assert C.input_hashes(case) == man["cases"][name]["inputs"]
    return C.run_ml(ctx.force_atlas_ml, case), golden("ref_" + name)["x"]


# --------------------------------------------------------------------------
# single-level forceAtlas

@pytest.mark.parametrize("small_max", ["512", "0"])  # one workgroup / grouped multi-block
@pytest.mark.parametrize("name", ["F1_d2", "F1_d3"])
def test_f1_small_level(ctx, man, golden, monkeypatch, name, small_max):
    monkeypatch.setenv("GE_SMALL_MAX", small_max)
    got, want = _fa(ctx, man, golden, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("env", [{}, {"GE_FA_PACK_ROWS": "6"}, {"GE_FA_PACKED": "0"}],
                         ids=["pack4", "pack6", "nopack"])
def test_f2_persistent(ctx, man, golden, monkeypatch, env):
    """200 iterations in one launch (fa_grouped_persistent): packed rows, 4 or 6 per
    block, or one wave per row."""
    monkeypatch.setenv("GE_PERSIST_REQUIRE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, want = _fa(ctx, man, golden, "F2")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("split", ["0", "1"])
def test_f3_grouped(ctx, man, golden, monkeypatch, split):
    """One fused launch per iteration, or repulsion + row kernels (GE_GRP_SPLIT=1)."""
    if split == "1":
        monkeypatch.setenv("GE_GRP_SPLIT", "1")
    got, want = _fa(ctx, man, golden, "F3")
    assert np.array_equal(got, want)


def test_f4_grouped_stream(ctx, man, golden):
    """fa_grouped_stream with one coordinate outside the exact-division domain."""
    got, want = _fa(ctx, man, golden, "F4")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("env", [{"GE_FA_SYM": "1"}, {"GE_FA_SYM": "0"}, {"GE_ROWS_TILES": "1"},
                                 {"GE_ROWS_TILES": "1", "GE_ROWS_SEGMENTS": "0"}],
                         ids=["sym", "ordered", "tiles", "tiles-whole-rows"])
def test_f5_large_level_kernels(ctx, man, golden, monkeypatch, env):
    """The large-level kernels on rows at and around the tile capacity and a heavy
    row: symmetric sweeps, ordered pairs, tiled rows with segments or whole rows."""
    monkeypatch.setenv("GE_STREAM_MAX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, want = _fa(ctx, man, golden, "F5")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["F6_nondefault", "F6_nohubs_normalize", "F7"])
def test_f6_f7_options_and_seeded_start(ctx, man, golden, name):
    got, want = _fa(ctx, man, golden, name)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", C.FA_TOLERANT)
def test_f8_linlog_delta(ctx, man, golden, name):
    """Device log / pow (ocml) against glibc: the project's bar for them, 1e-12
    relative after one iteration (tests/test_gpu_configs.py)."""
    got, want = _fa(ctx, man, golden, name)
    assert np.allclose(got, want, rtol=1e-12, atol=0.0)


# --------------------------------------------------------------------------
# multilevel

def test_m1_packed_size_classes(ctx, man, golden):
    got, want = _ml(ctx, man, golden, "M1")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("env", [{"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"},
                                 {"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "1e9"},
                                 {"GE_FAML_SYM": "1"}, {"GE_FAML_SYM": "0"}],
                         ids=["sweeps", "row-blocks", "plan-mix", "ordered"])
@pytest.mark.parametrize("name", ["M2_d2", "M2_d3", "M2_d2_repel", "M2_d3_repel"])
def test_m2_streamed_aggregates(ctx, man, golden, monkeypatch, name, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, want = _ml(ctx, man, golden, name)
    assert np.array_equal(got, want)


def test_m3_streamed_path(ctx, man, golden):
    got, want = _ml(ctx, man, golden, "M3")
    assert np.array_equal(got, want)


def _ml_plan(ctx, man, golden, monkeypatch, name, env=None):
    """A case through ge_faml_plan_* under the GE_FAML_RES_CAP its size classes need:
    (coordinates, the fixture's, the sizes by class, the plan's census and schedule)."""
    case = C.ml_case(name)
    assert C.input_hashes(case) == man["cases"][name]["inputs"]
    knob = C.ML_RES_CAP.get(name)
    if knob is None:
        monkeypatch.delenv("GE_FAML_RES_CAP", raising=False)
    else:
        monkeypatch.setenv("GE_FAML_RES_CAP", knob)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    got, cls, sched = run_plan(ctx, case)
    by_class = assert_census(cls, list(np.diff(case["PT"][0])), case["dim"], knob)
    return got, golden("ref_" + name)["x"], by_class, cls, sched


def test_m4_options_large_resident(ctx, man, golden, monkeypatch):
    """Every scalar option on fractional weights in faml_resident<3, 256, 4096>."""
    got, want, by_class, cls, _ = _ml_plan(ctx, man, golden, monkeypatch, "M4_options")
    assert by_class["large"] == [1031, 700, 257] and cls["blocks_large"] == 3
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", ["sweeps", "row-blocks", "ordered"])
@pytest.mark.parametrize("name", ["M4_nohubs_unweighted", "M5_weight_edges"])
def test_m4_m5_streamed(ctx, man, golden, monkeypatch, name, mode):
    """nohubs with the weights ignored, and one 2^61 edge per aggregate (two members of
    each outside weight_ok, in different row tiles of the largest), on the streamed
    aggregates as sweeps, row blocks and ordered pairs."""
    env = {"sweeps": {"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "0"},
           "row-blocks": {"GE_FAML_SYM": "1", "GE_FAML_SYM_CHAIN": "1e9"},
           "ordered": {"GE_FAML_SYM": "0"}}[mode]
    got, want, by_class, cls, sched = _ml_plan(ctx, man, golden, monkeypatch, name, env)
    assert by_class["streamed"] == [2600, 320, 700, 257, 1031, 300] and not by_class["large"]
    assert_schedule(sched, cls, by_class["streamed"], mode)
    assert np.array_equal(got, want)


def test_m5_coarse_edges_packed(ctx, man, golden, monkeypatch):
    """coords_A outside the domain, at the origin, shared by two joined aggregates, and
    r_A = 0, in the packed 64- and 256-member kernels."""
    got, want, by_class, cls, _ = _ml_plan(ctx, man, golden, monkeypatch, "M5_coarse_edges")
    assert not by_class["large"] and not by_class["streamed"]
    assert cls["blocks_small"] >= 2 and cls["blocks_mid"] >= 2
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name,large", [("M6_d1", [1000, 257]), ("M6_d4", [2048, 257])])
def test_m6_dims_1_and_4(ctx, man, golden, monkeypatch, name, large):
    """dim 1, and dim 4 with the large kernel at its capacity (2048 eight-double records),
    every resident class in one level."""
    got, want, by_class, cls, _ = _ml_plan(ctx, man, golden, monkeypatch, name)
    assert by_class["large"] == large and by_class["small"] and by_class["mid"]
    assert cls["blocks_large"] == len(large) and not by_class["streamed"]
    assert np.array_equal(got, want)


# --------------------------------------------------------------------------
# partition, embed, modularity

@pytest.mark.parametrize("name", C.P_NAMES)
def test_p_partition(ctx, man, golden, name):
    case = C.p_case(name)
    assert C.input_hashes(case) == man["cases"]["P_" + name]["inputs"]
    g = golden("ref_P_" + name)
    kw = {{"matching": "matching_iterations"}.get(k, k): v for k, v in case["kw"].items()}
    for cf in C.P_CFS:
        assert C.same_hier(ctx.partition(case["A"], cf, **kw),
                           C.hier_from(g, "cf" + C.cf_key(cf))), cf


def _device_levels(ctx, A, hier):
    As = [A]
    for PT in hier:
        As.append(ctx.ptap(As[-1], PT))
    return As


@pytest.mark.parametrize("d", C.E_DIMS)
def test_e_embed(ctx, man, golden, d):
    g = golden("ref_E")
    entry = man["cases"]["E"]
    hier = C.hier_from(g, "h")
    As = _device_levels(ctx, C.e_graph(), hier)
    assert C.input_hashes({"As": As}) == entry["inputs"]
    X = ctx.embed(As, hier, d, seed=entry["seed"])  # the reference's 100000 / 100 iterations
    assert np.array_equal(X, g[f"x_d{d}"])


def test_q_modularity(ctx, man, golden):
    g = golden("ref_E")
    hier = C.hier_from(g, "h")
    pairs = list(zip(_device_levels(ctx, C.e_graph(), hier), hier, man["cases"]["E"]["modularity"]))
    gp = golden("ref_P_rmat")
    for cf in C.P_CFS:
        hp = C.hier_from(gp, "cf" + C.cf_key(cf))
        pairs += list(zip(_device_levels(ctx, C.p_graph("rmat"), hp), hp,
                          man["cases"]["P_rmat"]["modularity"][C.cf_key(cf)]))
    assert len(pairs) >= 4
    for Al, PT, h in pairs:
        assert ctx.modularity(Al, C.vertex_of(PT), PT[2]) == float.fromhex(h)
