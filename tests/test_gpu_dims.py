"""Dimensions 5..16 on the device, bit for bit (np.array_equal) against the fixtures
recorded from the reference (tests/golden/ref_dims_*.npz, tests/dims_cases.py) and
against the oracle.

Above dimension 4 the library runs its "wide" schedule (csrc/ge_pair.hpp): the
one-workgroup kernel's general form (up to 256 rows), the fused per-iteration step
(graph replay for long runs), the ordered-pair streamed kernels and the CSR row
kernels, single level and multilevel, with LDS budgets derived per dimension.  There
is no persistent kernel or symmetric sweep there, so long runs replay a graph.  The sizes
are the smallest at which each of these paths is still selected.  GE_WIDE_MIN_DIM
sends dimension 2..4 through the same schedule, where the older goldens pin it.
"""
import numpy as np
import pytest

import dims_cases as D
import fa_route as route
import faml_plan as FP
import ge_amd as ge
import graphs as G
import ref_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def man():
    return D.manifest()


def rec_width(d):
    """Doubles per LDS member record (ge_pair.hpp rec_width)."""
    return 4 if d + 1 <= 4 else 8 if d + 1 <= 8 else (d + 2) & ~1


def large_cap(d):
    """Members of the largest LDS-resident aggregate (ge_faml.hip large_cap): 128 KiB of
    records, or what 159 KiB leave after the kernel's other arrays."""
    left = 160 * 1024 - 1024 - (4 * 513 + 8 * 256 * (d + 1) + 16)
    return min(left, 128 * 1024) // (8 * rec_width(d))


SMALL_WIDE_CAP = 256  # rows of the one-workgroup kernel above d = 4 (ge_fa_sched.hpp small_cap)
# GE_SMALL_MAX: "512" takes the one-workgroup kernel up to its cap, "0" never
SMALL = pytest.mark.parametrize("small_max", ["512", "0"], ids=["one-workgroup", "fused"])


def small_or_fused(A, d, iterations, small_max, **kw):
    """The route of a SMALL case below 128 iterations, from the schedule."""
    n = len(A[0]) - 1
    want = "fa_small_strict" if small_max == "512" and n <= SMALL_WIDE_CAP else "fa_grouped_step"
    return route.run_kernel(A, d, iterations, **kw) == want


# --------------------------------------------------------------------------
# single level

@SMALL
@pytest.mark.parametrize("d", D.ALL_DIMS)
def test_fa_every_dimension(ctx, oracle, monkeypatch, d, small_max):
    """Odd widths: padding and indexing of the records and the term buffers, in the
    one-workgroup kernel and in the fused step."""
    monkeypatch.setenv("GE_SMALL_MAX", small_max)
    A = G.erdos_renyi(130, 0.06, seed=d)
    assert small_or_fused(A, d, 3, small_max)
    want = oracle.force_atlas(A, d, iterations=3, seed=d)
    assert np.array_equal(ctx.force_atlas(A, d, iterations=3, seed=d), want)


@SMALL
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_one_and_two_vertices(ctx, oracle, monkeypatch, d, small_max):
    """(one workgroup: 8 lanes per row)"""
    monkeypatch.setenv("GE_SMALL_MAX", small_max)
    one = (np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0))
    x1 = G.random_coords(1, d, seed=d)
    assert small_or_fused(one, d, 7, small_max)
    assert small_max == "0" or route.schedule(1, d, iterations=7)["small_g_general"] == 8
    assert np.array_equal(ctx.force_atlas(one, d, coords=x1, iterations=7),
                          oracle.force_atlas(one, d, coords=x1, iterations=7))
    two = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.ones(2))
    x2 = G.random_coords(2, d, seed=d + 1)
    assert small_or_fused(two, d, 7, small_max)
    assert np.array_equal(ctx.force_atlas(two, d, coords=x2, iterations=7),
                          oracle.force_atlas(two, d, coords=x2, iterations=7))


@SMALL
@pytest.mark.parametrize("n", [63, 64, 65, SMALL_WIDE_CAP, SMALL_WIDE_CAP + 1])
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_one_workgroup_sizes(ctx, oracle, monkeypatch, d, n, small_max):
    """fa_small_strict<D, G, 256> (general form) with 2 lanes per row (the schedule gives
    2 from 33 to 128 rows, so 63, 64 and 65 all take them) and one (256), and both sides of
    its cap of 256 rows, where the fused step takes over; the same sizes on the fused step,
    one wave per row."""
    monkeypatch.setenv("GE_SMALL_MAX", small_max)
    A = G.erdos_renyi(n, 0.1, seed=n)
    s = route.schedule(n, d, iterations=30)
    assert small_or_fused(A, d, 30, small_max)
    assert s["small_g_general"] == (2 if n <= 128 else 1) if s["small"] else s["lanes"] == 64
    x0 = G.random_coords(n, d, seed=n)
    want = oracle.force_atlas(A, d, coords=x0, iterations=30)
    assert np.array_equal(ctx.force_atlas(A, d, coords=x0, iterations=30), want)


@SMALL
@pytest.mark.parametrize("name", D.fa_names())
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_fixture(ctx, oracle, man, monkeypatch, d, name, small_max):
    """n = 130 in the one-workgroup kernel and on the fused step: 1, 2 (Fprev matters) and
    25 iterations, supplied and seeded start, and the option / domain-edge cases, against
    the reference's bits."""
    monkeypatch.setenv("GE_SMALL_MAX", small_max)
    case = D.fa_case(name, d)
    assert C.input_hashes(case) == man["cases"][f"fa_d{d}"][name]["inputs"]
    assert small_or_fused(case["A"], d, case["iterations"], small_max, **case["kw"])
    got = C.run_fa(ctx.force_atlas, case)
    assert np.array_equal(got, D.load("fa", d)[name])
    assert np.array_equal(got, C.run_fa(oracle.force_atlas, case))


@pytest.mark.parametrize("d", D.DIMS)
def test_fa_long_run_graph_replay(ctx, oracle, d):
    """130 iterations (>= kPersistMin = 128 and >= 4 x 32): no persistent kernel above
    d = 4, so the plan replays the captured graph of 32 fused steps, then 2 plain ones."""
    case = D.fa_case("start_it1", d)
    assert route.run_kernel(case["A"], d, 130) == "fa_grouped_step"
    assert route.schedule(D.FA_N, d, iterations=130)["graph"]
    want = oracle.force_atlas(case["A"], d, coords=case["x0"], iterations=130)
    assert np.array_equal(ctx.force_atlas(case["A"], d, coords=case["x0"], iterations=130), want)


@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_ordered_pair_kernel(ctx, man, monkeypatch, d, tiles):
    """n = 130 forced past the streamed bound: fa_repulse_strict (one ragged tile of
    partners, one ragged wave slot) and the CSR row kernels, classed or tiled."""
    monkeypatch.setenv("GE_STREAM_MAX", "0")
    monkeypatch.setenv("GE_ROWS_TILES", tiles)
    for name in ("start_it25", "repel_2p70", "tiny", "isolated"):
        case = D.fa_case(name, d)
        assert route.run_kernel(case["A"], d, case["iterations"],
                                **case["kw"]) == "fa_repulse_strict_wide+rows", name
        assert np.array_equal(C.run_fa(ctx.force_atlas, case), D.load("fa", d)[name]), name


def grouped_cap(d):
    """Records the fused step keeps resident (ge_fa_sched.hpp grouped_cap): what 159 KiB leave
    after the two term buffers of 256 x d doubles, at most 96 KiB."""
    return min(160 * 1024 - 1024 - 2 * 256 * d * 8, 96 * 1024) // (8 * rec_width(d))


@pytest.mark.parametrize("grp", [None, "8"], ids=["wave-per-row", "8-lanes"])
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_resident_and_streamed_records(ctx, oracle, monkeypatch, d, grp):
    """Both sides of grouped_cap(d): fa_grouped_step with every record in LDS, and
    fa_grouped_stream with tiles of stream_tile(d) records and a ragged last one; with
    the wide schedule's two group sizes."""
    if grp:
        monkeypatch.setenv("GE_GRP_G", grp)
    for n in (grouped_cap(d), grouped_cap(d) + 1):
        A = G.rmat(n, 5 * n, seed=n)  # isolated vertices included
        x0 = G.random_coords(n, d, seed=d)
        x0[n // 2, d - 1] = C.TINY  # one tile outside the exact-division domain
        assert route.run_kernel(A, d, 2) == (
            "fa_grouped_step" if n == grouped_cap(d) else "fa_grouped_stream"), n
        assert route.schedule(n, d)["lanes"] == (8 if grp else 64)
        want = oracle.force_atlas(A, d, coords=x0, iterations=2)
        assert np.array_equal(ctx.force_atlas(A, d, coords=x0, iterations=2), want), n


def test_fa_group_size_threshold(ctx, oracle):
    """8191 rows take a wave per row, 8192 take 8 lanes (launch_grouped_step)."""
    for n in (8191, 8192):
        A = G.rmat(n, 4 * n, seed=7)
        x0 = G.random_coords(n, 5, seed=3)
        assert route.run_kernel(A, 5, 1) == "fa_grouped_stream"
        assert route.schedule(n, 5)["lanes"] == (64 if n == 8191 else 8)
        want = oracle.force_atlas(A, 5, coords=x0, iterations=1)
        assert np.array_equal(ctx.force_atlas(A, 5, coords=x0, iterations=1), want), n


@pytest.mark.parametrize("stream_max", [None, "0"], ids=["fused", "rows"])
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_plan_row_shard(ctx, oracle, monkeypatch, d, stream_max):
    """Rows (37, 101) through FaPlan.step against the oracle's step for those rows: the
    fused step, and the ordered-pair + row kernels, on a shard."""
    torch = pytest.importorskip("torch")
    if stream_max is not None:
        monkeypatch.setenv("GE_STREAM_MAX", stream_max)
    rb, re = 37, 101
    case = D.fa_case("start_it1", d)
    A, x0 = C.symmetric_weights(case["A"]), case["x0"]
    n = D.FA_N
    assert route.step_kernel(n, d, rb=rb, re=re) == (
        "fa_grouped_step" if stream_max is None else "fa_repulse_strict_wide+rows")
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in A]
    x = torch.from_numpy(x0.copy()).to(dev)
    y = torch.zeros_like(x)
    plan = ctx.fa_plan(n, len(A[1]), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), d, rb, re)
    deg = oracle.degrees(A)
    fprev = np.zeros((re - rb, d))
    cur = x0.copy()
    try:
        for _ in range(3):
            plan.step(x.data_ptr(), y.data_ptr())
            ctx.sync()
            nxt = cur.copy()
            oracle.fa_step_rows(A, cur, deg, rb, re, fprev, nxt)
            got = y.cpu().numpy()
            assert np.array_equal(got[rb:re], nxt[rb:re])
            # the other rows move too (another shard's work): keep both sides in step
            nxt[:rb] += 0.01
            nxt[re:] -= 0.01
            cur = nxt
            x.copy_(torch.from_numpy(cur))
    finally:
        plan.close()


@pytest.mark.parametrize("segments", ["1", "0"])
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_heavy_rows(ctx, oracle, monkeypatch, d, segments):
    """Hub rows longer than a row tile (512 entries) and a chunk of the split sum:
    heavy rows as binade-sum segments (heavy_finish_kernel) or whole rows
    (ordered_edge_sum_split, split_chunk(d) terms per chunk), rows at the tile bound."""
    monkeypatch.setenv("GE_STREAM_MAX", "0")
    monkeypatch.setenv("GE_ROWS_TILES", "1")
    monkeypatch.setenv("GE_ROWS_SEGMENTS", segments)
    A = G.with_degrees(G.rmat(1500, 6000, seed=d), {7: 511, 8: 512, 9: 513, 300: 1100}, seed=d)
    deg = np.diff(A[0])
    assert list(deg[[7, 8, 9, 300]]) == [511, 512, 513, 1100] and (deg == 0).any()
    A = C.symmetric_weights(A)
    x0 = G.random_coords(1500, d, seed=d)
    assert route.run_kernel(A, d, 3) == "fa_repulse_strict_wide+rows"
    want = oracle.force_atlas(A, d, coords=x0, iterations=3)
    assert np.array_equal(ctx.force_atlas(A, d, coords=x0, iterations=3), want)


@pytest.mark.parametrize("d", D.DIMS)
def test_fa_classed_heavy_row(ctx, oracle, monkeypatch, d):
    """Without tiles a row above 2048 entries takes one block (ordered_edge_sum_split),
    rows above 4 entries a wave."""
    monkeypatch.setenv("GE_STREAM_MAX", "0")
    monkeypatch.setenv("GE_ROWS_TILES", "0")
    A = G.with_hubs(G.rmat(2600, 9000, seed=d), [(5, 2300)], seed=d)
    assert np.diff(A[0]).max() > 2048
    x0 = G.random_coords(2600, d, seed=d)
    assert route.run_kernel(A, d, 2) == "fa_repulse_strict_wide+rows"
    want = oracle.force_atlas(A, d, coords=x0, iterations=2)
    assert np.array_equal(ctx.force_atlas(A, d, coords=x0, iterations=2), want)


@pytest.mark.parametrize("kw", [dict(linlog=1), dict(delta=0.5), dict(linlog=1, delta=0.5)],
                         ids=["linlog", "delta", "linlog-delta"])
@pytest.mark.parametrize("d", D.DIMS)
def test_fa_linlog_delta(ctx, oracle, d, kw):
    """Device log / pow (ocml) against glibc's: the project's bar, 1e-12 relative after
    one iteration.  delta acts on the weights, so they are fractional."""
    case = D.fa_case("start_it1", d)
    A = C.symmetric_weights(case["A"])
    want = oracle.force_atlas(A, d, coords=case["x0"], iterations=1, **kw)
    got = ctx.force_atlas(A, d, coords=case["x0"], iterations=1, **kw)
    assert np.allclose(got, want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("d", [5, 16])
def test_fa_overflowing_repel(ctx, oracle, d):
    """repel = 1e299: cij / eps^2 overflows for the self pair, which the `/` bodies must
    skip as the reference does.  (No width is padded, so no padded component exists.)"""
    case = D.fa_case("start_it1", d)
    want = oracle.force_atlas(case["A"], d, coords=case["x0"], iterations=1, repel=1e299)
    got = ctx.force_atlas(case["A"], d, coords=case["x0"], iterations=1, repel=1e299)
    assert np.isfinite(got).all() and np.array_equal(got, want)


def test_fa_fast_mode_runs_the_exact_kernels(ctx, oracle):
    """GE_MODE_FAST has no kernels above d = 4: it returns the STRICT bits."""
    case = D.fa_case("start_it2", 8)
    assert route.schedule(D.FA_N, 8, mode=ge.MODE_FAST)["mode"] == ge.MODE_STRICT
    assert route.run_kernel(case["A"], 8, 2, mode=ge.MODE_FAST) == "fa_grouped_step"
    got = ctx.force_atlas(case["A"], 8, coords=case["x0"], iterations=2, mode=ge.MODE_FAST)
    assert np.array_equal(got, D.load("fa", 8)["start_it2"])


# --------------------------------------------------------------------------
# multilevel, through the plan and its census

def _plan(ctx, monkeypatch, case, knob):
    """run_plan under GE_FAML_RES_CAP = knob; the census against the per-dimension
    large_cap (tests/faml_plan.py restates the rule for d <= 4)."""
    if knob is None:
        monkeypatch.delenv("GE_FAML_RES_CAP", raising=False)
    else:
        monkeypatch.setenv("GE_FAML_RES_CAP", knob)
    monkeypatch.setattr(FP, "large_cap", large_cap)
    got, cls, sched = FP.run_plan(ctx, case)
    by_class = FP.assert_census(cls, list(np.diff(case["PT"][0])), case["dim"], knob)
    # no symmetric sweeps above d = 4: the streamed aggregates run the ordered-pair kernel
    FP.assert_schedule(sched, cls, by_class["streamed"], "ordered")
    return got, by_class, cls


def _ml_graph(n, seed):
    return C.symmetric_weights(G.submatrix(G.rmat(n, 6 * n, seed=seed), np.arange(n)))


CLASS_SIZES = [1, 2, 63, 64, 65, 256, 257, 300]


@pytest.mark.parametrize("d", D.DIMS)
def test_faml_class_boundaries(ctx, oracle, monkeypatch, d):
    """Aggregates of 1, 2, 63, 64 (64-lane packs), 65, 256 (256-member packs), and under
    GE_FAML_RES_CAP=256 257 and a ragged 300 on the streamed ordered-pair kernel."""
    n = sum(CLASS_SIZES)
    case = C._ml(_ml_graph(n, d), CLASS_SIZES, d, d, 3, 23)
    got, by_class, cls = _plan(ctx, monkeypatch, case, "256")
    assert by_class["small"] == [1, 2, 63, 64] and by_class["mid"] == [65, 256]
    assert by_class["streamed"] == [257, 300] and not by_class["large"]
    assert np.array_equal(got, C.run_ml(oracle.force_atlas_ml, case))


@pytest.mark.parametrize("d", D.DIMS)
def test_faml_large_cap_boundary(ctx, oracle, monkeypatch, d):
    """Both sides of large_cap(d): the largest aggregate faml_resident holds in LDS at
    this record width, and one member more, which streams."""
    cap = large_cap(d)
    sizes = [cap, cap + 1, 257, 30]
    n = sum(sizes)
    case = C._ml(_ml_graph(n, d), sizes, d, d, 2, 29)
    got, by_class, cls = _plan(ctx, monkeypatch, case, "4096")
    assert cls["res_cap"] == cap
    assert by_class["large"] == [cap, 257] and cls["blocks_large"] == 2
    assert by_class["streamed"] == [cap + 1] and by_class["small"] == [30]
    assert np.array_equal(got, C.run_ml(oracle.force_atlas_ml, case))


@pytest.mark.parametrize("name", ["er90", "M1"])
@pytest.mark.parametrize("d", D.DIMS)
def test_faml_fixture(ctx, man, monkeypatch, d, name):
    """12 iterations against the reference's bits: ER(90) with partition(A, 0.2), and
    M1's aggregates of 1..256 members."""
    case = D.ml_case(name, d)
    assert C.input_hashes(case) == man["cases"][f"ml_d{d}"][name]["inputs"]
    want = D.load("ml", d)[name]
    assert np.array_equal(C.run_ml(ctx.force_atlas_ml, case), want)
    got, by_class, _ = _plan(ctx, monkeypatch, case, None)
    assert not by_class["large"] and not by_class["streamed"]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tiles", ["0", "1"])
def test_faml_fixture_streamed_hubs(ctx, man, monkeypatch, tiles):
    """M2 at d = 5 under GE_FAML_RES_CAP=256: streamed aggregates of 257..2600 members
    with two hub rows, as whole rows or as stored segments with their chains."""
    monkeypatch.setenv("GE_ROWS_TILES", tiles)
    case = D.ml_case("M2", 5)
    assert C.input_hashes(case) == man["cases"]["ml_d5"]["M2"]["inputs"]
    got, by_class, cls = _plan(ctx, monkeypatch, case, "256")
    assert by_class["streamed"] == [2600, 320, 700, 257, 1031, 300]
    if tiles == "1":
        assert cls["nseg"] > 0 and cls["nheavy"] >= 2
    assert np.array_equal(got, D.load("ml", 5)["M2"])


@pytest.mark.parametrize("d", D.ALL_DIMS)
def test_faml_every_dimension(ctx, oracle, d):
    sizes = C.M1_SIZES
    case = C._ml(C.layout_graph("packed"), sizes, sum(sizes), d, 2, 31)
    assert np.array_equal(C.run_ml(ctx.force_atlas_ml, case),
                          C.run_ml(oracle.force_atlas_ml, case))


# --------------------------------------------------------------------------
# radius step and embed

def _oracle_radius(oracle, cA, dim, base, PTc=None, cAc=None, rAc=None, Ac=None):
    import test_gpu_radius as TR
    return TR._oracle_radius(oracle, cA, dim, base, PTc, cAc, rAc, Ac)


@pytest.mark.parametrize("d", [5, 16])
def test_radius_base_case(ctx, oracle, d):
    cA = G.random_coords(40, d, seed=40)
    r1, c1, dev = ctx.radius_step(cA, d, True)
    r2, c2 = _oracle_radius(oracle, cA, d, True)
    assert dev and np.array_equal(r1, r2) and np.array_equal(c1, c2)


@pytest.mark.parametrize("d", [5, 16])
def test_radius_grouped(ctx, oracle, d):
    A = G.largest_component(G.rmat(4096, 40000, seed=12345))
    hier = oracle.partition(A, 0.125)
    As = oracle.hierarchy_As(A, hier)
    l = 0
    m = len(As[l + 1][0]) - 1
    PTc = hier[l + 1]
    cA = G.random_coords(m, d, seed=l)
    cAc = G.random_coords(PTc[2], d, seed=l + 10)
    rAc = np.random.RandomState(l).uniform(0.1, 1.0, PTc[2])
    r2, c2 = _oracle_radius(oracle, cA, d, False, PTc, cAc, rAc, As[l + 1])
    r1, c1, dev = ctx.radius_step(cA, d, False, PTc=PTc, coords_Ac=cAc, r_Ac=rAc, Ac=As[l + 1])
    assert dev and np.array_equal(r1, r2) and np.array_equal(c1, c2)


@pytest.mark.parametrize("d", D.E_DIMS)
def test_embed_fixture(ctx, man, d):
    """Context.embed end to end, the reference's own 100 000 / 100 iterations."""
    g = D.load_embed()
    entry = man["cases"]["embed"]
    hier = C.hier_from(g, "h")
    As = [D.e_graph()]
    for PT in hier:
        As.append(ctx.ptap(As[-1], PT))
    assert C.input_hashes({"As": As}) == entry["inputs"]
    assert np.array_equal(ctx.embed(As, hier, d, seed=entry["seed"]), g[f"x_d{d}"])


# --------------------------------------------------------------------------
# arguments

@pytest.mark.parametrize("d", [0, 17])
def test_dimension_out_of_range(ctx, d):
    torch = pytest.importorskip("torch")
    A = G.erdos_renyi(20, 0.3, seed=1)
    w = max(d, 1)

    def names_range(call):
        with pytest.raises(ge.GeError, match=r"1\.\.16"):
            call()

    names_range(lambda: ctx.force_atlas(A, d, coords=np.zeros((20, w)), iterations=1))
    PT = (np.array([0, 10, 20], np.int32), np.arange(20, dtype=np.int32), 2, 20)
    vA = ge.vertex_of(PT)
    names_range(lambda: ctx.force_atlas_ml(A, PT, vA, np.zeros((2, w)), np.ones(2), d,
                                           iterations=1))
    names_range(lambda: ctx.embed([A], [], d, base_iterations=1, ml_iterations=1))
    cA, rA = np.zeros(3 * w), np.zeros(3)  # (the C ABI: the wrapper sizes its arrays by dim)
    rc = ge.lib().ge_radius_step_device(ctx.h, 3, cA, rA, d, 1, 0, None, None, None, None, None,
                                        None, None)
    assert rc != 0 and "1..16" in ge.lib().ge_last_error().decode()
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in A]
    names_range(lambda: ctx.fa_plan(20, len(A[1]), t[0].data_ptr(), t[1].data_ptr(),
                                    t[2].data_ptr(), d, 0, 20))
    p = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (PT[0], PT[1], vA)]
    names_range(lambda: ge.FamlPlan(ctx, 20, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                    PT[0], p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), d))


# --------------------------------------------------------------------------
# the wide schedule at d <= 4 (GE_WIDE_MIN_DIM), against the goldens of the older paths

@pytest.mark.parametrize("name", ["F1_d2", "F1_d3", "F7"])
def test_wide_one_workgroup_reproduces_reference_fixtures(ctx, golden, monkeypatch, name):
    """The wide schedule's one-workgroup kernel at d = 2, 3 against the reference's bits
    (n = 97 over 30 iterations, a seeded start over 20)."""
    monkeypatch.setenv("GE_WIDE_MIN_DIM", "1")
    monkeypatch.setenv("GE_SMALL_MAX", "512")
    case = C.fa_case(name)
    assert len(case["A"][0]) - 1 <= SMALL_WIDE_CAP
    assert route.run_kernel(case["A"], case["dim"], case["iterations"], **case["kw"]) == "fa_small_strict"
    assert route.schedule(97, case["dim"])["wide"]
    assert np.array_equal(C.run_fa(ctx.force_atlas, case), golden("ref_" + name)["x"])


def test_wide_schedule_reproduces_fa_goldens(ctx, golden, monkeypatch):
    monkeypatch.setenv("GE_WIDE_MIN_DIM", "1")
    g = golden("fa_er300_d3")
    A = (g["A_ip"], g["A_ix"], g["A_dx"])
    for it in (1, 10, 100):
        assert np.array_equal(ctx.force_atlas(A, 3, coords=g["x0"], iterations=it),
                              g[f"x_it{it}"]), it
    g = golden("fa_rmat_d2_seeded")
    A = (g["A_ip"], g["A_ix"], g["A_dx"])
    assert np.array_equal(ctx.force_atlas(A, 2, iterations=20, seed=int(g["seed"])), g["x_it20"])


@pytest.mark.parametrize("stream_max", [None, "0"], ids=["fused", "rows"])
def test_wide_schedule_equals_default_at_d4(ctx, monkeypatch, stream_max):
    if stream_max is not None:
        monkeypatch.setenv("GE_STREAM_MAX", stream_max)
    A = G.rmat(1300, 8 * 1300, seed=1300)
    x0 = G.random_coords(1300, 4, seed=1)
    want = ctx.force_atlas(A, 4, coords=x0, iterations=5)
    monkeypatch.setenv("GE_WIDE_MIN_DIM", "4")
    assert route.schedule(1300, 4)["wide"] and route.run_kernel(A, 4, 5) == (
        "fa_grouped_step" if stream_max is None else "fa_repulse_strict_wide+rows")
    assert np.array_equal(ctx.force_atlas(A, 4, coords=x0, iterations=5), want)


def test_wide_schedule_reproduces_faml_goldens(ctx, golden, monkeypatch):
    monkeypatch.setenv("GE_WIDE_MIN_DIM", "1")
    g = golden("faml_rmat4096_l0")
    A = (g["A_ip"], g["A_ix"], g["A_dx"])
    X = ctx.force_atlas_ml(A, (g["P_ip"], g["P_ix"]), g["vA"], g["cA"], g["rA"], 3,
                           iterations=100, seed=int(g["seed"]))
    assert np.array_equal(X, g["x_it100"])
    # dim 4 with streamed aggregates (GE_FAML_RES_CAP=256: 2048 and 257 members stream)
    monkeypatch.setenv("GE_FAML_RES_CAP", "256")
    case = C.ml_case("M6_d4")
    assert np.array_equal(C.run_ml(ctx.force_atlas_ml, case), golden("ref_M6_d4")["x"])
