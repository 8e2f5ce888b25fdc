"""The oracle (oracle/ge_oracle.cpp) and the host library against the reference's
own code: LLNL/graph-embed's src/partitioner.cpp, src/embed.cpp,
src/matrixutils.cpp and include/forceatlas.hpp compiled unmodified into
oracle/_ref/ge_ref (oracle/Makefile, oracle/ref_shim.hpp, oracle/ref_driver.cpp).

Two kinds of test:
  - committed fixtures recorded from that binary (tests/golden/ref_*.npz,
    tests/golden/make_ref_fixtures.py) are reproduced bit for bit -- these run
    anywhere;
  - live runs of the binary on a wider sweep -- these need the binary, which is
    built wherever the reference tree is present (then a build failure fails the
    tests) and skip only where neither the tree nor a shipped binary exists.

Outside the pin: linalgcpp's own operations (Mult, Transpose, CooMatrix::ToSparse,
the readers) are graph-embed_amd/compat/'s on both sides, so P^T A P keeps its
dense-definition test (tests/test_oracle.py); mergeLeaves=true, which the library
declares and rejects; the numParts / single-P_T partition overloads, which neither
the oracle nor the library implements (they are only run for validity here).
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

import ge_amd as ge
import graphs as G
import ref_cases as C
import ref_lib as R

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "graph-embed_amd")


@pytest.fixture(scope="module")
def ref():
    if not R.available():  # raises where the tree is present and the build fails
        pytest.skip("neither the reference tree nor a built oracle/_ref/ge_ref is here")
    return R


@pytest.fixture(scope="module")
def man():
    return C.manifest()


def same(a, b):
    """Bitwise equal, NaN == NaN (one-member aggregates of the minimizer)."""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def test_reference_builds_where_its_tree_is():
    """No skip where the reference tree exists: the binary must build there."""
    if R.tree_present():
        assert R.available()
        info = R.build_info()
        assert "-ffp-contract=off" in info["flags"] and "-O2" in info["flags"]


# --------------------------------------------------------------------------
# committed fixtures

@pytest.mark.parametrize("name", list(C.FA_CASES))
def test_fixture_force_atlas(oracle, man, name):
    case = C.fa_case(name)
    assert C.input_hashes(case) == man["cases"][name]["inputs"]  # generator drift, not parity
    want = C.load(name)["x"]
    assert np.array_equal(C.run_fa(oracle.force_atlas, case), want)
    if case["x0"] is not None and name in ("F1_d3", "F3"):  # thread count does not matter
        assert np.array_equal(C.run_fa(lambda *a, **k: oracle.force_atlas(*a, nthreads=8, **k),
                                       case), want)


@pytest.mark.parametrize("name", list(C.ML_CASES))
def test_fixture_force_atlas_ml(oracle, man, name):
    case = C.ml_case(name)
    entry = man["cases"][name]
    assert C.input_hashes(case) == entry["inputs"]
    if name in C.ML_QUIRK:  # the local/global index quirk is exercised (ref_cases.py)
        assert entry["local_global_edges"] > 0
        if name == "M1":
            assert C.local_global_edges(case["A"], case["PT"]) == entry["local_global_edges"]
    assert np.array_equal(C.run_ml(oracle.force_atlas_ml, case), C.load(name)["x"])


@pytest.mark.parametrize("name", C.P_NAMES)
def test_fixture_partition(oracle, man, name):
    case = C.p_case(name)
    assert C.input_hashes(case) == man["cases"]["P_" + name]["inputs"]
    g = C.load("P_" + name)
    kw = case["kw"]
    host_kw = {{"matching": "matching_iterations"}.get(k, k): v for k, v in kw.items()}
    for cf in C.P_CFS:
        want = C.hier_from(g, "cf" + C.cf_key(cf))
        assert len(want) >= 1
        assert C.same_hier(oracle.partition(case["A"], cf, **kw), want), cf
        assert C.same_hier(oracle.partition(case["A"], cf, flat=True, **kw), want), cf
        assert C.same_hier(ge.partition(case["A"], cf, **host_kw), want), cf


def test_fixture_modularity(oracle, man):
    A = C.p_graph("rmat")
    g = C.load("P_rmat")
    checked = 0
    for cf in C.P_CFS:
        hier = C.hier_from(g, "cf" + C.cf_key(cf))
        want = [float.fromhex(h) for h in man["cases"]["P_rmat"]["modularity"][C.cf_key(cf)]]
        for Al, PT, q in zip(oracle.hierarchy_As(A, hier), hier, want):
            vA = C.vertex_of(PT)
            assert oracle.modularity(Al, vA, PT[2]) == q
            assert ge.modularity(Al, vA, PT[2]) == q
            checked += 1
    assert checked >= 3


def test_fixture_embed_and_its_modularity(oracle, man):
    A = C.e_graph()
    g = C.load("E")
    entry = man["cases"]["E"]
    hier = C.hier_from(g, "h")
    assert C.same_hier(oracle.partition(A, C.E_CF), hier)
    assert C.same_hier(ge.partition(A, C.E_CF), hier)
    As = oracle.hierarchy_As(A, hier)
    assert C.input_hashes({"As": As}) == entry["inputs"]
    for Al, PT, h in zip(As, hier, entry["modularity"]):
        assert oracle.modularity(Al, C.vertex_of(PT), PT[2]) == float.fromhex(h)
        assert ge.modularity(Al, C.vertex_of(PT), PT[2]) == float.fromhex(h)
    for d in C.E_DIMS:  # the reference's own 100000 / 100 iterations
        X = oracle.embed(As, hier, d, seed=entry["seed"], nthreads=1)
        assert np.array_equal(X, g[f"x_d{d}"]), d


def test_fixtures_fresh(ref, man):
    """Two cheap fixtures re-derived from the live binary equal the committed files,
    and the binary is built from the files and flags the manifest records."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_ref_fixtures as M
    for name in ("F1_d2", "F1_d3", "P_rmat"):
        arrays, entry = M.derive(name)
        assert entry == man["cases"][name]
        g = C.load(name)
        assert set(arrays) == set(g)
        for k, v in arrays.items():
            assert np.array_equal(v, g[k]), (name, k)
    if R.tree_present():
        assert R.build_info() == man["build"]


# --------------------------------------------------------------------------
# live: forceAtlas

def _weighted_graph(n=60, seed=4, self_loops=True):
    """Symmetric fractional weights, self-loops on every 7th vertex, one isolated vertex."""
    ip, ix, dx = G.erdos_renyi(n, 0.12, seed=seed)
    A = C.symmetric_weights((ip, ix, dx))
    rows = []
    for i in range(n):
        seg = list(zip(ix[ip[i]:ip[i + 1]].tolist(), A[2][ip[i]:ip[i + 1]].tolist()))
        seg = [(c, w) for c, w in seg if c != n - 1 and i != n - 1]  # isolate the last vertex
        if self_loops and i % 7 == 0:
            seg.append((i, 2.5))
        rows.append(sorted(seg))
    nip = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    nix = np.array([c for r in rows for c, _ in r], np.int32)
    ndx = np.array([w for r in rows for _, w in r], np.float64)
    assert nip[n] == nip[n - 1]
    return nip, nix, ndx


FA_FLIPS = dict(ks=0.2, ksmax=0.05, repel=1.5, attract=0.7, gravity=2.0, use_weights=0, linlog=1,
                nohubs=1, delta=2.0, tolerate=0.5, normalize=1)


def _option_sets(flips):
    sets = [{}] + [{k: v} for k, v in flips.items()]
    sets += [dict(p) for p in itertools.combinations(flips.items(), 2)]
    return sets


def test_live_force_atlas_options(oracle, ref):
    """Every option flipped alone and in pairs, plus delta = 0 and 0.5 (the other
    branches of include/forceatlas.hpp's delta test) on fractional weights."""
    A = _weighted_graph()
    X0 = G.random_coords(60, 2, seed=3)
    sets = _option_sets(FA_FLIPS) + [dict(delta=0.0), dict(delta=0.5), dict(delta=0.5, linlog=1)]
    assert len(sets) == 1 + 11 + 55 + 3
    bad = [kw for kw in sets
           if not np.array_equal(ref.force_atlas(A, 2, coords=X0, iterations=10, **kw),
                                 oracle.force_atlas(A, 2, coords=X0, iterations=10, **kw))]
    assert not bad, bad


def test_live_force_atlas_negative_weight_delta(oracle, ref):
    A = _weighted_graph(self_loops=False)
    ip, ix, dx = A
    dx = dx.copy()
    r, c = 0, int(ix[ip[0]])  # flip one edge's sign on both sides
    dx[ip[r]] = -dx[ip[r]]
    k = ip[c] + int(np.flatnonzero(ix[ip[c]:ip[c + 1]] == r)[0])
    dx[k] = -dx[k]
    X0 = G.random_coords(60, 3, seed=8)
    for kw in (dict(delta=2.0), dict(delta=0.5), {}):
        assert np.array_equal(ref.force_atlas((ip, ix, dx), 3, coords=X0, iterations=6, **kw),
                              oracle.force_atlas((ip, ix, dx), 3, coords=X0, iterations=6, **kw))


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_live_force_atlas_dims_and_starts(oracle, ref, dim):
    A = G.largest_component(G.rmat(300, 1500, seed=dim))
    n = len(A[0]) - 1
    X0 = G.random_coords(n, dim, seed=dim)
    assert np.array_equal(ref.force_atlas(A, dim, coords=X0, iterations=15),
                          oracle.force_atlas(A, dim, coords=X0, iterations=15))
    assert np.array_equal(ref.force_atlas(A, dim, iterations=15, seed=1000 + dim),
                          oracle.force_atlas(A, dim, iterations=15, seed=1000 + dim))


def test_live_force_atlas_coincident_isolated_and_single(oracle, ref):
    A = G.erdos_renyi(30, 0.05, seed=9)
    assert (np.diff(A[0]) == 0).any()
    X0 = G.random_coords(30, 2, seed=3)
    X0[5] = X0[6]  # distance clamped to epsilon
    X0[9] = 0.0    # magnitude clamped to epsilon
    assert same(ref.force_atlas(A, 2, coords=X0, iterations=10),
                oracle.force_atlas(A, 2, coords=X0, iterations=10))
    one = (np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0))
    x = np.array([[0.5, -0.25, 0.125]])
    assert same(ref.force_atlas(one, 3, coords=x, iterations=7),
                oracle.force_atlas(one, 3, coords=x, iterations=7))


def test_live_force_atlas_thread_count(ref):
    A = G.erdos_renyi(200, 0.05, seed=1)
    X0 = G.random_coords(200, 3)
    a = ref.force_atlas(A, 3, coords=X0, iterations=20, threads=1)
    b = ref.force_atlas(A, 3, coords=X0, iterations=20, threads=8)
    assert np.array_equal(a, b)


# --------------------------------------------------------------------------
# live: forceAtlasMultilevel

ML_FLIPS = {k: v for k, v in FA_FLIPS.items() if k != "normalize"}


def _ml_inputs(dim, weighted=True):
    sizes = [1, 2, 7, 40, 33, 70, 19]
    n = sum(sizes)
    A = G.submatrix(G.rmat(n, 8 * n, seed=5), np.arange(n))
    if weighted:
        A = C.symmetric_weights(A)
    PT = C.block_partition(n, sizes, seed=2)
    m = len(sizes)
    return (A, PT, C.vertex_of(PT), G.random_coords(m, dim, seed=m),
            np.random.RandomState(m).uniform(0.0, 0.6, m), dim)


def test_live_force_atlas_ml_options(oracle, ref):
    args = _ml_inputs(3)
    assert C.local_global_edges(args[0], args[1]) > 0
    sets = _option_sets(ML_FLIPS) + [dict(delta=0.0), dict(delta=0.5)]
    assert len(sets) == 1 + 10 + 45 + 2
    bad = [kw for kw in sets
           if not np.array_equal(ref.force_atlas_ml(*args, iterations=6, seed=23, **kw),
                                 oracle.force_atlas_ml(*args, iterations=6, seed=23, nthreads=1,
                                                       **kw))]
    assert not bad, bad


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_live_force_atlas_ml_dims(oracle, ref, dim):
    args = _ml_inputs(dim, weighted=False)
    want = ref.force_atlas_ml(*args, iterations=12, seed=77)
    assert np.array_equal(oracle.force_atlas_ml(*args, iterations=12, seed=77, nthreads=1), want)
    assert np.array_equal(oracle.force_atlas_ml(*args, iterations=12, seed=77, nthreads=8), want)


def test_live_force_atlas_ml_on_a_partition_level(oracle, ref):
    """Level 0 of a partition hierarchy, repel / attract default and 1.5 / 0.7."""
    A = G.largest_component(G.rmat(700, 4200, seed=5))
    PT = ref.partition(A, cf=0.125)[0]
    vA = C.vertex_of(PT)
    cA = G.random_coords(PT[2], 3, seed=11)
    rA = np.random.RandomState(3).uniform(0.1, 0.5, PT[2])
    for kw in ({}, dict(repel=1.5, attract=0.7)):
        assert np.array_equal(
            ref.force_atlas_ml(A, PT, vA, cA, rA, 3, iterations=12, seed=9, **kw),
            oracle.force_atlas_ml(A, PT, vA, cA, rA, 3, iterations=12, seed=9, nthreads=1, **kw))


# --------------------------------------------------------------------------
# live: partition, interpolation, modularity

@pytest.mark.parametrize("kw", [dict(), dict(positive_merging=False), dict(stall=0.9),
                                dict(matching=1), dict(matching=4, stall=0.95),
                                dict(positive_merging=False, matching=3)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "default")
def test_live_partition_options(oracle, ref, kw):
    host_kw = {{"matching": "matching_iterations"}.get(k, k): v for k, v in kw.items()}
    graphs = [G.largest_component(G.rmat(900, 5000, seed=6)),
              C.symmetric_weights(G.erdos_renyi(500, 0.02, seed=2))]
    for A in graphs:
        for cf in (0.05, 0.3):
            want = ref.partition(A, cf=cf, **kw)
            assert len(want) >= 1
            assert C.same_hier(oracle.partition(A, cf, **kw), want)
            assert C.same_hier(oracle.partition(A, cf, flat=True, **kw), want)
            assert C.same_hier(ge.partition(A, cf, **host_kw), want)
            As = oracle.hierarchy_As(A, want)
            for Al, PT in zip(As, want):
                q = ref.modularity(Al, PT)
                assert oracle.modularity(Al, C.vertex_of(PT), PT[2]) == q
                assert ge.modularity(Al, C.vertex_of(PT), PT[2]) == q


def test_live_partition_other_overloads_are_partitions(ref):
    """partition(A, numParts, ...) and partition(A, ...) -> one P_T: outside the
    oracle's and the library's scope (they reject them), run here for validity
    only: every vertex in exactly one aggregate."""
    A = G.largest_component(G.rmat(600, 3000, seed=3))
    n = len(A[0]) - 1
    for kw in (dict(num_parts=40), dict()):
        (PT,) = ref.partition(A, **kw)
        assert PT[3] == n and np.array_equal(np.sort(PT[1]), np.arange(n))
        assert 1 <= PT[2] < n


def test_live_interpolation_matrix(ref):
    sets = [[4, 1], [0], [5, 2, 3], [6]]
    want = ref.interpolation_matrix(7, sets)
    got = ge.interpolation_matrix(7, sets)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------
# live: embed, embedViaMinimization, Laplacian helpers

@pytest.mark.parametrize("dim", [2, 3])
def test_live_embed(oracle, ref, dim):
    A = G.largest_component(G.rmat(500, 2600, seed=8))
    hier = ref.partition(A, cf=0.2)
    assert len(hier) >= 2  # radius step in both branches and prolongation
    As = oracle.hierarchy_As(A, hier)
    want = ref.embed(As, hier, dim, seed=21)
    assert np.array_equal(oracle.embed(As, hier, dim, seed=21, nthreads=1), want)


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_live_embed_via_minimization(oracle, ref, dim):
    A = G.largest_component(G.rmat(150, 600, seed=dim))
    n = len(A[0]) - 1
    X0 = G.random_coords(n, dim, seed=1)
    want = ref.embed_via_minimization(A, dim, coords=X0, iterations=6)
    assert same(oracle.embed_via_minimization(A, dim, coords=X0, iterations=6), want)
    assert same(ge.embed_via_minimization(A, dim, coords=X0, iterations=6), want)
    want = ref.embed_via_minimization(A, dim, iterations=5, seed=17)  # seeded start
    assert same(oracle.embed_via_minimization(A, dim, iterations=5, seed=17), want)
    assert same(ge.embed_via_minimization(A, dim, iterations=5, seed=17), want)


def test_live_embed_via_minimization_default_overload(oracle, ref):
    A = G.largest_component(G.rmat(60, 200, seed=2))
    n = len(A[0]) - 1
    want = ref.embed_via_minimization(A, 2, coords="default")  # zero start, 1000 sweeps
    assert same(oracle.embed_via_minimization(A, 2, coords=np.zeros((n, 2)), iterations=1000),
                want)


def test_live_embed_via_minimization_multilevel(oracle, ref):
    """embedVia(As, P_Ts, 2, anyToMultilevel(embedViaMinimization)); a one-member
    aggregate is placed at c + r * (0 / 0) = NaN on both sides."""
    A = G.largest_component(G.rmat(400, 2000, seed=4))
    hier = ref.partition(A, cf=0.2)
    As = oracle.hierarchy_As(A, hier)
    want = ref.embed_via_minimization_ml(As, hier, 2, seed=5)
    got = oracle.embed_via_minimization_ml(As, hier, 2, seed=5, nthreads=1)
    assert same(got, want), int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())


@pytest.mark.parametrize("self_loops", [False, True])
def test_live_laplacian_helpers(ref, tmp_path, self_loops):
    """The drop-in identity / toLaplacian / fromLaplacian against src/matrixutils.cpp."""
    exe = str(tmp_path / "lap")
    subprocess.check_call(["g++", "-std=c++14", "-O2", f"-I{PKG}/include", f"-I{PKG}/compat",
                           os.path.join(HERE, "cpp", "laplacian.cpp"), "-o", exe])
    A = _weighted_graph(n=80, seed=6, self_loops=self_loops)
    R.write_csr(str(tmp_path / "a.bin"), A)
    subprocess.check_call([exe, str(tmp_path / "a.bin"), str(tmp_path / "o.bin")])
    with open(tmp_path / "o.bin", "rb") as f:
        got = R.read_csrs(f.read(), 3)
    for g, w in zip(got, ref.laplacian(A)):
        for a, b in zip(g, w):
            assert np.array_equal(a, b)
