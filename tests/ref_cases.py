"""The cases recorded from the reference binary (tests/golden/make_ref_fixtures.py
writes tests/golden/ref_*.npz and ref_manifest.json from them) and replayed by
tests/test_reference.py (oracle, host library) and tests/test_gpu_reference.py
(device paths).  Inputs are rebuilt from tests/graphs.py; the manifest holds a
sha256 of every input array so that generator drift shows up as a hash mismatch
and not as a parity failure.

Shapes are the smallest at which each device path is still selected -- the
shapes of the oracle-based tests in tests/test_gpu_parity.py.
"""
import functools
import hashlib
import json
import os

import numpy as np

import graphs as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "ref_manifest.json")


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def _canon(A):
    return (np.ascontiguousarray(A[0], np.int32), np.ascontiguousarray(A[1], np.int32),
            np.ascontiguousarray(A[2], np.float64))


def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"ref_{name}.npz"), allow_pickle=False))


def input_hashes(case):
    """sha256 of every array of a case dict (CSR triples and (indptr, indices) pairs by part)."""
    out = {}
    for k, v in sorted(case.items()):
        if isinstance(v, tuple) and v and isinstance(v[0], np.ndarray):
            for part, a in zip(("ip", "ix", "dx"), v):
                out[f"{k}_{part}"] = sha(a)
        elif isinstance(v, np.ndarray):
            out[k] = sha(v)
        elif isinstance(v, list) and v and isinstance(v[0], tuple):
            for l, M in enumerate(v):
                for part, a in zip(("ip", "ix", "dx"), M[:3]):
                    if isinstance(a, np.ndarray):
                        out[f"{k}{l}_{part}"] = sha(a)
    return out


def symmetric_weights(A):
    """Fractional weights from a few values, equal on (i, j) and (j, i)."""
    ip, ix, _ = A
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    w = 1.0 + ((np.minimum(rows, ix) * 7 + np.maximum(rows, ix) * 13) % 3) * 0.5
    return ip, ix, w


# --------------------------------------------------------------------------
# single-level forceAtlas: name -> dict(A, dim, x0 | None, iterations, seed, kw)

NONDEFAULT = dict(ks=0.2, ksmax=2.0, repel=1.5, attract=0.7, gravity=2.0, use_weights=0,
                  tolerate=0.5)  # test_fa_nondefault_params


def _fa(A, dim, x0, iterations, seed=0, **kw):
    return dict(A=_canon(A), dim=dim, x0=x0, iterations=iterations, seed=seed, kw=kw)


def _f1(dim):
    return _fa(G.erdos_renyi(97, 0.06, seed=dim), dim, G.random_coords(97, dim, seed=dim), 30)


def _f4():
    A = G.with_degrees(G.rmat(4500, 22500, seed=4500), {17: 700}, seed=1)
    X0 = G.random_coords(4500, 3, seed=1)
    X0[2500, 0] = 1e-70  # outside the exact-division domain: the general bodies
    return _fa(A, 3, X0, 3)


def _f5():
    A = G.with_degrees(G.rmat(3000, 12000, seed=3),
                       {7: 1023, 8: 1024, 9: 1025, 300: 700, 11: 2600}, seed=3)
    deg = np.diff(A[0])
    assert list(deg[[7, 8, 9, 300, 11]]) == [1023, 1024, 1025, 700, 2600] and (deg == 0).any()
    return _fa(A, 3, G.random_coords(3000, 3, seed=3), 3)


def _f6(iterations, weighted=False, **kw):
    A = G.erdos_renyi(1500, 0.004, seed=5)
    if weighted:
        A = symmetric_weights(A)
    return _fa(A, 3, G.random_coords(1500, 3, seed=2), iterations, **kw)


def _f7():
    A = G.largest_component(G.rmat(200, 900, seed=5))
    return _fa(A, 2, None, 20, seed=4242)


FA_CASES = {
    "F1_d2": lambda: _f1(2),
    "F1_d3": lambda: _f1(3),
    "F2": lambda: _fa(G.rmat(300, 1800, seed=303), 3, G.random_coords(300, 3, seed=300), 200),
    "F3": lambda: _fa(G.rmat(700, 4200, seed=700), 3, G.random_coords(700, 3, seed=1), 4),
    "F4": _f4,
    "F5": _f5,
    "F6_nondefault": lambda: _f6(4, **NONDEFAULT),
    "F6_nohubs_normalize": lambda: _f6(3, nohubs=1, normalize=1, use_weights=0),
    "F7": _f7,
    # device log / pow differ from glibc in the last place: compared with rtol 1e-12
    # after one iteration.  delta acts on the weights, so those two carry fractional ones.
    "F8_linlog": lambda: _f6(1, linlog=1),
    "F8_delta": lambda: _f6(1, weighted=True, delta=2.0),
    "F8_linlog_delta": lambda: _f6(1, weighted=True, linlog=1, delta=2.0),
}
FA_TOLERANT = ("F8_linlog", "F8_delta", "F8_linlog_delta")


@functools.lru_cache(maxsize=None)
def fa_case(name):
    return FA_CASES[name]()


def run_fa(force_atlas, case):
    """force_atlas: oracle_lib.force_atlas, ref_lib.force_atlas or Context.force_atlas."""
    return force_atlas(case["A"], case["dim"], coords=case["x0"], iterations=case["iterations"],
                       seed=case["seed"], **case["kw"])


# --------------------------------------------------------------------------
# forceAtlasMultilevel: name -> dict(A, PT, vA, cA, rA, dim, iterations, seed, kw)

def block_partition(n, sizes, seed=0):
    """P_T with aggregates of the given sizes over a random permutation of 0..n-1,
    members listed ascending (as the partitioner emits them)."""
    assert sum(sizes) == n
    perm = np.random.RandomState(seed).permutation(n)
    ip = np.cumsum([0] + list(sizes)).astype(np.int32)
    ix = np.concatenate([np.sort(perm[ip[a]:ip[a + 1]]) for a in range(len(sizes))])
    return ip, ix.astype(np.int32)


def vertex_of(PT):
    v = np.empty(len(PT[1]), dtype=np.int32)
    v[PT[1]] = np.repeat(np.arange(len(PT[0]) - 1, dtype=np.int32), np.diff(PT[0]))
    return v


def local_global_edges(A, PT):
    """Edges (v[i], j) inside an aggregate whose global id j equals the local index
    i of the row's vertex: forceAtlasMultilevel's attraction tests `j != i` with j
    global and i local (include/forceatlas.hpp:417), so such an edge takes the
    external branch.  The oracle and the kernels keep that on purpose."""
    ip, ix = A[0], A[1]
    vA = vertex_of(PT)
    count = 0
    for a in range(len(PT[0]) - 1):
        v = PT[1][PT[0][a]:PT[0][a + 1]]
        for i, g in enumerate(v):
            row = ix[ip[g]:ip[g + 1]]
            count += int(((row == i) & (vA[row] == a)).sum())
    return count


def _ml(A, sizes, pt_seed, dim, iterations, seed, **kw):
    n, m = sum(sizes), len(sizes)
    PT = block_partition(n, sizes, seed=pt_seed)
    return dict(A=_canon(A), PT=PT, vA=vertex_of(PT), cA=G.random_coords(m, dim, seed=m),
                rA=np.random.RandomState(m).uniform(0.0, 0.6, m), dim=dim,
                iterations=iterations, seed=seed, kw=kw)


M1_SIZES = [1, 2, 3, 5, 8, 13, 21, 34, 64, 9, 65, 100, 256, 200]
M2_SIZES = [2600, 320, 700, 257, 1031, 300, 90, 1]
M3_SIZES = [5000, 300, 40, 1]


def _m1():
    n = sum(M1_SIZES)
    return _ml(G.submatrix(G.rmat(n, 6 * n, seed=len(M1_SIZES)), np.arange(n)), M1_SIZES, n, 3,
               12, 31)


def _m2(dim, repel):
    n = sum(M2_SIZES)
    A = G.with_hubs(G.rmat(n, 10 * n, seed=11), [(3, 2000), (70, 3000)], seed=dim)
    return _ml(A, M2_SIZES, 5, dim, 6, 19, repel=repel)


def _m3():
    n = sum(M3_SIZES)
    return _ml(G.submatrix(G.rmat(n, 6 * n, seed=len(M3_SIZES)), np.arange(n)), M3_SIZES, n, 3,
               4, 31)


# --------------------------------------------------------------------------
# The multilevel layouts of tests/test_gpu_faml_paths.py: one per size class of
# faml_plan_build (ge_faml.hip), fractional weights, and the domain-edge inputs.

LARGE_SIZES = [1031, 700, 257, 90]  # LDS-resident one per block under GE_FAML_RES_CAP=4096
LAYOUTS = {
    # name: (sizes, P_T permutation seed, GE_FAML_RES_CAP or None)
    "packed": (M1_SIZES, sum(M1_SIZES), None),
    "large": (LARGE_SIZES, 7, "4096"),
    "streamed": (M2_SIZES, 5, "256"),
}
ML_OPTIONS = dict(ks=0.2, ksmax=0.05, repel=1.5, attract=0.7, gravity=2.0, tolerate=0.5)
TINY = 1e-70  # outside coord_ok (ge_math.hpp: |x| in [2^-200, 2^200] or 0)
HUGE_W = 2.0 ** 61  # deg + 1 above weight_ok's 2^60


@functools.lru_cache(maxsize=None)
def layout_graph(layout):
    """The unit-weight graph of a layout."""
    sizes = LAYOUTS[layout][0]
    n = sum(sizes)
    if layout == "packed":  # M1's graph
        return _canon(G.submatrix(G.rmat(n, 6 * n, seed=len(sizes)), np.arange(n)))
    if layout == "large":
        return _canon(G.rmat(n, 8 * n, seed=4))
    # M2's graph: two hub rows longer than a row tile (512 entries)
    return _canon(G.with_hubs(G.rmat(n, 10 * n, seed=11), [(3, 2000), (70, 3000)], seed=3))


def ml_layout(layout, dim=3, iterations=3, seed=19, weighted=True, **kw):
    A = layout_graph(layout)
    if weighted:
        A = symmetric_weights(A)
    sizes, pt_seed, _ = LAYOUTS[layout]
    return _ml(A, sizes, pt_seed, dim, iterations, seed, **kw)


def internal_edges(case, a):
    """(i, j, e): CSR entries e of member rows of aggregate a whose column is a member too,
    as local member indices i < j."""
    ip, ix = case["A"][0], case["A"][1]
    PT, vA = case["PT"], case["vA"]
    v = PT[1][PT[0][a]:PT[0][a + 1]]
    local = {int(g): i for i, g in enumerate(v)}
    out = []
    for i, g in enumerate(v):
        for e in range(ip[g], ip[g + 1]):
            j = ix[e]
            if vA[j] == a and local[int(j)] > i:
                out.append((i, local[int(j)], e))
    return out


def internal_degree_plus_one(case, a):
    """deg + 1 of the members of aggregate a as forceAtlasMultilevel counts it
    (include/forceatlas.hpp:362-383, use_weights on): the weights of the row's entries
    whose column lies in a, added in CSR order."""
    ip, ix, dx = case["A"]
    PT, vA = case["PT"], case["vA"]
    out = []
    for g in PT[1][PT[0][a]:PT[0][a + 1]]:
        acc = 0.0
        for e in range(ip[g], ip[g + 1]):
            if vA[ix[e]] == a:
                acc += dx[e]
        out.append(acc + 1)
    return np.array(out)


def with_heavy_edges(case):
    """One internal edge per aggregate with weight 2^61 in both directions: exactly two
    members of the aggregate leave weight_ok(deg + 1), so fast and fallback tiles mix.
    In the largest aggregate the two lie in different 64-row tiles, one of them in the
    last tile (ragged where the size is no multiple of 64)."""
    ip, ix, dx = case["A"]
    dx = dx.copy()
    PT = case["PT"]
    sizes = np.diff(PT[0])
    for a in range(len(sizes)):
        edges = internal_edges(case, a)
        if a == int(np.argmax(sizes)) and sizes[a] > 64:
            last = (sizes[a] - 1) // 64
            edges = [t for t in edges if t[1] // 64 == last and t[0] // 64 != last]
            assert edges, "no internal edge into the last tile: change the permutation seed"
        if not edges:
            continue
        i, j, e = edges[0]
        gi, gj = PT[1][PT[0][a] + i], PT[1][PT[0][a] + j]
        back = ip[gj] + int(np.flatnonzero(ix[ip[gj]:ip[gj + 1]] == gi)[0])
        assert ix[e] == gj and ix[back] == gi
        dx[e] = dx[back] = HUGE_W
    return dict(case, A=(ip, ix, dx))


def with_scaled_weights(case, factor):
    ip, ix, dx = case["A"]
    return dict(case, A=(ip, ix, dx * factor))


# aggregates of each layout that take the coords_A edges: `tiny` get a 1e-70 component,
# `origin` sits at 0, the two of `same` share their coordinates, `zero_r` has r_A = 0
COARSE_EDGES = {
    "packed": dict(tiny=(12, 7), origin=11, same=(13, 8), zero_r=10),
    "large": dict(tiny=(0,), origin=3, same=(1, 2), zero_r=2),
    "streamed": dict(tiny=(0,), origin=6, same=(4, 2), zero_r=3),
}


def edges_between(case, a, b):
    ip, ix = case["A"][0], case["A"][1]
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    vA = case["vA"]
    return int(((vA[rows] == a) & (vA[ix] == b)).sum())


def with_coarse_edges(case, layout):
    spec = COARSE_EDGES[layout]
    cA, rA = case["cA"].copy(), case["rA"].copy()
    for q, a in enumerate(spec["tiny"]):
        cA[a, q % cA.shape[1]] = TINY
    cA[spec["origin"]] = 0.0
    cA[spec["same"][1]] = cA[spec["same"][0]]
    rA[spec["zero_r"]] = 0.0
    return dict(case, cA=cA, rA=rA)


# --------------------------------------------------------------------------
# the cases pinned to the reference itself

M6_D1_SIZES = [1000, 257, 256, 65, 64, 30, 1]
M6_D4_SIZES = [2048, 257, 65, 64, 1]  # the large kernel at its dim-4 capacity, resident side


def _m6(dim, sizes):
    n = sum(sizes)
    return _ml(symmetric_weights(G.rmat(n, 6 * n, seed=dim)), sizes, dim, dim, 3, 23)


ML_CASES = {
    "M1": _m1,
    "M2_d2": lambda: _m2(2, 1.0),
    "M2_d3": lambda: _m2(3, 1.0),
    "M2_d2_repel": lambda: _m2(2, 1.5),
    "M2_d3_repel": lambda: _m2(3, 1.5),
    "M3": _m3,
    "M4_options": lambda: ml_layout("large", **ML_OPTIONS),
    "M4_nohubs_unweighted": lambda: ml_layout("streamed", nohubs=1, use_weights=0),
    "M5_weight_edges": lambda: with_heavy_edges(ml_layout("streamed")),
    "M5_coarse_edges": lambda: with_coarse_edges(ml_layout("packed"), "packed"),
    "M6_d1": lambda: _m6(1, M6_D1_SIZES),
    "M6_d4": lambda: _m6(4, M6_D4_SIZES),
}
# the GE_FAML_RES_CAP each case's size classes need (None: the plan's own rule)
ML_RES_CAP = {"M4_options": "4096", "M4_nohubs_unweighted": "256", "M5_weight_edges": "256",
              "M6_d1": "4096", "M6_d4": "4096"}
ML_QUIRK = ("M1", "M2_d2", "M2_d3", "M2_d2_repel", "M2_d3_repel")  # must hold such an edge


@functools.lru_cache(maxsize=None)
def ml_case(name):
    return ML_CASES[name]()


def run_ml(force_atlas_ml, case):
    return force_atlas_ml(case["A"], case["PT"], case["vA"], case["cA"], case["rA"], case["dim"],
                          iterations=case["iterations"], seed=case["seed"], **case["kw"])


# --------------------------------------------------------------------------
# partition: the seven cases of test_partition_flat_equals_map at n <= 2000 ids

P_NAMES = ("rmat", "hubs", "er", "weights", "nopos", "stall", "match3")
P_CFS = (0.125, 0.4)
P_KW = {"nopos": dict(positive_merging=False), "stall": dict(stall=0.97),
        "match3": dict(matching=3)}


@functools.lru_cache(maxsize=None)
def p_graph(name):
    if name == "er":
        A = G.erdos_renyi(1500, 0.008, seed=3)
    elif name == "hubs":
        A = G.with_hubs(G.largest_component(G.rmat(2000, 13000, seed=8)), [(5, 1000), (9, 500)])
    else:
        A = G.largest_component(G.rmat(2000, 15000, seed=10))
    if name == "weights":
        A = symmetric_weights(A)
    return _canon(A)


def p_case(name):
    return dict(A=p_graph(name), kw=P_KW.get(name, {}))


def cf_key(cf):
    return str(cf).replace(".", "p")


def hier_arrays(prefix, hier):
    out = {f"{prefix}_levels": np.array(len(hier), np.int32)}
    for l, PT in enumerate(hier):
        out[f"{prefix}_P{l}_ip"] = np.asarray(PT[0], np.int32)
        out[f"{prefix}_P{l}_ix"] = np.asarray(PT[1], np.int32)
    return out


def hier_from(g, prefix):
    out = []
    for l in range(int(g[f"{prefix}_levels"])):
        ip, ix = g[f"{prefix}_P{l}_ip"], g[f"{prefix}_P{l}_ix"]
        out.append((ip, ix, len(ip) - 1, len(ix)))
    return out


def same_hier(a, b):
    return len(a) == len(b) and all(
        x[2:] == y[2:] and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        for x, y in zip(a, b))


# --------------------------------------------------------------------------
# embed and modularity

E_SEED = 6
E_DIMS = (2, 3)
E_CF = 0.125


@functools.lru_cache(maxsize=None)
def e_graph():
    return _canon(G.largest_component(G.rmat(700, 4000, seed=5)))
