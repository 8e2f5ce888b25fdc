"""The synthetic levels of the batched minimiser tests (tests/test_minimize_ml.py,
tests/test_gpu_minimize_ml.py) and of tests/golden/make_min_fixtures.py, which
records tests/golden/ref_min_*.npz from the reference binary.

One level = a graph A, a P_T whose member lists interleave (ascending ids, but no
aggregate is a contiguous range), vertex_A, coords_A and r_A.  Inside an
aggregate: a ring plus a few chords; across aggregates: random edges, which the
embedder must ignore.  The sizes sit on both sides of every class boundary of
ge_minimize_dev.hip: P = 16 is its packed threshold, 64 the chunk of the wave
class.  Everything is drawn from numpy RandomState with fixed seeds; the sha256 of
every level is asserted before use, so that generator drift shows up as a hash
mismatch and not as a parity failure.
"""
import functools
import hashlib
import os
import subprocess

import numpy as np

import graphs as G

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "graph-embed_amd")

P = 16  # kPackDefault of graph-embed_amd/csrc/ge_minimize_dev.hip

# (size, kind): "ring" ring + chords; "bare" no internal edge at all (ends all-NaN);
# "loner" member 0 has no internal neighbour (skipped, but seen by the others)
SMALL = [(1, "ring"), (2, "ring"), (3, "ring"), (P - 1, "ring"), (P, "ring"), (P + 1, "ring"),
         (4, "bare"), (6, "loner")]
FULL = SMALL + [(63, "ring"), (64, "ring"), (65, "ring"), (129, "ring")]
LEVELS = {"small": (SMALL, 11, 1000), "full": (FULL, 12, 8)}  # aggregates, seed, sweeps
DIMS = {"small": (2, 3), "full": (2, 3, 4)}

SHA = {
    "small": "84385dd4deb96ad8fec6138d3ffb38609427bb07e0dda767b79d7f426dbe1b74",
    "full": "33b73d5692bc2eb01e7baf2eb5cd971637965735739485cd06bffbb0c8feac17",
}


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def _build(spec, seed):
    rs = np.random.RandomState(seed)
    sizes = [s for s, _ in spec]
    n, m = sum(sizes), len(sizes)
    perm = rs.permutation(n)
    pip = np.cumsum([0] + sizes).astype(np.int32)
    members = [np.sort(perm[pip[a]:pip[a + 1]]) for a in range(m)]
    src, dst = [], []
    for v, (r, kind) in zip(members, spec):
        if kind == "bare" or r < 2:
            continue
        ring = v[1:] if kind == "loner" else v
        k = len(ring)
        for i in range(k if k > 2 else k - 1):
            src.append(ring[i])
            dst.append(ring[(i + 1) % k])
        for _ in range(k // 4):  # chords
            i, j = rs.randint(0, k, 2)
            if i != j:
                src.append(ring[i])
                dst.append(ring[j])
    vA = np.empty(n, dtype=np.int32)
    for a, v in enumerate(members):
        vA[v] = a
    bare = {a for a, (_, kind) in enumerate(spec) if kind == "bare"}
    loners = {int(members[a][0]) for a, (_, kind) in enumerate(spec) if kind == "loner"}
    cross = 0
    while cross < n:  # cross-aggregate edges; the bare aggregate and the loner get some too
        i, j = (int(x) for x in rs.randint(0, n, 2))
        if vA[i] != vA[j]:
            src.append(i)
            dst.append(j)
            cross += 1
    for a in bare:
        assert any(vA[s] == a or vA[d] == a for s, d in zip(src, dst))
    # one self-loop, on the second member of the largest aggregate
    loop = int(members[int(np.argmax(sizes))][1])
    src.append(loop)
    dst.append(loop)
    A = G.csr_from_edges(n, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64))
    ip, ix = A[0], A[1]
    assert loop in ix[ip[loop]:ip[loop + 1]]
    assert all(vA[j] != vA[g] for g in loners for j in ix[ip[g]:ip[g + 1]])
    PT = (pip, np.concatenate(members).astype(np.int32))
    return dict(A=A, PT=PT, vA=vA, m=m, n=n, sizes=sizes,
                cA={d: rs.uniform(-1.0, 1.0, size=(m, d)) for d in (2, 3, 4)},
                rA=rs.uniform(0.1, 0.6, m))


def level_sha(lv):
    return _sha([lv["A"][0], lv["A"][1], lv["PT"][0], lv["PT"][1], lv["vA"], lv["rA"]]
                + [lv["cA"][d] for d in (2, 3, 4)])


@functools.lru_cache(maxsize=None)
def level(name):
    spec, seed, sweeps = LEVELS[name]
    lv = _build(spec, seed)
    lv["iterations"] = sweeps
    assert level_sha(lv) == SHA[name], (name, level_sha(lv))
    return lv


def sub_pattern(lv, a):
    """Aggregate a's internal edges as an r x r CSR pattern over local member indices
    (columns ascending; the self-loop stays, the embedder skips it)."""
    ip, ix = lv["A"][0], lv["A"][1]
    v = lv["PT"][1][lv["PT"][0][a]:lv["PT"][0][a + 1]]
    local = {int(g): i for i, g in enumerate(v)}
    sip, six = [0], []
    for g in v:
        six += sorted(local[int(j)] for j in ix[ip[g]:ip[g + 1]] if lv["vA"][j] == a)
        sip.append(len(six))
    return np.array(sip, dtype=np.int32), np.array(six, dtype=np.int32)


def place(lv, a, dim, nc):
    """anyToMultilevel's normalisation and placement (src/embed.cpp:67-79) of one
    aggregate's embedding nc, in the reference's operation order: the largest norm
    (magnitude: an ordered sum of squares, then sqrt), x / max, r_A * that, coords_A
    + that.  Python floats and numpy fp64 are IEEE and unfused."""
    mx = 0.0
    for row in nc:
        acc = 0.0
        for x in row:
            acc += float(x) * float(x)
        mg = float(np.sqrt(acc))
        if mg > mx:
            mx = mg
    with np.errstate(invalid="ignore", divide="ignore"):
        return lv["cA"][dim][a] + lv["rA"][a] * (nc / mx)


def compose(lv, dim, iterations, embed):
    """The level as the drop-in header composes it: embed(sub-pattern, dim, zeros,
    iterations) per aggregate, then place()."""
    X = np.zeros((lv["n"], dim))
    for a in range(lv["m"]):
        v = lv["PT"][1][lv["PT"][0][a]:lv["PT"][0][a + 1]]
        sub = sub_pattern(lv, a)
        nc = embed((sub[0], sub[1], np.ones(len(sub[1]))), dim, np.zeros((len(v), dim)),
                   iterations)
        X[v] = place(lv, a, dim, nc)
    return X


def same(a, b):
    """Bitwise equal values, NaNs at the same positions (sign and payload not compared)."""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# the end-to-end case: the hierarchy of tests/test_reference.py::
# test_live_embed_via_minimization_multilevel
E2E = dict(n=400, draws=2000, graph_seed=4, cf=0.2, dim=2, seed=5)


@functools.lru_cache(maxsize=None)
def e2e_graph():
    A = G.largest_component(G.rmat(E2E["n"], E2E["draws"], seed=E2E["graph_seed"]))
    return (np.ascontiguousarray(A[0], np.int32), np.ascontiguousarray(A[1], np.int32),
            np.ascontiguousarray(A[2], np.float64))


# (level, dim) of every recorded fixture array
CASES = [(name, dim) for name in LEVELS for dim in DIMS[name]]


def build_driver(tmp_path):
    exe = str(tmp_path / "minimize_ml_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "minimize_ml_driver.cpp"), f"-L{PKG}/lib",
                           "-lge", f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    return exe


def run_level(lv, dim, iterations=None, ctx=None, **kw):
    import ge_amd
    return ge_amd.embed_via_minimization_ml(
        lv["A"], lv["PT"], lv["vA"], lv["cA"][dim], lv["rA"], dim,
        iterations=lv["iterations"] if iterations is None else iterations, ctx=ctx, **kw)
