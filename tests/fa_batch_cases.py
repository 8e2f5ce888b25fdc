"""Inputs of the batched single-level forceAtlas tests (tests/test_fa_batch_cases.py,
tests/test_gpu_fa_batch.py): many small graphs whose sizes sit on every edge of
fa_batch_schedule (graph-embed_amd/csrc/ge_fa_sched.hpp), the hand-written class table
for them, and a numpy restatement of anyToMultilevel's sub-matrix extraction and
placement (src/embed.cpp:23-83) for the multilevel form.

size          what it is the edge of
1 2 3 4 5     the smallest graphs; lane-group boundary at 4 / 5
7 8 9         lane-group boundary at 8
16 17         lane-group boundary at 16
31 32 33      lane-group boundary at 32
63 64 65      wave / block edge
127 256 257   block class; 257 is serial at d >= 5
512 513       block / serial edge at d <= 4
"""
import functools

import numpy as np

import graphs as G

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 256, 257, 512, 513)
KINDS = ("path", "star", "clique", "rmat")
ITERATIONS = 300
WAVE, BLOCK, SERIAL = 0, 1, 2

# (class, lanes per row) per size, written out by hand from the rule of include/ge.h:
# wave up to 64 rows with the largest power of two of lanes that keeps n G <= 64; block
# up to 512 rows (256 on the wide schedule) with small_group's lanes for the general
# kernel's 512 (wide: 256) threads, i.e. doubled while n G 2 <= T; serial beyond.
_WAVE = {1: 64, 2: 32, 3: 16, 4: 16, 5: 8, 7: 8, 8: 8, 9: 4, 16: 4, 17: 2, 31: 2, 32: 2, 33: 1,
         63: 1, 64: 1}
TABLE = {
    # d = 3, STRICT: T = 512
    (3, "strict"): {**{n: (WAVE, g) for n, g in _WAVE.items()},
                    65: (BLOCK, 4), 127: (BLOCK, 4), 256: (BLOCK, 2), 257: (BLOCK, 1),
                    512: (BLOCK, 1), 513: (SERIAL, 0)},
    # d = 3, FAST: ge_force_atlas leaves the one-workgroup kernel, so does the batch
    (3, "fast"): {n: (SERIAL, 0) for n in SIZES},
    # d = 8 runs the exact kernels in both modes: T = 256, at most 256 rows
    (8, "strict"): {**{n: (WAVE, g) for n, g in _WAVE.items()},
                    65: (BLOCK, 2), 127: (BLOCK, 2), 256: (BLOCK, 1), 257: (SERIAL, 0),
                    512: (SERIAL, 0), 513: (SERIAL, 0)},
}
TABLE[(8, "fast")] = TABLE[(8, "strict")]


def _edges(n, kind, seed):
    if kind == "path":
        i = np.arange(n - 1)
        return i, i + 1
    if kind == "star":
        return np.zeros(n - 1, dtype=np.int64), np.arange(1, n)
    if kind == "clique":
        i, j = np.triu_indices(n, 1)
        return i, j
    s, d = G.rmat_edges(n, 3 * n, seed)
    return s, d


def graph(n, kind, seed, isolated=False, self_entry=False, weights=False):
    """A symmetric CSR graph of n vertices.  isolated: the last vertex has no entry;
    self_entry: vertex 0 has one on itself; weights: symmetric non-unit weights."""
    m = n - 1 if isolated and n > 2 else n
    if kind == "clique" and m > 64:
        kind = "rmat"  # n^2 entries are not what a large case is about
    src, dst = _edges(m, kind, seed) if m > 1 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    ip, ix, dx = G.csr_from_edges(n, np.asarray(src, np.int64), np.asarray(dst, np.int64))
    if self_entry:
        row = np.concatenate([[0], ix[ip[0]:ip[1]]]).astype(np.int32)
        ix = np.concatenate([row, ix[ip[1]:]]).astype(np.int32)
        dx = np.ones(len(ix))
        ip = ip.copy()
        ip[1:] += 1
    if weights:  # symmetric: a function of the unordered pair
        rows = np.repeat(np.arange(n), np.diff(ip))
        lo, hi = np.minimum(rows, ix), np.maximum(rows, ix)
        dx = np.array([0.5, 1.5, 2.25, 0.125])[(lo * 7 + hi * 13 + seed) % 4]
    return (np.ascontiguousarray(ip, np.int32), np.ascontiguousarray(ix, np.int32),
            np.ascontiguousarray(dx, np.float64))


@functools.lru_cache(maxsize=None)
def cases():
    """One graph per size of SIZES, the kinds in turn; every third one has an isolated
    vertex, every fourth a self entry, every second non-unit weights."""
    out = []
    for k, n in enumerate(SIZES):
        out.append(graph(n, KINDS[k % 4], seed=100 + k, isolated=k % 3 == 2,
                         self_entry=k % 4 == 1, weights=k % 2 == 1))
    return tuple(out)


def sizes_entries(graphs):
    return ([len(A[0]) - 1 for A in graphs], [len(A[1]) for A in graphs])


def start(graphs, dim, seed=5):
    """Initial coordinates per graph, U(-1, 1) from one numpy stream."""
    rs = np.random.RandomState(seed)
    return [rs.uniform(-1.0, 1.0, size=(len(A[0]) - 1, dim)) for A in graphs]


def same(a, b, nan_ok=False):
    """Bitwise-equal values; with nan_ok, NaNs at the same positions count as equal."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    eq = a == b
    if nan_ok:
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(eq.all())


# ---- the multilevel form ----------------------------------------------------------

def sub_matrix(A, PT, vA, a):
    """Aggregate a's r x r sub-matrix as anyToMultilevel builds it (src/embed.cpp:33-62,
    CooMatrix::ToSparse): 1.0 per stored entry of A between members, duplicates summed,
    self entries kept, rows in P_T order, columns ascending by position in the P_T row.
    The weights of A are not read."""
    ip, ix = np.asarray(A[0]), np.asarray(A[1])
    v = np.asarray(PT[1])[PT[0][a]:PT[0][a + 1]]
    local = {int(g): i for i, g in enumerate(v)}
    sip, six, sdx = [0], [], []
    for g in v:
        cols = sorted(local[int(j)] for j in ix[ip[g]:ip[g + 1]] if vA[j] == a)
        for q, c in enumerate(cols):
            if q and c == cols[q - 1]:
                sdx[-1] += 1.0
            else:
                six.append(c)
                sdx.append(1.0)
        sip.append(len(six))
    return (np.array(sip, dtype=np.int32), np.array(six, dtype=np.int32),
            np.array(sdx, dtype=np.float64))


def place(cA_a, rA_a, nc):
    """src/embed.cpp:66-82 in the reference's operation order: the largest magnitude (an
    ordered sum of squares, then sqrt), x / max, r_A * that, coords_A + that.  One member
    at the origin of its own layout divides 0 by 0, as the reference does."""
    mx = 0.0
    for row in nc:
        acc = 0.0
        for x in row:
            acc += float(x) * float(x)
        mg = float(np.sqrt(acc))
        if mg > mx:
            mx = mg
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(cA_a) + rA_a * (np.asarray(nc) / mx)


def ml_compose(A, PT, vA, cA, rA, dim, embed):
    """anyToMultilevel(embed) on one level: embed(sub-matrix, dim) per aggregate."""
    X = np.zeros((len(A[0]) - 1, dim))
    for a in range(len(PT[0]) - 1):
        v = np.asarray(PT[1])[PT[0][a]:PT[0][a + 1]]
        X[v] = place(cA[a], rA[a], embed(sub_matrix(A, PT, vA, a), dim))
    return X


@functools.lru_cache(maxsize=None)
def ml_level():
    """An R-MAT graph and a P_T whose aggregates span 1..70 members: interleaved member
    lists (no aggregate is a contiguous range, none is sorted), one aggregate of one
    member and one whose members share no edge."""
    n = 400
    A = G.largest_component(G.rmat(n, 2400, seed=21))
    n = len(A[0]) - 1
    rs = np.random.RandomState(22)
    want = [1, 2, 3, 5, 8, 9, 17, 33, 64, 65, 70]
    sizes = want + [4] * ((n - sum(want) - 6) // 4)
    sizes.append(n - sum(sizes) - 6)
    perm = rs.permutation(n)
    ip, ix = A[0], A[1]
    # six vertices no two of which share an entry: the aggregate without internal edges
    bare = []
    for g in perm:
        if len(bare) < 6 and all(int(j) not in bare for j in ix[ip[g]:ip[g + 1]]):
            bare.append(int(g))
    rest = [int(g) for g in perm if int(g) not in set(bare)]
    members, at = [], 0
    for s in sizes:
        members.append(rest[at:at + s])
        at += s
    members.append(bare)
    members = [m for m in members if len(m)]
    pip = np.cumsum([0] + [len(m) for m in members]).astype(np.int32)
    pix = np.concatenate([np.array(m, dtype=np.int32) for m in members])
    vA = np.empty(n, dtype=np.int32)
    for a, m in enumerate(members):
        vA[m] = a
    m = len(members)
    return dict(A=A, PT=(pip, pix), vA=vA, n=n, m=m, bare=m - 1,
                cA={d: rs.uniform(-1.0, 1.0, size=(m, d)) for d in (2, 3, 8)},
                rA=rs.uniform(0.1, 0.6, m))
