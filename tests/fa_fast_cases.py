"""Inputs and references of the single-level FAST repulsion tests (fa_repulse_fast and
fa_reduce_parts, graph-embed_amd/csrc/ge_fa.hip, around fast_rep_pair, ge_pair.hpp):
tests/test_fa_fast_cases.py on the CPU, tests/test_gpu_fa_fast.py on the device.  No
device code here.

The kernel's shape.  A block of kFastThreads = 256 lanes holds kRowsPerThreadFast = 4
rows per lane (row slot r of lane t is row base + t + 256 r: a row block is 1 024 rows)
and one of jb j-chunks; it walks its chunk in tiles of kTileJ = 256 partners and writes
one partial sum per row, and fa_reduce_parts adds a row's jb partials in chunk order:
    jb = max(1, min(kFastJBlocks, ceil(n / kTileJ))),   jchunk = ceil(n / jb),
kFastJBlocks = 16 (chunking() restates the two formulas and EXPECT pins them for every
size, so that a change of the constants breaks the tests loudly).  Sizes:
    1, 2, 5            the plan path at tiny n; with few terms the term error dominates;
    255, 256, 257      jb goes from 1 to 2; at 257 jchunk = 129 and both tiles are ragged;
    1023, 1024, 1025   the row-block edge: the last lane's fourth row slot, then a second
                       block of one row; jb goes from 4 to 5;
    4096               jb = 16 and every chunk is exactly one tile;
    4097               17 tiles capped at 16 chunks: jchunk = 257, a full tile plus a tile
                       of one in every chunk but the last.
Every size has a ring plus random chords with fractional symmetric weights (use_weights
changes deg + 1 from n = 2 up) and seeded coordinates, uniform in [-1, 1]^d, d = 1..4,
from numpy RandomState with fixed seeds; the sha256 of each input is asserted before use.
Variants: `degenerate` (n = 257, 1 025, 4 097: a coincident pair, a pair 0.25 eps apart
and a vertex at the exact origin, the partners of each pair in different j-chunks and row
slots and one vertex in a chunk's second tile where there is one, placement() asserts it
from the formulas above) and the scales `x1e9` and `x1e-300` of n = 1 025 (at
1e-300 every squared distance underflows to 0 and every pair is clamped).

The bound.  Per row i and component k, with u = 2^-53,
    |F_ik - F*_ik| <= 1.01 (n + 16 + K_TERM) u sum_{j != i} |t_ijk|,
F* and the |t| the long-double sum of include/forceatlas.hpp:148-167, clamp included
(far_cases.exact_rows).  K_TERM = 24 is the project's term error of fast_rep_pair,
(16.5 + 1.5 d) u = 22.5 u at d = 4 rounded up (derivation: tests/test_gpu_faml_fast.py's
docstring; imported from far_cases, not copied).  The sums: a row's partners 0 .. n - 1
are split over the jb chunks, each chunk one lane's chain of fma's in j order, n fma
roundings in all, every partial sum of a chunk bounded by sum |t|: n u sum |t|; the
reduce then adds the jb <= kFastJBlocks = 16 partials serially, each of its roundings
again bounded by u sum |t|: 16 u sum |t|.  The factor 1.01 covers the second-order terms
((n + 40) u < 1e-12) and the reference's own rounding (n 2^-64 sum |t|, 2^-11 of the
bound).  Rows with sum |t| = 0 occur only at n = 1 and must be exactly 0.  The bound is
not tuned to the device.

The restatement (restate()) follows the kernel's order in float64 numpy: per chunk one
serial chain over j ascending, then the serial reduce over chunks, the clamp as
min(1 / sqrt(s), 1 / eps).  numpy has no fma, so a term has other roundings than the
kernel's, by the same count: s = sum e_k e_k unfused is d products (together 1 u of s, a
sum of positive parts) and d - 1 additions on top of the e's 2 u, (2 + d) u as fused;
y = 1 / sqrt(s) is half of that plus the root's and the quotient's rounding, (3 + d / 2) u
against the kernel's (3.5 + d / 2) u; y (y y) (11 + 1.5 d) u; w three roundings more,
(14 + 1.5 d) u; e_k w is e_k's rounding and the product's own, which the kernel's fma
does not have: (16 + 1.5 d) u, 22 u at d = 4.  The addition to the chain is the sum's
rounding, as in the kernel.  That is below 24 as well, so the restatement is held to the
same constant and needs none of its own.
"""
import functools
import hashlib

import numpy as np

import far_cases as FAR
from far_cases import K_TERM, KFAEPS, LD, U  # noqa: F401  (the project's constants)

TILE_J = 256          # kTileJ
FAST_THREADS = 256    # kFastThreads
ROWS_PER_THREAD = 4   # kRowsPerThreadFast
FAST_JBLOCKS = 16     # kFastJBlocks
ROW_BLOCK = FAST_THREADS * ROWS_PER_THREAD

SIZES = (1, 2, 5, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)
DIMS = (1, 2, 3, 4)
DEGENERATE = (257, 1025, 4097)
SCALES = {"x1e9": 1e9, "x1e-300": 1e-300}
SCALED = 1025
# (n, variant)
INPUTS = ([(n, "plain") for n in SIZES] + [(n, "degenerate") for n in DEGENERATE]
          + [(SCALED, v) for v in SCALES])
INPUT_IDS = [f"n{n}-{v}" for n, v in INPUTS]

# (dim, repel, use_weights): every dimension with both repel values, weights on and off
# (tests/faml_fast_cases.CASES)
CASES = [(1, 1.0, 1), (2, 1.0, 1), (2, 3.5, 0), (3, 1.0, 0), (3, 3.5, 1), (4, 3.5, 1), (4, 1.0, 0)]
CASE_IDS = [f"d{d}-repel{r:g}-w{w}" for d, r, w in CASES]

# n: (jb, jchunk)
EXPECT = {1: (1, 1), 2: (1, 2), 5: (1, 5), 255: (1, 255), 256: (1, 256), 257: (2, 129),
          1023: (4, 256), 1024: (4, 256), 1025: (5, 205), 4096: (16, 256), 4097: (16, 257)}

SHA = {1: "547c5b16659b35505f44d643fc83fdadb1917187e16d1c81f728fe31ef5981b5",
       2: "b81856ade9dd29298d0a803d410b442018a62c58c727d6f569f00cbde0926521",
       5: "c348e61041dd246ea3eb63a247dd44997dfdb6ac7731ed9f79794568e05ec3b8",
       255: "e0ee7a38c59c62681b54281f978f446bb7aaf4656d30375bccdd82619fbde7db",
       256: "a11d32c04115b10e85940241293b76bd7ed58129b43218157414180b9ec68a9c",
       257: "d7ac8f4e10080e65b4a8f4d8807ce21f15c3bbd46f451223ca949797ed2ead0a",
       1023: "0660d094bd81e3e75ed2783a3b8aa23a2fe17a06a317cf353fe4e626af7ac197",
       1024: "45b091780cf184976db9d7b174a7d6ed375ff63c63f466cb4924f6cb3df976c8",
       1025: "ff6d983582d60a93b2540c6fb144fa94902288122f9202fdbdfe24d344c3e7ca",
       4096: "e9285f0cea6e67f61fd2dc9176d662f04a2ec9667013406b1cddc7db4208f6e2",
       4097: "0c9d1fac593b0a064aabbc6428838476ccb428e0810e5a44f69eebdca9405278"}

# n: (twin_a, twin_b, near_a, near_b, origin)
PLACES = {257: (3, 256, 70, 137, 128),
          1025: (3, 1024, 300, 800, 600),
          4097: (3, 4096, 770, 1500, 2700)}


def chunking(n):
    """(jb, jchunk) of fa_schedule (ge_fa_sched.hpp: fast_jb) and fa_repulse_fast."""
    jb = max(1, min(FAST_JBLOCKS, -(-n // TILE_J)))
    return jb, -(-n // jb)


def chunk_of(j, n):
    """(j-chunk, tile within the chunk) that holds partner j."""
    jchunk = chunking(n)[1]
    return j // jchunk, (j % jchunk) // TILE_J


def slot_of(i, rb=0):
    """(row block, row slot, lane) of row i in a plan whose rows begin at rb."""
    q = i - rb
    return q // ROW_BLOCK, (q % ROW_BLOCK) // FAST_THREADS, q % FAST_THREADS


def _build(n):
    rs = np.random.RandomState(2000 + n)
    if n >= 3:
        src = list(range(n))
        dst = [(i + 1) % n for i in range(n)]
    else:
        src, dst = ([0], [1]) if n == 2 else ([], [])
    a = rs.randint(0, n, size=n // 2)
    b = rs.randint(0, n, size=n // 2)
    keep = a != b
    src += list(a[keep])
    dst += list(b[keep])
    lo = np.minimum(src, dst).astype(np.int64)
    hi = np.maximum(src, dst).astype(np.int64)
    pairs = np.unique(lo * n + hi)
    lo, hi = pairs // n, pairs % n
    w = 0.25 + 0.125 * ((lo * 7 + hi * 13) % 11)  # fractional, the same for both directions
    r = np.concatenate([lo, hi])
    c = np.concatenate([hi, lo])
    v = np.concatenate([w, w])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    ip = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ip, r + 1, 1)
    ip = np.cumsum(ip).astype(np.int32)
    X = {d: rs.uniform(-1.0, 1.0, size=(n, d)) for d in DIMS}
    return (ip, c.astype(np.int32), v.astype(np.float64)), X


@functools.lru_cache(maxsize=None)
def case(n):
    """(A, {d: X}) of the n-vertex input; A = (indptr, indices, data)."""
    assert chunking(n) == EXPECT[n], (n, chunking(n))
    A, X = _build(n)
    got = FAR._sha(list(A) + [X[d] for d in DIMS])
    assert got == SHA[n], f"the n = {n} input changed: sha256 {got}"
    for a in list(A) + list(X.values()):
        a.setflags(write=False)
    return A, X


@functools.lru_cache(maxsize=None)
def masses(n, use_weights):
    m = FAR.masses(case(n)[0], bool(use_weights))
    m.setflags(write=False)
    return m


def placement(n):
    """The degenerate variant's vertices, with the kernel's geometry asserted: the two
    partners of each pair in different j-chunks and in different row slots, the five
    vertices in five j-chunks where there are that many, and at n = 4 097 one of them in a
    chunk's second tile (the tile of one)."""
    twin_a, twin_b, near_a, near_b, origin = P = PLACES[n]
    assert len(set(P)) == 5 and max(P) < n
    jb = chunking(n)[0]
    chunks = [chunk_of(j, n)[0] for j in P]
    assert max(chunks) < jb
    assert len(set(chunks)) == min(5, jb), chunks
    for a, b in ((twin_a, twin_b), (near_a, near_b)):
        assert chunk_of(a, n)[0] != chunk_of(b, n)[0]
        # n = 257 has one row outside the first row slot: the coincident pair takes it
        assert slot_of(a)[:2] != slot_of(b)[:2] or (n < 2 * FAST_THREADS and a == near_a)
    assert len({slot_of(i)[:2] for i in P}) >= min(4, -(-n // FAST_THREADS))
    if chunking(n)[1] > TILE_J:
        assert 1 in [chunk_of(j, n)[1] for j in P]
    return P


def coords(n, d, variant="plain"):
    """A fresh copy of the variant's coordinates (n x d)."""
    X = case(n)[1][d].copy()
    if variant == "degenerate":
        twin_a, twin_b, near_a, near_b, origin = placement(n)
        X[twin_b] = X[twin_a]
        X[near_b] = X[near_a]
        X[near_b, 0] += 0.25 * KFAEPS
        X[origin] = 0.0
    elif variant != "plain":
        X *= SCALES[variant]
    return X


@functools.lru_cache(maxsize=None)
def reference(n, variant, d, repel, use_weights):
    """(F*, sum |t|) per row and component in longdouble: far_cases.exact_rows, the
    clamped sum of include/forceatlas.hpp:148-167, in blocks of rows.  Computed once per
    key and never modified."""
    X, m = coords(n, d, variant), masses(n, use_weights)
    parts = [FAR.exact_rows(X, m, repel, np.arange(a, min(n, a + 256))) for a in range(0, n, 256)]
    F, T = (np.concatenate([p[k] for p in parts]) for k in (0, 1))
    F.setflags(write=False)
    T.setflags(write=False)
    return F, T


def bound(n, T):
    """The module docstring's bound from the reference's sum |t| (rows x d, longdouble)."""
    return LD(1.01 * (n + FAST_JBLOCKS + K_TERM) * U) * T


def ratio(got, n, Fr, T):
    """(largest error / bound over the entries with a positive bound, all entries
    within the bound and exactly 0 where the bound is 0)."""
    err = np.abs(got.astype(LD) - Fr)
    b = bound(n, T)
    pos = b > 0
    worst = float((err[pos] / b[pos]).max()) if pos.any() else 0.0
    return worst, bool((err <= b).all())


def restate(X, m, repel):
    """fa_repulse_fast and fa_reduce_parts in float64 numpy, all rows at once: per chunk
    one serial chain over j ascending, then the chunks' partials added in chunk order."""
    n, d = X.shape
    jb, jchunk = chunking(n)
    di = m * repel
    inv_eps = 1.0 / KFAEPS
    parts = []
    with np.errstate(divide="ignore"):
        for b in range(jb):
            acc = np.zeros((n, d))
            for j in range(b * jchunk, min(n, (b + 1) * jchunk)):
                e = X - X[j]
                s = e[:, 0] * e[:, 0]
                for k in range(1, d):
                    s = s + e[:, k] * e[:, k]
                y = np.minimum(1.0 / np.sqrt(s), inv_eps)
                w = di * m[j] * (y * y * y)
                acc = acc + e * w[:, None]
            parts.append(acc)
    F = np.zeros((n, d))
    for p in parts:
        F = F + p
    return F
