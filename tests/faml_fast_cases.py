"""The synthetic level of the multilevel FAST-mode tests (tests/test_faml_fast_cases.py
on the CPU, tests/test_gpu_faml_fast.py on the device).

One level, built like tests/min_cases.py: member lists that interleave (ascending
ids, no aggregate a contiguous range), inside an aggregate a ring plus skewed chords
(low local indices get more of them), random cross edges, one hub with more than 200
internal neighbours, fractional symmetric weights.  Everything comes from numpy
RandomState with fixed seeds and the sha256 of the level is asserted before use.

Sizes, under GE_FAML_RES_CAP=256 (257 members is already a streamed aggregate), with
R = 4 the rows per lane of faml_fast_repulse (kFastR, ge_faml.hip; an item is up to
64 R = 256 rows):
  streamed  257 (64 R + 1: one full item and an item of one row), 320 (a ragged item
            of one whole tile), 321 (a ragged item of two row slots, the second with
            one row), 512 (2 x 64 R: only full items; 64 R itself is 256 members, which
            the plan's floor of 256 keeps resident), 575 (2 x 64 R + 63: two full items
            and a 63-row one) -- 257 and 320 adjacent in P_T storage, so a tile read
            past base + s would meet the neighbour's members;
  resident  1, 7, 64, 65, 256 (the packed <= 64 and <= 256 classes).
"""
import functools
import hashlib

import numpy as np

import graphs as G

R = 4  # kFastR
RES_CAP = "256"
SIZES = [257, 320, 1, 321, 7, 512, 64, 575, 65, 256]
STREAMED = [a for a, s in enumerate(SIZES) if s > 256]
RESIDENT = [a for a, s in enumerate(SIZES) if s <= 256]
HUB_AGG = 7  # the 575-member aggregate
DIMS = (1, 2, 3, 4)
SEED = 23  # of the start (uniform_stream)
KFAEPS = 0.00001
REL_TOL_FAST = 1e-5  # include/ge.h, tests/test_gpu_parity.py
MODE_FAST = 1

SHA = "e98ed5dd3a6e17115b728212fe308e401c782ceda521ed562479126c720a30d7"

# (dim, repel, use_weights): every dimension with both repel values, weights on and off
CASES = [(1, 1.0, 1), (2, 1.0, 1), (2, 3.5, 0), (3, 1.0, 0), (3, 3.5, 1), (4, 3.5, 1), (4, 1.0, 0)]
CASE_IDS = [f"d{d}-repel{r:g}-w{w}" for d, r, w in CASES]


def fast_items(sizes=None):
    """Row items of one faml_fast_repulse launch over the streamed aggregates."""
    sizes = [SIZES[a] for a in STREAMED] if sizes is None else sizes
    return sum((s + 64 * R - 1) // (64 * R) for s in sizes)


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def _build():
    rs = np.random.RandomState(77)
    n, m = sum(SIZES), len(SIZES)
    perm = rs.permutation(n)
    pip = np.cumsum([0] + SIZES).astype(np.int32)
    members = [np.sort(perm[pip[a]:pip[a + 1]]) for a in range(m)]
    src, dst = [], []
    for a, v in enumerate(members):
        k = len(v)
        if k < 2:
            continue
        for i in range(k if k > 2 else 1):  # ring
            src.append(v[i])
            dst.append(v[(i + 1) % k])
        for _ in range(k // 2):  # chords, skewed towards low local indices
            i = int(k * rs.random_sample() ** 3)
            j = int(rs.randint(0, k))
            if i != j:
                src.append(v[i])
                dst.append(v[j])
        if a == HUB_AGG:  # member 5 joined to 240 other members
            for j in rs.choice(np.setdiff1d(np.arange(k), [5]), size=240, replace=False):
                src.append(v[5])
                dst.append(v[int(j)])
    vA = np.empty(n, dtype=np.int32)
    for a, v in enumerate(members):
        vA[v] = a
    cross = 0
    while cross < 2 * n:
        i, j = (int(x) for x in rs.randint(0, n, 2))
        if vA[i] != vA[j]:
            src.append(i)
            dst.append(j)
            cross += 1
    ip, ix, _ = G.csr_from_edges(n, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64))
    rows = np.repeat(np.arange(n), np.diff(ip))
    lo, hi = np.minimum(rows, ix).astype(np.int64), np.maximum(rows, ix).astype(np.int64)
    dx = np.array([0.25, 0.5, 0.75, 1.5, 2.25])[(lo * 7 + hi * 13) % 5]  # symmetric, fractional
    PT = (pip, np.concatenate(members).astype(np.int32))
    return dict(A=(ip, ix.astype(np.int32), dx), PT=PT, vA=vA, n=n, m=m,
                cA={d: rs.uniform(-1.0, 1.0, size=(m, d)) for d in DIMS},
                rA=rs.uniform(0.1, 0.6, m))


def level_sha(lv):
    return _sha(list(lv["A"]) + [lv["PT"][0], lv["PT"][1], lv["vA"], lv["rA"]]
                + [lv["cA"][d] for d in DIMS])


@functools.lru_cache(maxsize=None)
def level():
    lv = _build()
    assert level_sha(lv) == SHA, level_sha(lv)
    for k in ("vA", "rA"):
        lv[k].setflags(write=False)
    return lv


def internal_dp1(lv, use_weights):
    """deg + 1 of every member by P_T position as forceAtlasMultilevel counts it
    (include/forceatlas.hpp:362-383): the row's entries whose column lies in the
    member's aggregate, added in CSR order."""
    ip, ix, dx = lv["A"]
    vA, pix = lv["vA"], lv["PT"][1]
    out = np.empty(lv["n"])
    for c, g in enumerate(pix):
        acc = 0.0
        for e in range(ip[g], ip[g + 1]):
            if vA[ix[e]] == vA[g]:
                acc += dx[e] if use_weights else 1.0
        out[c] = acc + 1
    return out


def start(oracle, dim, degenerate=False):
    """The seeded start in P_T storage order (n x dim).  degenerate: in the streamed
    aggregates 257 and 575, one coincident pair, one pair closer than kFaEps and one
    member at the exact origin, in different row slots and tiles."""
    lv = level()
    n = lv["n"]
    X = oracle.uniform_stream(SEED, n * dim).reshape(n, dim).copy()
    if degenerate:
        pip = lv["PT"][0]
        for a in (0, HUB_AGG):
            base, s = int(pip[a]), SIZES[a]
            twin_a, twin_b, near_a, near_b, origin = 3, s - 1, 70, s // 2 + 9, 64
            assert len({twin_a, twin_b, near_a, near_b, origin}) == 5
            X[base + twin_b] = X[base + twin_a]
            X[base + near_b] = X[base + near_a]
            X[base + near_b, 0] += 0.25 * KFAEPS
            X[base + origin] = 0.0
    return X


def repulsion_reference(lv, X, dp1, repel):
    """Per streamed member and component, in np.longdouble: the repulsion sum
    F_ik = sum_{j != i} t_ijk and A_ik = sum_{j != i} |t_ijk|, with
    t_ijk = e_k (d_i repel) d_j / max(|e|, eps)^3, e = x_i - x_j (include/forceatlas.hpp:
    394-410, clamp included).  Rows of other members are 0."""
    L = np.longdouble
    n, dim = X.shape
    F = np.zeros((n, dim), dtype=L)
    Aabs = np.zeros((n, dim), dtype=L)
    pip = lv["PT"][0]
    eps = L(KFAEPS)
    for a in STREAMED:
        b0, b1 = int(pip[a]), int(pip[a + 1])
        x = X[b0:b1].astype(L)
        d = dp1[b0:b1].astype(L)
        for i in range(b1 - b0):
            e = x[i] - x  # (s, dim)
            dis = np.maximum(np.sqrt((e * e).sum(axis=1)), eps)
            w = (d[i] * L(repel)) * d / (dis * dis * dis)
            t = e * w[:, None]
            t[i] = 0
            F[b0 + i] = t.sum(axis=0)
            Aabs[b0 + i] = np.abs(t).sum(axis=0)
    return F, Aabs


def drift(got, want, members):
    """max |dX| / max |X| over the given fine vertices."""
    return float(np.abs(got[members] - want[members]).max() / np.abs(want[members]).max())


def members_of(lv, aggs):
    pip, pix = lv["PT"][0], lv["PT"][1]
    return np.concatenate([pix[pip[a]:pip[a + 1]] for a in aggs]).astype(np.int64)
