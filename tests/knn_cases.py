"""Inputs and an independent reference for the exact k nearest neighbours and the
neighbourhood precision ("layout neighbours", include/ge.h).

The reference shares nothing with the code under test.  Where every squared distance is
exact -- coordinates that are small multiples of 2^-10, for which fma and multiply + add
agree and no sum rounds -- it is numpy (`reference`).  For arbitrary doubles it is a
`fractions.Fraction` chain that rounds once per operation the definition names: each
e_k = x_i[k] - x_j[k], s = e_0 e_0, then s = fma(e_k, e_k, s) (`reference_fraction`, n <=
300 so that it runs in seconds).  Both sort the candidates by (s, j) with Python's sort
and are computed once per input at k = 64: the order is total, so the neighbours at a
smaller k are a prefix.

`restate_insertions` restates one chain of the scan in Python (the threshold is the list's
last s, strict less inserts) to count list insertions: what ge_knn_info reports, summed
over the call's j splits.
"""
import functools
import math
from fractions import Fraction

import numpy as np

MAX_K = 64
INF = float("inf")

# ---- the documented shape (include/ge.h, ge_knn_info) --------------------------------
TILE_J = 256
LDS_BUDGET = 80 * 1024   # half of a CU's 160 KiB
ENTRY_BYTES = 12
MAX_SPLIT = 16
TARGET_BLOCKS = 512


def rows_per_wg(k, d):
    """The most of 256, 128, 64 query rows whose lists of k 12-byte entries fit beside the
    partner tile (256 records of d doubles up to d = 4, of 16 above) in 80 KiB."""
    tile = TILE_J * (d if d <= 4 else 16) * 8
    for rows in (256, 128):
        if tile + rows * k * ENTRY_BYTES <= LDS_BUDGET:
            return rows
    return 64


def switch_ks(d):
    """The largest k with 256 rows per workgroup and the largest with 128."""
    return [max(k for k in range(1, MAX_K + 1) if rows_per_wg(k, d) == r) for r in (256, 128)]


def auto_jsplit(n, n_rows, k, d):
    r = rows_per_wg(k, d)
    blocks = max(1, -(-n_rows // r))
    return max(1, min(-(-TARGET_BLOCKS // blocks), MAX_SPLIT, -(-n // TILE_J)))


# ---- inputs ---------------------------------------------------------------------------
def exact_coords(n, d, seed=1):
    """Multiples of 2^-10 in [-1/2, 1/2]: every difference, square and sum of up to 16
    squares is exact in a double."""
    rs = np.random.RandomState(seed)
    return rs.randint(-512, 513, size=(n, d)).astype(np.float64) / 1024.0


def lattice(n, d):
    """The first n points of an integer lattice of side ceil(n^(1/d)): ties everywhere."""
    m = 1
    while m ** d < n:
        m += 1
    i = np.arange(n)
    return np.stack([(i // m ** c) % m for c in range(d)], axis=1).astype(np.float64)


def coincident(n, d):
    return np.full((n, d), 0.375)


def duplicated(n, d, seed=2):
    """Every point of exact_coords(ceil(n / 2)) twice: vertex i and i + ceil(n / 2)."""
    h = -(-n // 2)
    X = exact_coords(h, d, seed)
    return np.concatenate([X, X])[:n].copy()


def random_doubles(n, d, seed=3):
    rs = np.random.RandomState(seed)
    return rs.uniform(-1.0, 1.0, size=(n, d)) * 10.0 ** rs.randint(-2, 3, size=(n, 1))


def closer_line(n, d=1):
    """Seen from vertex 0 every later partner is closer: x_0 = 0, x_j = (n - j) 2^-10."""
    X = np.zeros((n, d))
    X[1:, 0] = (n - np.arange(1, n)) / 1024.0
    return X


def farther_line(n, d=1):
    """Seen from vertex 0 every later partner is farther: x_j = j 2^-10."""
    X = np.zeros((n, d))
    X[:, 0] = np.arange(n) / 1024.0
    return X


BAD_KINDS = ("nan", "inf", "overflow")


def bad_vertices(kind, n):
    """Which vertices of with_bad(kind, n, d) are outside the domain."""
    return [n // 3] if kind in ("nan", "inf") else [n // 3, (2 * n) // 3]


def with_bad(kind, n, d, seed=4):
    """exact_coords with one NaN vertex, one infinite vertex, or one vertex at +1e200 and
    one at -1e200 (their squared differences overflow, also against each other)."""
    X = exact_coords(n, d, seed)
    v = bad_vertices(kind, n)
    if kind == "nan":
        X[v[0], d // 2] = np.nan
    elif kind == "inf":
        X[v[0], d - 1] = -np.inf
    else:
        X[v[0], 0] = 1e200
        X[v[1], 0] = -1e200
    return X


# ---- the references -------------------------------------------------------------------
def _select(s_row, i, k):
    """The first k candidates of row i by (s, j), from its row of squared distances."""
    ok = np.isfinite(s_row)
    ok[i] = False
    js = np.nonzero(ok)[0]
    if len(js) > k:  # everything up to the k-th smallest s, ties included
        cut = np.partition(s_row[js], k - 1)[k - 1]
        js = js[s_row[js] <= cut]
    best = sorted((float(s_row[j]), int(j)) for j in js)[:k]
    idx = [j for _, j in best] + [-1] * (k - len(best))
    d2 = [s for s, _ in best] + [INF] * (k - len(best))
    return idx, d2


def reference(X, k=MAX_K, rows=None):
    """numpy; only for inputs whose squared distances are exact (or overflow)."""
    X = np.asarray(X, np.float64)
    n = len(X)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    idx = np.empty((len(rows), k), np.int32)
    d2 = np.empty((len(rows), k))
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(0, len(rows), 256):
            r = rows[b:b + 256]
            e = X[r, None, :] - X[None, :, :]
            s = (e * e).sum(axis=2)
            for t, i in enumerate(r):
                idx[b + t], d2[b + t] = _select(s[t], int(i), k)
    return idx, d2


def _fl(q):
    """A Fraction rounded to the nearest double (ties to even); +inf on overflow."""
    try:
        return float(q)
    except OverflowError:
        return INF


def dist2_fraction(xi, xj):
    """The chain of include/ge.h with one rounding per operation."""
    if not (all(map(math.isfinite, xi)) and all(map(math.isfinite, xj))):
        return INF  # NaN or +inf: either way no candidate
    e = [_fl(Fraction(a) - Fraction(b)) for a, b in zip(xi, xj)]
    s = _fl(Fraction(e[0]) * Fraction(e[0]))
    for ek in e[1:]:
        if s == INF:
            return INF
        s = _fl(Fraction(ek) * Fraction(ek) + Fraction(s))
    return s


def reference_fraction(X, k=MAX_K, rows=None):
    X = np.asarray(X, np.float64)
    n = len(X)
    assert n <= 300
    pts = [tuple(float(v) for v in row) for row in X]
    S = np.full((n, n), INF)
    for i in range(n):
        for j in range(i):
            S[i, j] = S[j, i] = dist2_fraction(pts[i], pts[j])  # the same bits both ways
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = [_select(S[int(i)], int(i), k) for i in rows]
    return (np.array([o[0] for o in out], np.int32).reshape(len(rows), k),
            np.array([o[1] for o in out], np.float64).reshape(len(rows), k))


@functools.lru_cache(maxsize=None)
def case(kind, n, d):
    """(X, idx, dist2) of a named input at k = 64, computed once; read-only."""
    exact = True
    if kind == "exact":
        X = exact_coords(n, d)
    elif kind == "lattice":
        X = lattice(n, d)
    elif kind == "coincident":
        X = coincident(n, d)
    elif kind == "duplicated":
        X = duplicated(n, d)
    elif kind == "closer":
        X = closer_line(n, d)
    elif kind == "farther":
        X = farther_line(n, d)
    elif kind in BAD_KINDS:
        X = with_bad(kind, n, d)
    elif kind == "doubles":
        X, exact = random_doubles(n, d), False
    else:
        raise KeyError(kind)
    idx, d2 = reference(X) if exact else reference_fraction(X)
    for a in (X, idx, d2):
        a.setflags(write=False)
    return X, idx, d2


def restate_insertions(X, rows, k, jsplit=1):
    """List insertions of the scan, summed over the query rows and the jsplit chains of
    ceil(n / jsplit) ascending partners each."""
    X = np.asarray(X, np.float64)
    n = len(X)
    chunk = -(-n // jsplit)
    total = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for i in rows:
            e = X[i][None, :] - X
            s = (e * e).sum(axis=1)  # exact inputs only
            for b in range(jsplit):
                held = []
                for j in range(min(n, b * chunk), min(n, (b + 1) * chunk)):
                    tau = held[-1] if len(held) == k else INF
                    if j != i and s[j] < tau:
                        held.append(float(s[j]))
                        held.sort()  # stable: the new entry lands behind its equals
                        del held[k:]
                        total += 1
    return total


# ---- neighbourhood --------------------------------------------------------------------
def csr(rows_of):
    ip = np.zeros(len(rows_of) + 1, np.int32)
    ip[1:] = np.cumsum([len(r) for r in rows_of])
    ix = np.array([j for r in rows_of for j in r], np.int32)
    return ip, ix, np.ones(len(ix))


def ring(n):
    return csr([sorted({(i - 1) % n, (i + 1) % n}) for i in range(n)])


def circle(n):
    a = 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(a), np.sin(a)], axis=1)


HUB_KMAX = 8


def mixed_graph(n=60):
    """Row 0: a hub on every other vertex (degree above HUB_KMAX); row 1: a self entry
    and duplicate entries; row 2: isolated; row 3: only a self entry; the rest a ring.
    Not symmetric."""
    rows_of = [sorted({(i - 1) % n, (i + 1) % n}) for i in range(n)]
    rows_of[0] = list(range(1, n))
    rows_of[1] = [1, 1, 2, 2, 5, 7, 7]
    rows_of[2] = []
    rows_of[3] = [3]
    return csr(rows_of)


def neighbourhood_reference(A, nbrs, kmax, rows=None):
    """per_row {k_i, hits_i} and the totals from the reference's neighbours (k >= kmax)."""
    ip, ix = A[0], A[1]
    n = len(ip) - 1
    rows = range(n) if rows is None else rows
    per = []
    for q, i in enumerate(rows):
        cols = set(int(j) for j in ix[ip[i]:ip[i + 1]])
        ki = min(len(cols - {i}), kmax)
        first = [int(j) for j in nbrs[q][:ki] if j >= 0]
        per.append((ki, sum(j in cols for j in first)))
    per = np.array(per, np.int32).reshape(len(per), 2)
    totals = np.array([(per[:, 0] > 0).sum(), per[:, 0].sum(), per[:, 1].sum()], np.int64)
    return per, totals
