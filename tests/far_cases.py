"""Inputs and a numpy restatement of GE_MODE_FARFIELD (graph-embed_amd/csrc/ge_far.hip)
for tests/test_far_cases.py (CPU) and tests/test_gpu_farfield.py (device).

Inputs, from numpy RandomState with fixed seeds, sha256 asserted before use:
  n = 4 097   65 leaves of 64 sorted points, the last with one point, in 5 groups of
              G = 16: two levels (leaves, groups);
  n = 16 449  = 64 16^2 + 64 + 1: 258 leaves, 17 groups, 2 top cells -- the second top
              cell holds 65 points in one group of a full and a one-point leaf.
Coordinates are uniform in [-1, 1]^d, d = 1..4; the graph is a ring plus chords with
fractional symmetric weights, so every mass deg + 1 is > 1.  degenerate(d) moves points
of the n = 4 097 input: a coincident pair, a pair closer than kFaEps, a point at the
origin and a clump of 70 coincident points at the box's lower corner (key 0, so the
clump fills sorted positions 0..69 and leaf 0 has radius 0).

The restatement follows ge_far.hip step by step in float64 where the device's bits
matter (box, scale, keys, the acceptance rule) and in np.longdouble where a sum is the
reference for a rounding bound.
"""
import functools
import hashlib

import numpy as np

LEAF = 64
G = 16
MAX_LEVELS = 8
KFAEPS = 0.00001
U = 2.0 ** -53
K_TERM = 24  # rounding term (terms + 24) u sum |t|: tests/test_gpu_faml_fast.py's count
SIZES = (4097, 16449)
DIMS = (1, 2, 3, 4)
LD = np.longdouble

SHA = {4097: "89ece00b4be445e944989e0874e54d6d3bddd6b29de8ee20302dfac06d539f7a",
       16449: "7fba76807a51f9b6536ab942a879ec407ca23061632be2bd151f862f52d44caf"}


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def _build(n):
    rs = np.random.RandomState(1000 + n)
    src = list(range(n))
    dst = [(i + 1) % n for i in range(n)]
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
    ip = np.zeros(n + 1, dtype=np.int32)
    np.add.at(ip, r + 1, 1)
    ip = np.cumsum(ip).astype(np.int32)
    X = {d: rs.uniform(-1.0, 1.0, size=(n, d)) for d in DIMS}
    return (ip, c.astype(np.int32), v.astype(np.float64)), X


@functools.lru_cache(maxsize=None)
def case(n):
    """(A, {d: X}) of the n-vertex input; A = (indptr, indices, data)."""
    A, X = _build(n)
    got = _sha(list(A) + [X[d] for d in DIMS])
    assert got == SHA[n], f"the n = {n} input changed: sha256 {got}"
    return A, X


def masses(A, use_weights=True):
    """deg + 1 as degp1_kernel computes it: the serial row sum (np.add.reduceat adds in
    stored order only for short rows; rows here have < 8 entries, below numpy's pairwise
    block), plus one."""
    ip, _, dx = A
    deg = np.zeros(len(ip) - 1)
    for i in range(len(deg)):
        s = 0.0
        for e in range(ip[i], ip[i + 1]):
            s += dx[e] if use_weights else 1.0
        deg[i] = s
    return deg + 1


def degenerate(d):
    """The n = 4 097 coordinates with the hard points: 10 and 11 coincide, 20 and 21 are
    3e-6 apart (closer than kFaEps), 30 is the origin, 100..169 sit on the lower corner."""
    X = case(4097)[1][d].copy()
    X[11] = X[10]
    X[21] = X[20]
    X[21, 0] += 3e-6
    X[30] = 0.0
    X[100:170] = -1.0
    return X


# -- steps 1-4: box, keys, order, summaries ------------------------------------------

def level_shape(n):
    """[(cells, points per cell)] from the leaves up: levels are added until the top
    has at most G cells."""
    out, cnt, pts = [], -(-n // LEAF), LEAF
    while True:
        out.append((cnt, pts))
        if cnt <= G or len(out) == MAX_LEVELS:
            return out
        cnt, pts = -(-cnt // G), pts * G


def box_of(X):
    d = X.shape[1]
    lo = X.min(axis=0)
    ext = float((X.max(axis=0) - lo).max())
    with np.errstate(over="ignore"):
        scale = np.ldexp(1.0, 63 // d) / ext if ext > 0 else 0.0
    if not np.isfinite(scale):
        scale = 0.0
    return np.concatenate([lo, [scale]])


def keys_of(X, box):
    """far_keys in float64: bit (b d + k) of the key is bit b of q_k."""
    n, d = X.shape
    bits = 63 // d
    qmax = np.uint64((1 << bits) - 1)
    keys = np.zeros(n, dtype=np.uint64)
    for k in range(d):
        f = np.floor((X[:, k] - box[k]) * box[d])
        q = np.where(f >= 2.0 ** 63, qmax, np.minimum(f, 2.0 ** 63 - 1024).astype(np.uint64))
        q = np.minimum(q, qmax)
        if d == 1:
            keys = q
        else:
            for b in range(bits):
                keys |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * d + k)
    return keys


def summaries(Xs, ms, pts, dtype=np.float64):
    """Cells of `pts` consecutive sorted records: rows {c, M, a}; a carries the device's
    (1 + 2^-40).  dtype=LD gives the reference values, a without the factor."""
    n, d = Xs.shape
    cnt = -(-n // pts)
    out = np.zeros((cnt, d + 2), dtype=dtype)
    Xs, ms = Xs.astype(dtype), ms.astype(dtype)
    for q in range(cnt):
        x, m = Xs[q * pts:(q + 1) * pts], ms[q * pts:(q + 1) * pts]
        M = m.sum()
        c = (m[:, None] * x).sum(axis=0) / M
        a = np.sqrt(((x - c) ** 2).sum(axis=1).max())
        out[q, :d], out[q, d] = c, M
        out[q, d + 1] = a * (1.0 + 2.0 ** -40) if dtype == np.float64 else a
    return out


def own_layout(X, m, item_rows, theta):
    """The layout the restatement builds itself, in the form FaPlan.far_layout() returns."""
    box = box_of(X)
    keys = keys_of(X, box)
    perm = np.argsort(keys, kind="stable").astype(np.int32)
    Xs, ms = X[perm], m[perm]
    return {"perm": perm, "keys": keys[perm], "box": box, "item_rows": item_rows, "theta": theta,
            "cells": [summaries(Xs, ms, pts) for _, pts in level_shape(len(X))],
            "items": summaries(Xs, ms, item_rows)}


# -- step 5: the walk -------------------------------------------------------------------

def walk(layout, q, n):
    """The cells item q accepts, [(level, index)], and the leaves it evaluates pair by
    pair, both in walk order (merged order: `order`, entries (level, index, accepted))."""
    cells, theta = layout["cells"], layout["theta"]
    d = cells[0].shape[1] - 2
    cI, aI = layout["items"][q, :d], layout["items"][q, d + 1]
    top = len(cells) - 1
    order = []
    l, idx = top, 0
    while True:
        cc = cells[l][idx]
        e = cI - cc[:d]
        s = e[0] * e[0]
        for k in range(1, d):
            s = s + e[k] * e[k]
        t = np.sqrt(s) - aI
        aC = cc[d + 1]
        if aC <= theta * t and t - aC >= KFAEPS:
            order.append((l, idx, True))
        elif l == 0:
            order.append((0, idx, False))
        else:
            l, idx = l - 1, idx * G
            continue
        done = False
        while True:
            idx += 1
            if l == top:
                done = idx >= len(cells[top])
                break
            if idx % G == 0 or idx >= len(cells[l]):
                idx = (idx - 1) // G
                l += 1
                continue
            break
        if done:
            return order


def cell_range(level, idx, n):
    pts = LEAF * G ** level
    return idx * pts, min(n, (idx + 1) * pts)


def partners(layout, order, Xs, ms, n):
    """Partner positions and masses of one item, in the order the lane adds them."""
    d = Xs.shape[1]
    P, W = [], []
    for l, idx, acc in order:
        if acc:
            P.append(layout["cells"][l][idx][None, :d])
            W.append(layout["cells"][l][idx][d:d + 1])
        else:
            a, b = cell_range(0, idx, n)
            P.append(Xs[a:b])
            W.append(ms[a:b])
    return np.concatenate(P), np.concatenate(W)


def pair_sums(xi, di, P, W):
    """In longdouble: F_i = d_i sum_j W_j (x_i - p_j) / max(|x_i - p_j|, eps)^3 and
    sum_j |t_ijk|, for rows xi (r x d) against partners P (k x d)."""
    e = xi.astype(LD)[:, None, :] - P.astype(LD)[None, :, :]
    dis = np.maximum(np.sqrt((e * e).sum(axis=2)), LD(KFAEPS))
    t = e * (di.astype(LD)[:, None] * W.astype(LD)[None, :] / dis ** 3)[:, :, None]
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def replay_item(layout, q, X, m, repel):
    """What far_repulse computes for item q, in longdouble from the layout's float64
    cells: (sorted positions, F, sum |t|, terms per row, walk order)."""
    n = len(X)
    Xs, ms = X[layout["perm"]], m[layout["perm"]]
    r0, r1 = q * layout["item_rows"], min(n, (q + 1) * layout["item_rows"])
    order = walk(layout, q, n)
    P, W = partners(layout, order, Xs, ms, n)
    F, T = pair_sums(Xs[r0:r1], ms[r0:r1] * repel, P, W)
    return np.arange(r0, r1), F, T, len(W), order


def exact_rows(X, m, repel, rows):
    """The exact clamped sum of include/forceatlas.hpp:148-167 for `rows` (original
    ids), in longdouble: (F, sum |t|).  The self pair contributes 0."""
    return pair_sums(X[rows], m[rows] * repel, X, m)


def cell_moments(layout, X, m):
    """Per level, rows (mu_C, S_C, a*_C) about the layout's c_C, in longdouble."""
    n = len(X)
    Xs, ms = X[layout["perm"]].astype(LD), m[layout["perm"]].astype(LD)
    out = []
    for l, cells in enumerate(layout["cells"]):
        d = cells.shape[1] - 2
        mom = np.zeros((len(cells), 3), dtype=LD)
        for q in range(len(cells)):
            a, b = cell_range(l, q, n)
            dx = Xs[a:b] - cells[q, :d].astype(LD)
            r2 = (dx * dx).sum(axis=1)
            mom[q] = (np.sqrt((((ms[a:b, None] * dx).sum(axis=0)) ** 2).sum()),
                      (ms[a:b] * r2).sum(), np.sqrt(r2.max()))
        out.append(mom)
    return out


def truncation_bound(layout, order, moments, xi, di):
    """d_i sum over the accepted cells of 2 mu / rho^3 + 3 S / (rho - a*)^4, per row."""
    d = xi.shape[1]
    out = np.zeros(len(xi), dtype=LD)
    for l, idx, acc in order:
        if not acc:
            continue
        mu, S, astar = moments[l][idx]
        rho = np.sqrt(((xi.astype(LD) - layout["cells"][l][idx][:d].astype(LD)) ** 2).sum(axis=1))
        assert (rho > astar).all()
        out += 2 * mu / rho ** 3 + 3 * S / (rho - astar) ** 4
    return out * di.astype(LD)


def rounding(T, terms):
    """The rounding term per row: the 2-norm over components of (terms + 24) u sum |t|."""
    return 1.01 * (terms + K_TERM) * U * np.sqrt((T.astype(LD) ** 2).sum(axis=1))


def accepted_counts(layout, n):
    """Over all items: accepted cells per level, leaves evaluated pair by pair, pair terms
    (rows x partners, an accepted cell being one partner, less each row's self pair)."""
    acc = [0] * len(layout["cells"])
    leaves = terms = 0
    for q in range(len(layout["items"])):
        rows = min(n, (q + 1) * layout["item_rows"]) - q * layout["item_rows"]
        k = 0
        for l, idx, ok in walk(layout, q, n):
            if ok:
                acc[l] += 1
                k += 1
            else:
                leaves += 1
                a, b = cell_range(0, idx, n)
                k += b - a
        terms += rows * (k - 1)  # less each row's self pair
    return acc, leaves, terms
