"""The synthetic level of the multilevel FARFIELD tests (tests/test_faml_far_cases.py on
the CPU, tests/test_gpu_faml_far.py on the device) and the restatement of the segmented
far-field engine (graph-embed_amd/csrc/ge_far.hip, far_seg_*): tests/far_cases.py applied
to one aggregate's members at a time, with the key's bit count as a parameter.

One level under GE_FAML_RES_CAP=256, built like tests/faml_fast_cases.py (member ids
interleave across aggregates, so position -> vertex is exercised; ring plus chords
inside an aggregate, random cross edges, fractional symmetric weights, so every internal
deg + 1 is > 1).  Aggregate sizes in P_T order:
  257            4 leaves plus a one-point leaf; the leaves are the top
  64, 1, 256     resident classes
  1024           exactly 16 leaves, one level
  300            a small streamed aggregate
  1025           17 leaves; the second top cell is one leaf of one point
  4097           65 leaves in 5 groups
  16449          three levels; a 65-point top cell of a full leaf and a one-point leaf
Coordinates (P_T storage order) are uniform in [-1, 1]^d about a per-aggregate offset,
d = 1..4.  degenerate(d): in the 4097 aggregate a coincident pair, a pair 3e-6 apart and
70 members on the box's lower corner (key 0: sorted positions 0..69, so leaf 0 has
radius 0); the 1025 aggregate with all members coincident.  Everything comes from numpy
RandomState with fixed seeds; the sha256 is asserted before use.
"""
import functools

import numpy as np

import far_cases as F
import faml_fast_cases as FF
import graphs as G

RES_CAP = "256"
SIZES = [257, 64, 1, 256, 1024, 300, 1025, 4097, 16449]
STREAMED = [a for a, s in enumerate(SIZES) if s > 256]
RESIDENT = [a for a, s in enumerate(SIZES) if s <= 256]
DIMS = (1, 2, 3, 4)
RANK_BITS = 23  # kFarSegRankBits
A4097, A1025, A16449 = SIZES.index(4097), SIZES.index(1025), SIZES.index(16449)
SHA = "bbb13775ebb4fe7a8eb4e2c29dc31bfdb52763eaaf603faae4f421945877f86d"


def key_bits(d):
    """Morton bits per axis of the composite key (far_seg_key_bits, GE_FAR_ML_KEY_BITS)."""
    return (64 - RANK_BITS) // d


def far_aggs(far_min):
    """The aggregates that take the far field, larger first (GE_FAML_SCHED_FARAGGS)."""
    return sorted((a for a in STREAMED if SIZES[a] >= far_min), key=lambda a: (-SIZES[a], a))


def fast_items(far_min=None):
    """Row items of faml_fast_repulse: all streamed aggregates, or those below far_min."""
    return sum((SIZES[a] + 255) // 256 for a in STREAMED if far_min is None or SIZES[a] < far_min)


def _build():
    rs = np.random.RandomState(1900)
    n, m = sum(SIZES), len(SIZES)
    perm = rs.permutation(n)
    pip = np.cumsum([0] + SIZES).astype(np.int32)
    members = [np.sort(perm[pip[a]:pip[a + 1]]) for a in range(m)]
    src, dst = [], []
    for v in members:
        k = len(v)
        if k < 2:
            continue
        ring = np.arange(k if k > 2 else 1)
        src += list(v[ring])
        dst += list(v[(ring + 1) % k])
        i, j = rs.randint(0, k, k // 2), rs.randint(0, k, k // 2)
        src += list(v[i[i != j]])
        dst += list(v[j[i != j]])
    vA = np.empty(n, dtype=np.int32)
    for a, v in enumerate(members):
        vA[v] = a
    i, j = rs.randint(0, n, 2 * n), rs.randint(0, n, 2 * n)
    keep = vA[i] != vA[j]
    src += list(i[keep])
    dst += list(j[keep])
    ip, ix, _ = G.csr_from_edges(n, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64))
    rows = np.repeat(np.arange(n), np.diff(ip))
    lo, hi = np.minimum(rows, ix).astype(np.int64), np.maximum(rows, ix).astype(np.int64)
    dx = np.array([0.25, 0.5, 0.75, 1.5, 2.25])[(lo * 7 + hi * 13) % 5]  # symmetric, fractional
    off = {d: rs.uniform(-3.0, 3.0, size=(m, d)) for d in DIMS}
    X = {d: rs.uniform(-1.0, 1.0, size=(n, d)) + np.repeat(off[d], SIZES, axis=0) for d in DIMS}
    return dict(A=(ip, ix.astype(np.int32), dx), PT=(pip, np.concatenate(members).astype(np.int32)),
                vA=vA, n=n, m=m, X=X, off=off,
                cA={d: rs.uniform(-1.0, 1.0, size=(m, d)) for d in DIMS},
                rA=rs.uniform(0.1, 0.6, m))


@functools.lru_cache(maxsize=None)
def level():
    lv = _build()
    got = F._sha(list(lv["A"]) + [lv["PT"][0], lv["PT"][1], lv["vA"], lv["rA"]]
                 + [lv["cA"][d] for d in DIMS] + [lv["X"][d] for d in DIMS])
    assert got == SHA, f"the level changed: sha256 {got}"
    for d in DIMS:
        lv["X"][d].setflags(write=False)
    return lv


@functools.lru_cache(maxsize=None)
def masses(use_weights=1):
    """Internal deg + 1 by P_T position (the plan's DP)."""
    return FF.internal_dp1(level(), use_weights)


def span(a):
    pip = level()["PT"][0]
    return int(pip[a]), int(pip[a + 1])


def degenerate(d):
    """The level's coordinates with the hard points (module docstring)."""
    lv = level()
    X = lv["X"][d].copy()
    b, _ = span(A4097)
    X[b + 11] = X[b + 10]
    X[b + 21] = X[b + 20]
    X[b + 21, 0] += 3e-6
    # an integer point at or below every member's coordinate: masses are multiples of 1/4,
    # so the clump's leaf sums are exact and its centre is the point itself
    X[b + 100:b + 170] = np.floor(lv["off"][d][A4097] - 1.0)
    b, e = span(A1025)
    X[b:e] = X[b]
    return X


# -- the restatement: far_cases per aggregate, keys of `bits` bits per axis --------------

def box_of(X, bits):
    d = X.shape[1]
    lo = X.min(axis=0)
    ext = float((X.max(axis=0) - lo).max())
    with np.errstate(over="ignore"):
        scale = np.ldexp(1.0, bits) / ext if ext > 0 else 0.0
    if not np.isfinite(scale):
        scale = 0.0
    return np.concatenate([lo, [scale]])


def keys_of(X, box, bits):
    """far_seg_keys' Morton part in float64: bit (b d + k) of the key is bit b of q_k."""
    n, d = X.shape
    qmax = np.uint64((1 << bits) - 1)
    keys = np.zeros(n, dtype=np.uint64)
    for k in range(d):
        f = np.floor((X[:, k] - box[k]) * box[d])
        q = np.minimum(np.minimum(f, 2.0 ** 62).astype(np.uint64), qmax)
        if d == 1:
            keys = q
        else:
            for b in range(bits):
                keys |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * d + k)
    return keys


def own_layout(X, m, item_rows, theta, bits):
    """One aggregate's layout as the restatement builds it, in FamlPlan.far_layout()'s form."""
    box = box_of(X, bits)
    keys = keys_of(X, box, bits)
    perm = np.argsort(keys, kind="stable").astype(np.int32)
    Xs, ms = X[perm], m[perm]
    return {"perm": perm, "keys": keys[perm], "box": box, "item_rows": item_rows, "theta": theta,
            "key_bits": bits,
            "cells": [F.summaries(Xs, ms, pts) for _, pts in F.level_shape(len(X))],
            "items": F.summaries(Xs, ms, item_rows)}


def sample_items(s, item_rows):
    """First, last (the one-point tail where there is one), the one before it and a middle item."""
    nit = -(-s // item_rows)
    return sorted({0, nit // 2, max(nit - 2, 0), nit - 1})


def device_cells(Xs, ms, ranges):
    """cell_summary (ge_far.hip) bit for bit, in float64: per range [a, b) of sorted records
    lane j adds records a + j, a + j + 64, ... ascending (M by +, the weighted coordinates
    by fma: exact rationals rounded once), then the xor butterfly 32, 16, .. 1; c = sums / M;
    a = (1 + 2^-40) sqrt(max_j sum_k (x_jk - c_k)^2), squares added in k order."""
    from fractions import Fraction
    d = Xs.shape[1]
    out = np.zeros((len(ranges), d + 2))
    lanes = np.arange(64)
    for q, (a, b) in enumerate(ranges):
        x, m = Xs[a:b], ms[a:b]
        M, sx = np.zeros(64), np.zeros((64, d))
        for j0 in range(0, b - a, 64):
            cnt = min(64, b - a - j0)
            xb, mb = x[j0:j0 + cnt], m[j0:j0 + cnt]
            M[:cnt] = M[:cnt] + mb
            if j0 == 0:
                sx[:cnt] = mb[:, None] * xb  # fma(m, x, 0): one rounding
            else:
                for j in range(cnt):
                    for k in range(d):
                        sx[j, k] = float(Fraction(mb[j]) * Fraction(xb[j, k]) + Fraction(sx[j, k]))
        for o in (32, 16, 8, 4, 2, 1):
            M = M + M[lanes ^ o]
            sx = sx + sx[lanes ^ o]
        c = sx[0] / M[0]
        e = x[:, 0] - c[0]
        s2 = e * e
        for k in range(1, d):
            e = x[:, k] - c[k]
            s2 = s2 + e * e
        out[q, :d], out[q, d] = c, M[0]
        out[q, d + 1] = np.sqrt(s2.max()) * (1.0 + 2.0 ** -40)
    return out


def cell_ranges(s, pts):
    return [(q * pts, min(s, (q + 1) * pts)) for q in range(-(-s // pts))]
