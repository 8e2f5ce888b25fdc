"""Inputs, long-double references, bounds and float64 restatements of the layout energy
(include/ge.h, "layout energy"; graph-embed_amd/csrc/ge_energy.hip around energy_pair,
ge_energy.hpp): tests/test_energy_cases.py on the CPU, tests/test_gpu_energy.py on the
device.  No device code here.

Inputs.  The graphs and coordinates of tests/fa_fast_cases.py, imported, not copied: its
sizes 1 .. 4 097 are the tile, j-chunk and row-block edges of this pass too (the all-pairs
kernel has fa_repulse_fast's shape: 256 lanes x 4 row slots, tiles of 256, jb = max(1,
min(16, ceil(n / 256))) chunks), with its `degenerate` variants (a coincident pair, a pair
0.25 eps apart, a vertex at the origin) and its two scales (at x1e-300 every squared
distance underflows: every pair is clamped and every length reads as 0).  For the CSR row
pass one more input, hub(): 1 200 vertices, stars from graphs.with_hubs on an empty graph
so that rows of exactly 0, 1, 63, 64, 65, 128, 129 and 600 entries exist (asserted: 64 is
the last one-lane row, 65 the first wave row, 128 / 129 two full strides and one more),
fractional symmetric weights and one negative weight (delta = 0.5 takes its sign), seeded
coordinates in [-1, 1]^3.  Dimensions 5, 8, 16 draw seeded coordinates for the n = 257 and
1 025 graphs.  The sha256 of every input is asserted before use.

Reference.  The five columns in np.longdouble, straight from the definitions of
include/ge.h, with the masses m = deg + 1 taken as the float64 values degp1_kernel
computes (far_cases.masses) as given inputs.  Each column comes with T, the sum of the
absolute values of its terms, which the bounds are relative to.

Bounds, u = 2^-53; A_UF = 2^-508 (below).  None is tuned to the device.
  REP_i, PAIRDIST_i:  1.01 (n + 16 + K_PAIR(d)) u T  [+ (n - 1) A_UF for PAIRDIST],
    K_PAIR(d) = 7 + d / 2.  The sums: n fma / add roundings of the chunk chains, each
    partial sum below T, and 16 for the serial add of at most 16 chunks, as in
    fa_fast_cases.  The term: y = 1 / sqrt(s) carries the project's (3.5 + d / 2) u
    (fa_fast_cases' count of fast_rep_pair's first lines, which energy_pair repeats);
    REP's term m_j min(y, 1 / eps) adds 0.5 u for the constant 1 / eps (a rounded
    quotient where the reference divides by the double eps) and nothing for the fma; the
    column is ((repel / 2) m_i) P, two roundings more (repel / 2 is exact): 6 + d / 2.
    PAIRDIST's term d = s y: y is within 2.5 u of 1 / sqrt(s_c) for the computed s_c, which
    is within (2 + d) u of s, so s_c y = sqrt(s) (1 + (1 + d / 2) u) (1 + 2.5 u) and one
    rounding: 4.5 + d / 2.  One unit to spare, so that the unfused numpy restatement,
    which rounds m_j yh before adding it, is held to the same constant.
  ATT_i, EDGELEN_i:  1.01 (chain + K') u T  [+ terms A_UF for EDGELEN], chain = terms for a
    row of up to 64 entries (one lane, stored order) and ceil(terms / 64) + 64 above (64
    interleaved chains, then the 64 lane sums added in order).  The factor 1.01 is the pair
    columns': it covers the second-order terms ((chain + K') u < 1e-13 here) and the
    reference's own rounding (terms 2^-64 sum |t|, 2^-11 of the first-order count), which
    the first-order counts below leave out.
    EDGELEN: d = sqrt(s), (1.5 + d / 2) u: K' = 2 + d / 2.
    ATT, linear: dh = max(d, eps) (1.5 + d / 2) u, psi = (dh / 2) dh twice that and one
    rounding, (4 + d) u, a' psi one more, the two final roundings (attract / 2 times the
    sum, divided by m_i under nohubs): K' = 7 + d.
    ATT, linlog: psi = q log1p(dh) - dh with q = fl(1 + dh).  The bound is absolute in the
    intermediates: |t| = |a'| ((1 + dh) log(1 + dh) + dh), not |a'| psi, because the
    subtraction cancels for small dh.  q is within (eps_d + 1) u of 1 + dh (eps_d = 1.5 +
    d / 2), log1p(dh_c) within eps_d u of log1p(dh) relative (x / ((1 + x) log1p(x)) <= 1)
    plus the library's LOG1P_ULP, the product one rounding: (2 eps_d + 2 + LOG1P_ULP) u of
    (1 + dh) log(1 + dh); dh_c is off by eps_d u dh and the subtraction rounds once, u |psi|
    <= u |t|: (2 eps_d + 3 + LOG1P_ULP) u |t| = (6 + d + LOG1P_ULP) u |t|, against the linear
    (4 + d): K' grows by 2 + LOG1P_ULP.
    ATT, delta not in {0, 1}: a' = sign(a) pow(|a|, delta): K' grows by POW_ULP.
  GRAV_i:  (3.5 + d / 2) u T + gravity m_i A_UF  (|x_i| as d above, then two products).
  A_UF: the kernels form sums of squares without scaling.  A sum of squares below the
    smallest normal double, 2^-1022, is held to at best 2^-1075 absolute and may be 0; the
    Newton steps of energy_pair then start from a halved s that may itself round to 0, and
    the distance s y comes out anywhere in [0, 2.25 x 2^-511]; the true one is below
    2^-511.  Such a term is therefore off by less than 2^-508 = 1.2e-153, absolutely, and a
    sum of squares above 2^-1022 loses less than that to its underflowed products.  Only
    the unclamped lengths need it: a clamped distance below eps is exactly eps either way.
  Totals: the rows' bounds summed, plus the reduction's own roundings: a value passes
    through 2 + 8 additions inside its block of 1 024 and at most ceil(rows / 1 024) serial
    additions of block sums, every partial sum below the column's T: (10 + ceil(rows /
    1 024)) u sum_i T_i.
LOG1P_ULP and POW_ULP: the device library's documentation is not installed next to the
compiler, so both were measured (scripts/micro/ocml_ulp.hip on an MI355X, ROCm 7, against
np.longdouble): log1p on 2^20 log-uniform operands in [1e-5, 4] (the hub input's clamped
distances lie in [1e-5, 2 sqrt 3]), pow(a, 0.5) on 2^20 uniform a in [0.125, 2] (the hub
input's |weights| lie in [0.25, 1.5]).  Largest observed relative error, in units of u: 1.129 (log1p, at
0.0650) and 1.836 (pow, at 0.1250); the bounds use twice those (scripts/ocml_ulp.py prints
them).
"""
import functools

import numpy as np

import fa_fast_cases as C
import far_cases as FAR
import graphs as G
from far_cases import KFAEPS, LD, U  # noqa: F401

COLS = 5
REP, ATT, GRAV, PAIRDIST, EDGELEN = range(COLS)
LANE_ROW = 64       # kEnergyLaneRow
BLOCK_ROWS = 1024   # kEnergyBlockRows
A_UF = 2.0 ** -508
MEASURED_LOG1P = 1.129  # u, largest observed relative error of the device's log1p
MEASURED_POW = 1.836    # u, of pow(a, 0.5)
LOG1P_ULP = 2 * MEASURED_LOG1P
POW_ULP = 2 * MEASURED_POW

INPUTS = C.INPUTS
INPUT_IDS = C.INPUT_IDS
CASES = C.CASES
CASE_IDS = C.CASE_IDS

HUB_N = 1200
HUB_D = 3
HUB_ROWS = (0, 1, 63, 64, 65, 128, 129, 600)
HUB_STARS = [(10, 63), (200, 64), (400, 65), (600, 128), (800, 129), (1000, 600)]
HUB_SHA = "07ed6c647f5e6decc0900d79a7117fe27e610c570807460c7fc675051cc818b7"
# (linlog, nohubs, delta, use_weights) on the hub input
HUB_CASES = [(0, 0, 1.0, 1), (0, 0, 1.0, 0), (1, 0, 1.0, 1), (0, 1, 1.0, 1), (0, 0, 0.0, 1),
             (0, 0, 0.5, 1), (1, 1, 0.5, 1)]
HUB_IDS = [f"linlog{a}-nohubs{b}-delta{c:g}-w{w}" for a, b, c, w in HUB_CASES]

WIDE_DIMS = (5, 8, 16)
WIDE_SIZES = (257, 1025)
WIDE_SHA = {(257, 5): "1950a3f4b5ea8924cf08d8bf4e8ce0eb12c55fed53539c98a9d5dce0f9c0c43b",
            (257, 8): "a679530384dc07fb710fde596385337551c793f31767e123c66fc61342fac83e",
            (257, 16): "b5178eb200706c2956d86f4f19ea52c6a3a944932c898bfd74e314efe26c9df1",
            (1025, 5): "85121791fb3168bf41b296301719020379cae19a824a16ee215395a88fcf1ea3",
            (1025, 8): "51214df8d90822eef36b194559fd627ec1f9c27806eb86ee4c790fc9dc9143a1",
            (1025, 16): "22e3dea5d078b4fa735fb12151343afa2f749c2e06be9c30ab5e49dc8927067a"}


def k_pair(d):
    return 7 + d / 2


def k_att(d, linlog, delta, use_weights):
    k = 7 + d
    if linlog:
        k += 2 + LOG1P_ULP
    if use_weights and delta not in (0.0, 1.0):
        k += POW_ULP
    return k


@functools.lru_cache(maxsize=None)
def hub():
    """(A, X) of the hub input."""
    empty = (np.zeros(HUB_N + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    ip, ix, _ = G.with_hubs(empty, HUB_STARS, seed=90)
    rows = np.repeat(np.arange(HUB_N), np.diff(ip))
    lo, hi = np.minimum(rows, ix).astype(np.int64), np.maximum(rows, ix).astype(np.int64)
    dx = 0.25 + 0.125 * ((lo * 7 + hi * 13) % 11)  # fractional, symmetric
    neg = (lo == min(10, ix[ip[10]])) & (hi == max(10, ix[ip[10]]))  # hub 10's first entry
    assert neg.sum() == 2
    dx[neg] = -0.375
    lens = set(np.diff(ip).tolist())
    assert lens >= set(HUB_ROWS), sorted(lens)
    X = np.random.RandomState(4242).uniform(-1.0, 1.0, size=(HUB_N, HUB_D))
    A = (ip.astype(np.int32), ix.astype(np.int32), dx.astype(np.float64))
    got = FAR._sha(list(A) + [X])
    assert got == HUB_SHA, f"the hub input changed: sha256 {got}"
    for a in list(A) + [X]:
        a.setflags(write=False)
    return A, X


@functools.lru_cache(maxsize=None)
def wide_coords(n, d):
    X = np.random.RandomState(7000 + 17 * n + d).uniform(-1.0, 1.0, size=(n, d))
    got = FAR._sha([X])
    assert got == WIDE_SHA[(n, d)], f"the n = {n}, d = {d} coordinates changed: sha256 {got}"
    X.setflags(write=False)
    return X


def masses(A, use_weights):
    """deg + 1 as degp1_kernel: the serial row sum in float64, plus one."""
    return FAR.masses(A, bool(use_weights))


def params(**kw):
    p = dict(repel=1.0, attract=1.0, gravity=1.0, delta=1.0, use_weights=1, linlog=0, nohubs=0)
    p.update(kw)
    return p


# --------------------------------------------------------------------------
# the long-double reference

def _pairs_ld(X, m):
    """P_i = sum_{j != i} m_j / max(d_ij, eps), its absolute twin and L_i = sum d_ij."""
    n = len(X)
    Xl, ml = X.astype(LD), m.astype(LD)
    P, Pa, L = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    for a in range(0, n, 256):
        b = min(n, a + 256)
        e = Xl[a:b, None, :] - Xl[None, :, :]
        dist = np.sqrt((e * e).sum(axis=2))
        inv = 1 / np.maximum(dist, LD(KFAEPS))
        own = (np.arange(a, b)[:, None] == np.arange(n)[None, :])
        inv = np.where(own, LD(0), inv)
        P[a:b] = (inv * ml[None, :]).sum(axis=1)
        Pa[a:b] = (inv * np.abs(ml)[None, :]).sum(axis=1)
        L[a:b] = np.where(own, LD(0), dist).sum(axis=1)
    return P, Pa, L


def _edges_ld(A, X, p):
    """Per stored entry: its row, the term a' psi(dh), its |t| and the length d."""
    ip, ix, dx = A
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    Xl = X.astype(LD)
    e = Xl[ix] - Xl[rows]
    dist = np.sqrt((e * e).sum(axis=1))
    dh = np.maximum(dist, LD(KFAEPS))
    dh = np.where(np.isnan(dist), dist, dh)
    if p["linlog"]:
        big = (1 + dh) * np.log1p(dh)
        psi, psia = big - dh, big + dh
    else:
        psi = dh * dh / 2
        psia = psi
    a = dx.astype(LD) if p["use_weights"] else np.ones(len(ix), LD)
    if p["delta"] == 0.0:
        a = np.ones(len(ix), LD)
    elif p["delta"] != 1.0:
        a = np.sign(a) * np.abs(a) ** LD(p["delta"])
    return rows, a * psi, np.abs(a) * psia, dist


def _reference(A, X, m, p):
    n = len(X)
    P, Pa, L = _pairs_ld(X, m)
    rows, t, ta, dist = _edges_ld(A, X, p)
    ml = m.astype(LD)
    R, T = np.zeros((n, COLS), LD), np.zeros((n, COLS), LD)
    half_r, half_a = LD(p["repel"]) / 2, LD(p["attract"]) / 2
    R[:, REP], T[:, REP] = half_r * ml * P, abs(half_r) * np.abs(ml) * Pa
    att, atta, ln = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    np.add.at(att, rows, t)
    np.add.at(atta, rows, ta)
    np.add.at(ln, rows, dist)
    hub_div = ml if p["nohubs"] else LD(1)
    R[:, ATT], T[:, ATT] = half_a * att / hub_div, abs(half_a) * atta / np.abs(hub_div)
    norm = np.sqrt((X.astype(LD) ** 2).sum(axis=1))
    R[:, GRAV] = LD(p["gravity"]) * ml * norm
    T[:, GRAV] = np.abs(R[:, GRAV])
    R[:, PAIRDIST] = T[:, PAIRDIST] = L
    R[:, EDGELEN] = T[:, EDGELEN] = ln
    R.setflags(write=False)
    T.setflags(write=False)
    return R, T


@functools.lru_cache(maxsize=None)
def reference(n, variant, d, repel, use_weights):
    """(R, T) (n x 5, longdouble) of an input of fa_fast_cases, every other parameter at
    its default.  Computed once per key and never modified."""
    A = C.case(n)[0]
    return _reference(A, C.coords(n, d, variant), C.masses(n, use_weights),
                      params(repel=repel, use_weights=use_weights))


@functools.lru_cache(maxsize=None)
def hub_reference(linlog, nohubs, delta, use_weights):
    A, X = hub()
    return _reference(A, X, masses(A, use_weights),
                      params(linlog=linlog, nohubs=nohubs, delta=delta, use_weights=use_weights,
                             repel=3.5, attract=0.75, gravity=2.0))


def hub_params(linlog, nohubs, delta, use_weights):
    return params(linlog=linlog, nohubs=nohubs, delta=delta, use_weights=use_weights, repel=3.5,
                  attract=0.75, gravity=2.0)


@functools.lru_cache(maxsize=None)
def wide_reference(n, d):
    A = C.case(n)[0]
    return _reference(A, wide_coords(n, d), C.masses(n, 1), params())


# --------------------------------------------------------------------------
# the bounds

def bounds(A, d, T, p, gravity_m):
    """Per row and column (n x 5, longdouble) from the reference's T; gravity_m is
    gravity |m_i| (the underflow allowance of GRAV)."""
    n = T.shape[0]
    terms = np.diff(A[0]).astype(np.int64)
    chain = np.where(terms > LANE_ROW, -(-terms // LANE_ROW) + LANE_ROW, terms).astype(LD)
    B = np.zeros((n, COLS), LD)
    pair = LD(1.01 * (n + 16 + k_pair(d)) * U)
    B[:, REP] = pair * T[:, REP]
    B[:, PAIRDIST] = pair * T[:, PAIRDIST] + LD((n - 1) * A_UF)
    k = k_att(d, p["linlog"], p["delta"], p["use_weights"])
    B[:, ATT] = LD(1.01 * U) * (chain + k) * T[:, ATT]
    B[:, EDGELEN] = LD(1.01 * U) * (chain + 2 + d / 2) * T[:, EDGELEN] + terms * LD(A_UF)
    B[:, GRAV] = LD((3.5 + d / 2) * U) * T[:, GRAV] + gravity_m.astype(LD) * LD(A_UF)
    return B


def totals_bound(B, T):
    """The rows' bounds summed plus (10 + ceil(rows / 1 024)) u sum T per column."""
    rows = B.shape[0]
    return B.sum(axis=0) + LD((10 + -(-rows // BLOCK_ROWS)) * U) * T.sum(axis=0)


def ratio(got, R, B):
    """(largest error / bound over the entries with a positive bound; every entry within
    its bound, and equal to the reference where the bound is 0)."""
    err = np.abs(got.astype(LD) - R)
    pos = B > 0
    worst = float((err[pos] / B[pos]).max()) if pos.any() else 0.0
    return worst, bool((err <= B).all())


# --------------------------------------------------------------------------
# the restatement: the kernels' order in float64 numpy

def restate_pairs(X, m):
    """energy_pairs and the chunk sum of energy_rows_kernel, all rows at once: per chunk
    one serial chain over j ascending, then the chunks' partials added in chunk order."""
    n, d = X.shape
    jb, jchunk = C.chunking(n)
    inv_eps = 1.0 / KFAEPS
    rows = np.arange(n)
    Ps, Ls = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(jb):
            P, L = np.zeros(n), np.zeros(n)
            for j in range(b * jchunk, min(n, (b + 1) * jchunk)):
                e = X - X[j]
                s = e[:, 0] * e[:, 0]
                for k in range(1, d):
                    s = s + e[:, k] * e[:, k]
                y = 1.0 / np.sqrt(s)
                dist = np.where(s == 0.0, 0.0, s * y)
                yh = np.where(rows == j, 0.0, np.minimum(y, inv_eps))
                P = P + m[j] * yh
                L = L + dist
            Ps.append(P)
            Ls.append(L)
    P, L = np.zeros(n), np.zeros(n)
    for a, b in zip(Ps, Ls):
        P, L = P + a, L + b
    return P, L


def _row_sum(v):
    """A row's terms in the row pass's order: serial up to 64 entries; above, lane l's
    chain over entries l, l + 64, ..., then the 64 lane sums in lane order from +0."""
    if len(v) <= LANE_ROW:
        s = 0.0
        for t in v:
            s = s + t
        return s
    lanes = []
    for lane in range(LANE_ROW):
        s = 0.0
        for t in v[lane::LANE_ROW]:
            s = s + t
        lanes.append(s)
    s = 0.0
    for t in lanes:
        s = s + t
    return s


def restate(A, X, m, p):
    """The five columns (n x 5, float64) in the kernels' order."""
    ip, ix, dx = A
    n, d = X.shape
    P, L = restate_pairs(X, m)
    rows = np.repeat(np.arange(n), np.diff(ip))
    e = X[ix] - X[rows]
    s = np.zeros(len(ix))
    for k in range(d):
        s = s + e[:, k] * e[:, k]
    dist = np.sqrt(s)
    dh = np.where(dist < KFAEPS, KFAEPS, dist)
    psi = (1.0 + dh) * np.log1p(dh) - dh if p["linlog"] else (0.5 * dh) * dh
    if not p["use_weights"] or p["delta"] == 0.0:
        t = psi
    elif p["delta"] == 1.0:
        t = dx * psi
    else:
        t = (np.sign(dx) * np.abs(dx) ** p["delta"]) * psi
    out = np.zeros((n, COLS))
    for i in range(n):
        att = _row_sum(t[ip[i]:ip[i + 1]].tolist())
        out[i, ATT] = 0.5 * p["attract"] * att
        if p["nohubs"]:
            out[i, ATT] = out[i, ATT] / m[i]
        out[i, EDGELEN] = _row_sum(dist[ip[i]:ip[i + 1]].tolist())
    out[:, REP] = (0.5 * p["repel"] * m) * P
    s = np.zeros(n)
    for k in range(d):
        s = s + X[:, k] * X[:, k]
    out[:, GRAV] = (p["gravity"] * m) * np.sqrt(s)
    out[:, PAIRDIST] = L
    return out


def reduce_totals(vals):
    """energy_block_sums and energy_sum_blocks in float64 numpy, bit for bit: blocks of
    1 024 consecutive rows (+0 past the last), ((v0 + v1) + (v2 + v3)) per four rows, the
    256 sums folded in halves (a[t] + a[t + h], h = 128 .. 1), the block sums added in
    block order from +0.  A pure function of the values."""
    vals = np.asarray(vals, np.float64)
    rows, cols = vals.shape
    nblocks = -(-rows // BLOCK_ROWS)
    pad = np.zeros((nblocks * BLOCK_ROWS, cols))
    pad[:rows] = vals
    v = pad.reshape(nblocks, 256, 4, cols)
    with np.errstate(invalid="ignore"):
        a = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
        h = 128
        while h >= 1:
            a = a[:, :h] + a[:, h:2 * h]
            h //= 2
        total = np.zeros(cols)
        for b in range(nblocks):
            total = total + a[b, 0]
    return total


# --------------------------------------------------------------------------
# the gradient identity's layout (tests/test_energy_cases.py)

GRAD_N, GRAD_D = 12, 3
GRAD_SHA = "7f014aa1c5a2fd1055744aaa25046d78b5c689bae03f11384192554e6ffcdc2e"


@functools.lru_cache(maxsize=None)
def grad_case():
    """12 points in [-1, 1]^3 no closer than 0.3 (no pair near the clamp, none at the
    origin) on a symmetric ring with chords and fractional weights."""
    lo = np.array(list(range(GRAD_N)) + [0, 2, 3, 5])
    hi = np.array([(i + 1) % GRAD_N for i in range(GRAD_N)] + [6, 9, 7, 10])
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    w = 0.25 + 0.125 * ((lo * 7 + hi * 13) % 11)
    r, c, v = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    ip = np.zeros(GRAD_N + 1, np.int64)
    np.add.at(ip, r + 1, 1)
    A = (np.cumsum(ip).astype(np.int32), c.astype(np.int32), v.astype(np.float64))
    X = np.random.RandomState(GRAD_SEED).uniform(-1.0, 1.0, size=(GRAD_N, GRAD_D))
    e = X[:, None, :] - X[None, :, :]
    sep = np.sqrt((e * e).sum(axis=2)) + 10 * np.eye(GRAD_N)
    assert sep.min() > 0.3, sep.min()
    got = FAR._sha(list(A) + [X])
    assert got == GRAD_SHA, f"the gradient layout changed: sha256 {got}"
    return A, X


GRAD_SEED = 10


def energy_ld(A, X, m, p):
    """E = REP + ATT + GRAV summed over the rows, longdouble (X may be longdouble)."""
    n = len(X)
    Xl, ml = X.astype(LD), m.astype(LD)
    e = Xl[:, None, :] - Xl[None, :, :]
    dist = np.sqrt((e * e).sum(axis=2))
    inv = np.where(np.eye(n, dtype=bool), LD(0), 1 / np.maximum(dist, LD(KFAEPS)))
    rep = (LD(p["repel"]) / 2 * ml[:, None] * ml[None, :] * inv).sum()
    ip, ix, dx = A
    rows = np.repeat(np.arange(n), np.diff(ip))
    dh = np.maximum(dist[rows, ix], LD(KFAEPS))
    psi = (1 + dh) * np.log1p(dh) - dh if p["linlog"] else dh * dh / 2
    a = dx.astype(LD) if p["use_weights"] else np.ones(len(ix), LD)
    t = a * psi
    if p["nohubs"]:
        t = t / ml[rows]
    att = LD(p["attract"]) / 2 * t.sum()
    grav = (LD(p["gravity"]) * ml * np.sqrt((Xl * Xl).sum(axis=1))).sum()
    return rep + att + grav


def force_ld(A, X, m, p):
    """The reference's force after gravity (include/forceatlas.hpp:146-211), longdouble,
    delta = 1."""
    n = len(X)
    Xl, ml = X.astype(LD), m.astype(LD)
    ip, ix, dx = A
    F = np.zeros(Xl.shape, LD)
    for i in range(n):
        for j in range(n):
            if i != j:
                e = Xl[j] - Xl[i]
                dis = max(np.sqrt((e * e).sum()), LD(KFAEPS))
                F[i] += -(e / dis) * (ml[i] * ml[j] * LD(p["repel"]) / (dis * dis))
        for k in range(ip[i], ip[i + 1]):
            e = Xl[ix[k]] - Xl[i]
            dis = max(np.sqrt((e * e).sum()), LD(KFAEPS))
            fa = np.log1p(dis) if p["linlog"] else dis
            fa = fa * (LD(dx[k]) if p["use_weights"] else LD(1))
            if p["nohubs"]:
                fa = fa / ml[i]
            F[i] += (e / dis) * (LD(p["attract"]) * fa)
        F[i] += -Xl[i] / np.sqrt((Xl[i] * Xl[i]).sum()) * LD(p["gravity"]) * ml[i]
    return F


def gradient_ld(A, X, m, p, h=1e-5):
    """Central differences of energy_ld with step h, longdouble."""
    Xl = X.astype(LD)
    g = np.zeros(Xl.shape, LD)
    for i in range(Xl.shape[0]):
        for k in range(Xl.shape[1]):
            up, dn = Xl.copy(), Xl.copy()
            up[i, k] += LD(h)
            dn[i, k] -= LD(h)
            g[i, k] = (energy_ld(A, up, m, p) - energy_ld(A, dn, m, p)) / (2 * LD(h))
    return g
