"""Directed operands for the exact fp64 helpers of the strict kernels
(graph-embed_amd/csrc/ge_math.hpp sqrt_normal / recip_of / div_by / div_by_nz,
ge_pair.hpp pair_den / rep_term) with a correctly rounded reference (test
infrastructure; tests/test_math_cases.py checks this module on the CPU,
tests/test_gpu_math_exact.py runs the cases on the device).

The reference is exact: a quotient is float(Fraction(n) / Fraction(d)) (Python
rounds the rational correctly), a square root is math.isqrt on a scaled integer
with the round-to-nearest-even decision taken on the integer remainder.  Nothing
here is random and nothing is read from a file; every family is built when the
module is imported and its size is a constant the CPU test asserts, so a family
cannot shrink silently.

Families
  denominators  significands 2^53 - k and 2^52 + k (k = 1..8) over the binades a
                clamped norm can lie in ([1e-5, 2^202]), and eps itself.  2^53 - 1
                (all ones) is the exceptional denominator of the quotient's final
                correction step: RN(1/d) = 2^-e (1 + 2^-52) there, but a Newton
                step from the power of two below it returns that power of two.
  numerators    +-2^-j and +-1.5 2^-j (j = 0..60) and the integers 1..4096 times
                the denominator's binade, +-d, 0, and the pull form fl(q 100).
  squares       around 4^m and 2 4^m, the squares of the denominators with their
                neighbours, exact squares A^2.
  geometries    coordinate pairs whose distance is a hard denominator exactly,
                found by scanning the second component (scan_e1); HARD_PAIRS are
                those with a component quotient within 2^-100 of a rounding
                boundary, laid out as antipodal points for the kernel tests.
"""
import math
from fractions import Fraction

import numpy as np

import graphs as G

EPS = 0.00001  # kFaEps (ge_pair.hpp), include/forceatlas.hpp:110, :337


# --------------------------------------------------------------------------
# the exact reference

def exact_div(n, d):
    """RN(n / d) for finite doubles, d != 0."""
    if n == 0.0:
        return math.copysign(0.0, n) * math.copysign(1.0, d)
    return float(Fraction(n) / Fraction(d))


def exact_sqrt(s):
    """RN(sqrt(s)) for a finite double s > 0."""
    m, e = math.frexp(s)
    M, e = int(math.ldexp(m, 53)), e - 53  # s = M 2^e, 2^52 <= M < 2^53
    if e & 1:
        M, e = M << 1, e - 1
    N = M << 54  # 2^106 <= N < 2^108: the integer root has 54 bits, the last one the half ulp
    r = math.isqrt(N)
    rem = N - r * r
    q, half = r >> 1, r & 1
    if half and (rem > 0 or (q & 1)):
        q += 1
    return math.ldexp(q, (e - 54) // 2 + 1)


def midpoint_distance(n, d):
    """|n/d - m| / |n/d| for the rounding boundary m nearest to the exact n/d."""
    q = Fraction(n) / Fraction(d)
    r = float(q)
    mids = [(Fraction(r) + Fraction(math.nextafter(r, t))) / 2 for t in (math.inf, -math.inf)]
    return min(abs(q - m) for m in mids) / abs(q)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def hexf(x):
    return float(x).hex()


# --------------------------------------------------------------------------
# the domain the strict kernels admit (ge_math.hpp), restated

def coord_ok(x):
    a = abs(x)
    return a == 0.0 or 2.0 ** -200 <= a <= 2.0 ** 200


def weight_ok(w):
    return 2.0 ** -60 <= w <= 2.0 ** 60


def exact_den(d):
    return 2.0 ** -960 <= abs(d) <= 2.0 ** 960


def norm_ok(d):
    """A clamped norm of in-domain coordinates."""
    return EPS <= d <= 2.0 ** 202


def quotient_ok(n, d):
    """The conditions under which v_div_scale leaves its operands alone (ge_math.hpp
    (a)-(e)): the shared-reciprocal replay of n / d is the compiler's own sequence."""
    if n == 0.0:
        return exact_den(d)
    return (exact_den(d) and abs(n) >= 2.0 ** -252 and abs(n) < abs(d) * 2.0 ** 768
            and abs(exact_div(n, d)) >= 2.0 ** -650)


# --------------------------------------------------------------------------
# denominators

KS = tuple(range(1, 9))
HIGH_SIGS = tuple(2 ** 53 - k for k in KS)  # just below a power of two; k = 1: all ones
LOW_SIGS = tuple(2 ** 52 + k for k in KS)   # just above one
# binades [2^E, 2^(E+1)): those of 1e-5 (-17; its low half lies below eps, so the
# 2^52 + k family starts one binade up), 2^-3, 2^-1, 1, 2^5, 2^52, 2^100, 2^201
HIGH_BINADES = (-17, -16, -3, -1, 0, 5, 52, 100, 201)
LOW_BINADES = (-16, -3, -1, 0, 5, 52, 100, 201)


def _den(sig, E):
    return math.ldexp(sig, E - 52)


def binade(d):
    return math.frexp(d)[1] - 1


DENOMINATORS = tuple([_den(s, E) for E in HIGH_BINADES for s in HIGH_SIGS] +
                     [_den(s, E) for E in LOW_BINADES for s in LOW_SIGS] + [EPS])
N_DENOMINATORS = 8 * 9 + 8 * 8 + 1


def _sig(d):
    return int(math.ldexp(math.frexp(d)[0], 53))


def _hard_squares():
    """Norms whose square rounds to a hard significand although theirs is not one:
    dis around sqrt(2) 2^E and around 2^E, found among the doubles next to
    sqrt(target)."""
    out = []
    for E in (-3, 0, 5):
        for sig in HIGH_SIGS + LOW_SIGS:
            for odd in (0, 1):  # dd = sig 2^(2E + odd - 52)
                dd = math.ldexp(sig, 2 * E + odd - 52)
                c = exact_sqrt(dd)
                for step in range(-4, 5):
                    dis = c
                    for _ in range(abs(step)):
                        dis = math.nextafter(dis, math.inf if step > 0 else -math.inf)
                    if dis * dis == dd and _sig(dis) not in HIGH_SIGS + LOW_SIGS:
                        out.append(dis)
    return tuple(sorted(set(out)))


HARD_SQUARE_NORMS = _hard_squares()


# --------------------------------------------------------------------------
# numerators

JS = tuple(range(0, 61))
INTS = tuple(range(1, 4097))
# the pull form (include/forceatlas.hpp:440): ((cb - ca) / d) * 100 / mag -- the
# numerators fl(q * 100) of a division by the member's clamped norm
PULL_Q = tuple(exact_div(s * n, d) * 100.0
               for d in (_den(HIGH_SIGS[0], 0), _den(LOW_SIGS[0], 0), _den(HIGH_SIGS[2], -1),
                         _den(LOW_SIGS[4], 5))
               for n in (1.0, 0.75, 0.3, 1e-3) for s in (1.0, -1.0))
N_NUM_PER_DEN = 4 * len(JS) + len(INTS) + 3 + len(PULL_Q)


def numerators(d):
    """Every numerator family for the denominator d."""
    scale = math.ldexp(1.0, binade(d))
    out = []
    for j in JS:
        p = math.ldexp(scale, -j)
        out += [p, -p, 1.5 * p, -1.5 * p]
    out += [k * scale for k in INTS]
    out += [d, -d, 0.0]
    out += list(PULL_Q)
    return out


def component_numerators(d):
    """The numerators a vector component over its norm can take: no integers above 1."""
    scale = math.ldexp(1.0, binade(d))
    out = []
    for j in JS:
        p = math.ldexp(scale, -j)
        out += [p, -p, 1.5 * p, -1.5 * p]
    return out + [d, -d, 0.0]


N_COMP_PER_DEN = 4 * len(JS) + 3


# --------------------------------------------------------------------------
# DIV: (n, d) -> n / d

def _div_cases():
    n, d = [], []
    for den in DENOMINATORS:
        nums = numerators(den)
        n += nums
        d += [den] * len(nums)
    return np.array(n), np.array(d)


DIV_N, DIV_D = _div_cases()
N_DIV = N_DENOMINATORS * N_NUM_PER_DEN


def div_reference():
    return np.array([exact_div(float(a), float(b)) for a, b in zip(DIV_N, DIV_D)])


# --------------------------------------------------------------------------
# SQRT: s -> sqrt(s), s in [2^-504, 2^405]

SQRT_M = (-251, -100, -17, -8, -1, 0, 1, 3, 26, 100, 201)
SQUARE_INTS = tuple([2 ** 26 - 1 - i for i in range(64)] + [3, 5, 7, 11, 4097, 46341, 94906267 % 2 ** 26] +
                    [(2654435761 * i) % 2 ** 26 | 1 for i in range(1, 186)])
SQUARE_M = (-100, 0, 100)


def _sqrt_cases():
    out = []
    for m in SQRT_M:
        for k in KS:
            out += [math.ldexp(1.0 + k * 2.0 ** -52, 2 * m), math.ldexp(1.0 - k * 2.0 ** -53, 2 * m),
                    math.ldexp(1.0 + k * 2.0 ** -52, 2 * m + 1),
                    math.ldexp(2.0 - k * 2.0 ** -52, 2 * m)]
    for d in DENOMINATORS + HARD_SQUARE_NORMS:
        s = d * d
        out += [math.nextafter(s, 0.0), s, math.nextafter(s, math.inf)]
    for A in SQUARE_INTS:
        out += [math.ldexp(float(A * A), 2 * m) for m in SQUARE_M]
    return np.array(out)


SQRT_S = _sqrt_cases()
N_SQRT = (len(SQRT_M) * 8 * 4 + 3 * (N_DENOMINATORS + len(HARD_SQUARE_NORMS))
          + len(SQUARE_INTS) * len(SQUARE_M))


def sqrt_reference():
    return np.array([exact_sqrt(float(s)) for s in SQRT_S])


# --------------------------------------------------------------------------
# PAIR: (s, n, c) -> dis = max(sqrt(s), eps), n / dis, c / (dis * dis)

def _pair_cases():
    s, n, c = [], [], []
    t = 0
    for dis in DENOMINATORS:
        # every component numerator, each with another of the integers 1..4096
        for num in component_numerators(dis):
            s.append(dis * dis)
            n.append(num)
            c.append(float(INTS[(t * 37) % len(INTS)]))
            t += 1
    for dis in HARD_SQUARE_NORMS:
        # dis * dis is the hard denominator here: every integer over it
        nums = component_numerators(dis)
        for i, k in enumerate(INTS):
            s.append(dis * dis)
            n.append(nums[i % len(nums)])
            c.append(float(k))
    # below the clamp and at it: dis = eps, rdis from the capped y0
    for sq in (EPS * EPS, math.nextafter(EPS * EPS, 0.0), 1e-12, 2.0 ** -504):
        for num in (1e-6, -1e-6, 2.0 ** -200, 0.0):
            s.append(sq)
            n.append(num)
            c.append(6.0)
    return np.array(s), np.array(n), np.array(c)


PAIR_S, PAIR_N, PAIR_C = _pair_cases()
N_PAIR = N_DENOMINATORS * N_COMP_PER_DEN + len(HARD_SQUARE_NORMS) * len(INTS) + 16


def pair_reference():
    """Columns: dis, n / dis, c / fl(dis dis)."""
    out = np.empty((len(PAIR_S), 3))
    for i, (s, n, c) in enumerate(zip(PAIR_S, PAIR_N, PAIR_C)):
        dis = max(exact_sqrt(float(s)), EPS)
        out[i] = dis, exact_div(float(n), dis), exact_div(float(c), dis * dis)
    return out


# --------------------------------------------------------------------------
# geometries: e = (e0, e1) with RN(sqrt(fl(e0^2 + fl(e1^2)))) = T exactly

GEO_M = (0, -3, 5)
GEO_T = tuple([math.ldexp(2 ** 53 - k, m - 53) for m in GEO_M for k in (1, 2, 3, 4)] +
              [math.ldexp(2 ** 52 + k, m - 52) for m in GEO_M for k in (1, 3, 5, 7)])
GEO_E0 = tuple([2.0 ** -j for j in range(1, 7)] + [1.5 * 2.0 ** -j for j in range(1, 7)])
SCAN_ULPS = 4096


def geo_scale(T):
    """2^m of a hard distance T = 2^m (1 +- tiny)."""
    m, e = math.frexp(T)
    return math.ldexp(1.0, e if m > 0.75 else e - 1)


def scan_e1(T, e0):
    """The double nearest to sqrt(T^2 - e0^2), among those within SCAN_ULPS of it,
    with sqrt(fl(e0^2 + fl(e1^2))) == T; None if there is none."""
    c = np.array([math.sqrt(T * T - e0 * e0)])
    offs = np.arange(-SCAN_ULPS, SCAN_ULPS + 1, dtype=np.int64)
    offs = offs[np.argsort(np.abs(offs), kind="stable")]
    cand = (c.view(np.int64) + offs).view(np.float64)
    hit = np.flatnonzero(np.sqrt(e0 * e0 + cand * cand) == T)
    return float(cand[hit[0]]) if len(hit) else None


def _geometries():
    out = []
    for T in GEO_T:
        for f in GEO_E0:
            e0 = f * geo_scale(T)
            e1 = scan_e1(T, e0)
            out.append((T, e0, e1))
    return tuple(out)


GEOMETRIES = _geometries()  # (T, e0, e1); e1 is None where the scan found nothing
N_GEOMETRIES = len(GEO_T) * len(GEO_E0)
NEAR = Fraction(1, 2 ** 100)


def near_midpoint(g):
    """Whether e0 / T or e1 / T of a geometry lies within 2^-100 (relative) of a
    rounding boundary."""
    T, e0, e1 = g
    return min(midpoint_distance(e0, T), midpoint_distance(e1, T)) < NEAR


HARD_PAIRS = tuple(g for g in GEOMETRIES if g[2] is not None and near_midpoint(g))


def antipodal(g, dim):
    """The two points +e/2 and -e/2 of a geometry in `dim` dimensions (zeros appended):
    their difference is e exactly and each one's norm is T/2."""
    T, e0, e1 = g
    p = np.zeros(dim)
    p[0], p[1] = e0 / 2, e1 / 2
    return p, -p


# --------------------------------------------------------------------------
# REP: (x_i, x_j, deg_i + 1, deg_j + 1, repel) -> rep_term, D = 1..4

REP_WEIGHTS = ((1.0, 1.0, 1.0), (3.0, 7.0, 1.0), (2.0, 5.0, 1.5), (1025.0, 4096.0, 1.0),
               (2.5, 1.5, 0.75), (64.0, 33.0, 1.0))


def rep_cases(dim):
    """Rows (x_i[dim], x_j[dim], deg_i + 1, deg_j + 1, repel)."""
    rows = []
    if dim == 1:
        t = 0
        for d in DENOMINATORS + HARD_SQUARE_NORMS:
            if d > 2.0 ** 200:
                continue  # d / 2 must stay a coordinate of the domain
            for sgn in (1.0, -1.0):
                rows.append([sgn * d / 2, -sgn * d / 2, *REP_WEIGHTS[t % len(REP_WEIGHTS)]])
                t += 1
        return np.array(rows)
    for t, g in enumerate(GEOMETRIES):
        a, b = antipodal(g, dim)
        for u in range(2):
            w = REP_WEIGHTS[(2 * t + u) % len(REP_WEIGHTS)]
            xi, xj = (a, b) if u == 0 else (b, a)
            rows.append([*xi, *xj, *w])
    return np.array(rows)


N_REP = {1: 2 * (N_DENOMINATORS - 16 + len(HARD_SQUARE_NORMS)), 2: 2 * N_GEOMETRIES,
         3: 2 * N_GEOMETRIES, 4: 2 * N_GEOMETRIES}


def rep_reference(rows, dim):
    """rep_term as the reference writes it (include/forceatlas.hpp:152-166), one rounding
    per operation, with the exact quotients and root."""
    out = np.empty((len(rows), dim))
    for r, row in enumerate(rows):
        row = [float(v) for v in row]
        xi, xj = row[:dim], row[dim:2 * dim]
        dip1, djp1, repel = row[2 * dim:]
        e = [a - b for a, b in zip(xi, xj)]
        s = e[0] * e[0]
        for k in range(1, dim):
            s = s + e[k] * e[k]
        dis = max(exact_sqrt(s), EPS) if s > 0.0 else EPS
        cij = dip1 * djp1
        cij = cij * repel
        val = exact_div(cij, dis * dis)
        out[r] = [exact_div(ek, dis) * val for ek in e]
    return out


# --------------------------------------------------------------------------
# layouts for the kernel tests: the hard pairs, then random filler

def layout(n, dim, seed=5):
    """n points in dim >= 2 dimensions: both points of every hard pair (rows 2p and
    2p + 1), then uniform(-1, 1) filler.  No point lies at the origin."""
    assert n >= 2 * len(HARD_PAIRS) and dim >= 2
    X = np.random.RandomState(seed).uniform(-1.0, 1.0, size=(n, dim))
    for p, g in enumerate(HARD_PAIRS):
        X[2 * p], X[2 * p + 1] = antipodal(g, dim)
    assert np.abs(X).max(axis=1).min() > 0.0
    return X


def pair_edges(step=3):
    """(src, dst) joining the two points of every step-th hard pair."""
    p = np.arange(0, len(HARD_PAIRS), step, dtype=np.int64)
    return 2 * p, 2 * p + 1


# One heavy pair per binade of the hard distances: the first all-ones pair of m = 0, -3
# and 5 (HARD_PAIRS follows GEO_T x GEO_E0).  A heavy edge puts deg + 1 ~ w on both points,
# so their mutual repulsion term (c_ij ~ w^2) dominates its row's sum and its last bit
# survives into the coordinates; among hundreds of terms of its own size a one-ulp error
# of one term is absorbed by the adds.  The partner is the farthest point of the circle
# the pairs share, so only one pair per circle can dominate, and between circles the
# weights must grow about as T^1.5 (cross term / mutual term = w_q / w_p (T_p / d_pq)^2).
HEAVY_PAIRS = {0: 2.0 ** 20, 18: 2.0 ** 17, 36: 2.0 ** 25}


def with_pair_weights(A, heavy, src_of=lambda p: (2 * p, 2 * p + 1)):
    """A with the entries between the two points of pair p set to heavy[p], both ways."""
    ip, ix, dx = A
    dx = np.array(dx, dtype=np.float64, copy=True)
    for p, w in heavy.items():
        a, b = src_of(p)
        for u, v in ((a, b), (b, a)):
            e = ip[u] + np.flatnonzero(ix[ip[u]:ip[u + 1]] == v)
            assert len(e) == 1
            dx[e[0]] = w
    return ip, ix, dx


def crafted_fa_case(n, dim, seed=5):
    """(A, X0): layout(n, dim) on a small R-MAT joined along every third hard pair, so
    that the attraction sees the hard distances too; HEAVY_PAIRS by heavy edges."""
    A = G.rmat(n, 4 * n, seed=seed)
    rows = np.repeat(np.arange(n), np.diff(A[0]))
    ps, pd = pair_edges()
    A = G.csr_from_edges(n, np.concatenate([rows, ps]), np.concatenate([A[1].astype(np.int64), pd]))
    return with_pair_weights(A, HEAVY_PAIRS), layout(n, dim, seed=seed)
