"""Inputs for the CSR row pass (graph-embed_amd/csrc/ge_rows.hpp) whose terms are known
exactly, with the class each row is built for.  tests/test_rows_cases.py proves the
classes on the CPU; tests/test_gpu_rows.py runs them on the device.

Binade rows.  A heavy row of the single-level plan in tile mode is cut into segments
that add rint(t / u) as integers, u = ulp(s0) of the row's repulsion sum s0 = P0 u, and
heavy_finish_kernel rebuilds the serial sum as (P0 + S) u -- valid only when no term is a
tie, no term reaches 2^36 units, every base is a normal number and every prefix stays
strictly inside (2^52, 2^53).  To place a row exactly on each of those edges the terms
must be known to the unit:

  a hub sits at (1, .., 1); each neighbour differs from it in ONE component c by delta,
  |delta| >= 2e-5 (above the reference's distance clamp), with few enough bits that
  1 + delta and delta^2 are exact.  Then dis = |delta|, dir = +-1 in c and +0 elsewhere,
  and with attract = 1 the term is delta * w in component c and +0 in the others.  With
  gravity = 0 the stored force is the row's sum itself.  The graph is a set of directed
  stars (the row pass and the oracle's fa_step_rows_frep read only the row); each hub owns
  its leaves, whose ids ascend in term order, since stored order is column order.

A term is written in eighths of the row's unit: units8 = 8 t / u, so a fractional part
of .25 is 2, .375 is 3 and a tie is 4 (mod 8).

Structure rows use random coordinates and frep = uniform (deg + 1) 1e6; what matters
there is which loop, slot and remainder a row's length selects.
"""
import numpy as np

# ge_rows.hpp
TILE_ROWS, TILE_CAP, ROW_T = 64, 512, 256
HEAVY_DEG, MED_DEG, TILE_MIN_ROWS, CHAIN_EARLY = 2048, 32, 65536, 8192
BIG = 1 << 36  # a term of this many units is flagged
# GE_ROW_* (include/ge.h)
NONE, BINADE, FLAG, BASE, RANGE, WHOLE = 0, 1, 2, 4, 8, 16

T52 = 1 << 52
K = 32768        # terms of about K units of 2^-30: delta ~ 3.05e-5, above the 1e-5 clamp
UEXP = -30
MID = T52 + (T52 >> 1)  # a base in the middle of its binade
KSMAX = 1e6      # binade rows: |F| ~ 2^23 and speed ~ 3e-5, so the cap is not reached
DIMS = (1, 2, 3, 4)


def split_chunk(d):
    """Terms per chunk of ordered_edge_sum_split."""
    return 192 * (4 if d <= 4 else 2 if d <= 8 else 1)


class Row:
    """One hub row: terms (comp, delta, weight) in stored order, base[c] per dimension
    (floats), the status the device must report, and whether (P0 + S) u equals the
    serial sum (None: not asserted)."""

    def __init__(self, name, uexp, terms, base, expect, formula_equal=None):
        self.name, self.uexp, self.terms, self.base = name, uexp, terms, base
        self.expect, self.formula_equal = expect, formula_equal
        self.hub = None

    @property
    def deg(self):
        return len(self.terms)


def _delta(units8, uexp):
    return float(np.ldexp(float(units8), uexp - 3))


def _base(P0, uexp):
    return float(np.ldexp(float(P0), uexp))


def _terms(comp, units8, uexp=UEXP):
    return [(comp, _delta(v, uexp), 1.0) for v in units8]


def _rint8(v):
    """rint(v / 8) of an integer v that is no tie."""
    assert v % 8 != 4
    return (v + 4) // 8 if v >= 0 else -((-v + 4) // 8)


def _vec(d, j, val, other):
    b = [other] * d
    b[j] = val
    return b


def binade_rows(d):
    """The binade rows at dimension d; the special component moves through the
    dimensions with the case index."""
    rows = []
    quiet = _base(MID, UEXP)  # the other dimensions: a valid base, terms of +0

    def add(name, units8, P0, expect, eq=None, uexp=UEXP, terms=None, base=None):
        j = len(rows) % d
        t = terms(j) if terms is not None else _terms(j, units8, uexp)
        b = base(j) if base is not None else _vec(d, j, _base(P0, uexp), quiet)
        rows.append(Row(name, uexp, t, b, expect, eq))

    frac = [8 * K + 2, 8 * K + 3]  # K + .25, K + .375
    n = 600
    one_way = [frac[i % 2] for i in range(n)]
    A = sum(abs(_rint8(v)) for v in one_way)
    for sgn, tag in ((1, "pos"), (-1, "neg")):
        # valid: the prefixes walk to one unit inside each end of the binade
        add(f"valid-low-{tag}", [-sgn * v for v in one_way], sgn * (T52 + 1 + A), BINADE, True)
        add(f"valid-high-{tag}", [sgn * v for v in one_way], sgn * (2 * T52 - 1 - A), BINADE, True)
        # range edge: m - A = 2^52 / m + A = 2^53 exactly; the signs alternate, so every
        # prefix is P0 or K units inside of it and the formula would still be right
        alt = [(1 if i % 2 == 0 else -1) * frac[i % 2] for i in range(n)]
        add(f"edge-low-{tag}", [sgn * v for v in alt], sgn * (T52 + A), RANGE, True)
        add(f"edge-high-{tag}", [-sgn * v for v in alt], sgn * (2 * T52 - A), RANGE, True)
        # real crossing: 600 terms out of the binade, 600 back.  Below 2^52 the spacing
        # halves, so -(K + .375) u is added as -(K + .5) u; above 2^53 it doubles, and
        # (K' + .375) u with K' odd rounds to an even count.  Three segments.
        k2 = K + 1
        add(f"cross-low-{tag}", [-sgn * (8 * K + 3)] * n + [sgn * 8 * K] * n,
            sgn * (T52 + 300 * K), RANGE, False)
        add(f"cross-high-{tag}", [sgn * (8 * k2 + 3)] * n + [-sgn * 8 * k2] * n,
            sgn * (2 * T52 - 300 * k2), RANGE, False)
        # the same walk from far enough inside: valid
        add(f"cross-low-inside-{tag}", [-sgn * (8 * K + 3)] * n + [sgn * 8 * K] * n,
            sgn * (T52 + 1200 * K + 1), BINADE, True)
    # ties: one term of (K + .5) u among 1199 of (K + .25) u (K even, so every prefix has
    # P0's parity): entries 0, 255 | 256 (a thread's second slot), 511 | 512 (a segment's
    # last and the next one's first), inside the last, shortest segment, and last.
    # rint gives K; the serial sum gives K + 1 on an odd prefix.
    for pos in (0, 255, 256, 511, 512, 1100, 1199):
        for par, tag, eq in ((1, "odd", False), (0, "even", True)):
            u8 = [8 * K + 2] * 1200
            u8[pos] = 8 * K + 4
            add(f"tie-{pos}-{tag}", u8, MID + par, FLAG, eq)
    # the segmented row's serial fallback at ordered_edge_sum<D, 1>'s stride of 64
    for deg in (513, 576, 577):
        u8 = [8 * K + 2] * deg
        u8[0] = 8 * K + 4
        add(f"tie-deg{deg}", u8, MID + 1, FLAG, False)

    # a tie in one dimension while every other dimension has valid terms of its own
    def tie_dim(j):
        t = []
        for i in range(1200):
            c = i % d
            t.append((c, _delta(8 * K + (4 if i == 700 + j else 2), UEXP), 1.0))
        return t
    add("tie-one-dim", None, None, FLAG, False, terms=tie_dim,
        base=lambda j: [_base(MID + 1, UEXP)] * d)
    # large terms: u = 2^-40, delta = 2^-4 is 2^36 units; the weight 1 - 2^-36 makes it
    # 2^36 - 1.  A neighbour with a non-finite coordinate gives a NaN term.
    k40 = 1 << 25
    for tag, w, dl, expect in (("2^36", 1.0, 2.0 ** -4, FLAG),
                               ("2^36-1", 1.0 - 2.0 ** -36, 2.0 ** -4, BINADE),
                               ("nan", 1.0, np.nan, FLAG), ("+inf", 1.0, np.inf, FLAG),
                               ("-inf", 1.0, -np.inf, FLAG)):
        def big(j, w=w, dl=dl):
            t = _terms(j, [8 * k40 + 2] * 600, -40)
            t[300] = (j, dl, w)
            return t
        add(f"large-{tag}", None, MID, expect, True if expect == BINADE else None, uexp=-40,
            terms=big)
    # bases: one dimension's repulsion sum is not a usable base, beside valid ones (at
    # d = 1 the only dimension, which also holds the terms).  The least normal has
    # P0 = 2^52 exactly (range); the largest finite is a valid base.
    tiny, least, largest = 5e-324 * 12345, 2.0 ** -1022, float(np.finfo(np.float64).max)
    for tag, val, e1, en in (("+0", 0.0, FLAG | BASE, FLAG | BASE),
                             ("-0", -0.0, FLAG | BASE, FLAG | BASE),
                             ("subnormal", tiny, FLAG | BASE, FLAG | BASE),
                             ("least-normal", least, FLAG | RANGE, RANGE),
                             ("largest", largest, BINADE, BINADE),
                             ("+inf", np.inf, FLAG | BASE, FLAG | BASE),
                             ("-inf", -np.inf, FLAG | BASE, FLAG | BASE),
                             ("nan", np.nan, FLAG | BASE, FLAG | BASE)):
        def base(j, val=val):
            b = _vec(d, j, _base(MID, UEXP), quiet)
            b[(j + 1) % d] = val
            return b
        add(f"base-{tag}", one_way, None, e1 if d == 1 else en, None, base=base)
    return rows


def star_graph(rows, d, first_hub=0):
    """Directed stars: hubs first_hub .., then every hub's leaves with ascending ids.
    Returns dict(A, X, frep, n); sets row.hub."""
    H = len(rows)
    n = first_hub + H + sum(r.deg for r in rows)
    ip = np.zeros(n + 1, dtype=np.int64)
    X = np.ones((n, d))
    frep = np.zeros((n, d))
    ix, dx = [], []
    leaf = first_hub + H
    for q, r in enumerate(rows):
        r.hub = first_hub + q
        ip[r.hub + 1] = r.deg
        frep[r.hub] = r.base
        ids = np.arange(leaf, leaf + r.deg)
        for (c, dl, w), v in zip(r.terms, ids):
            X[v, c] = 1.0 + dl
        ix.append(ids)
        dx.append(np.array([w for _, _, w in r.terms]))
        leaf += r.deg
    ip = np.cumsum(ip)
    A = (ip.astype(np.int32), np.concatenate(ix).astype(np.int32), np.concatenate(dx))
    return dict(A=A, X=X, frep=frep, n=n, dim=d, rows=rows)


_binade = {}


def binade_case(d):
    """The binade graph at dimension d (built once; treat as read-only)."""
    if d not in _binade:
        g = star_graph(binade_rows(d), d)
        for a in (g["X"], g["frep"]) + g["A"]:
            a.setflags(write=False)
        _binade[d] = g
    return _binade[d]


# --------------------------------------------------------------------------
# one row, restated in numpy (float64 ufuncs round every operation separately)

EPS = 0.00001  # include/forceatlas.hpp:110


def row_terms(A, X, i, attract=1.0, use_weights=True):
    """The attraction terms of row i in stored order and the reference's operation
    order (include/forceatlas.hpp:169-203; tests/pyref.py force_atlas): deg x dim."""
    ip, ix, dx = A
    e0, e1 = int(ip[i]), int(ip[i + 1])
    with np.errstate(all="ignore"):
        t = X[ix[e0:e1]] - X[i]
        s = t[:, 0] * t[:, 0]
        for k in range(1, X.shape[1]):
            s = s + t[:, k] * t[:, k]
        dis = np.sqrt(s)
        dis = np.where(dis < EPS, EPS, dis)
        w = dx[e0:e1] if use_weights else np.ones(e1 - e0)
        fa = attract * (dis * w)
        return (t / dis[:, None]) * fa[:, None]


def serial_force(base, terms, xi, gravity, dip1):
    """The reference's force of the row: the serial chain, then gravity (:205-211)."""
    with np.errstate(all="ignore"):
        acc = np.array(base, dtype=np.float64)
        for t in terms:
            acc = acc + t
        m2 = np.float64(0.0)
        for x in xi:
            m2 = m2 + x * x
        g = (-np.asarray(xi) / np.sqrt(m2)) * gravity * dip1
        return acc + g


def _base_of(s0):
    """binade_base: (ok, uexp, P0)."""
    b = int(np.float64(s0).view(np.int64))
    ex = (b >> 52) & 0x7ff
    if ex == 0 or ex == 0x7ff:
        return False, 0, 0
    P0 = (b & (T52 - 1)) | T52
    return True, ex - 1023 - 52, -P0 if b < 0 else P0


def binade_formula(base, terms):
    """segment_rows + heavy_finish_kernel's decision for one heavy row: (status, sum or
    None).  Segments of TILE_CAP entries; a segment with a base that is not normal
    raises the flag and adds nothing; a flagged large term adds nothing; a tie is added
    as rint rounds it."""
    d = len(base)
    bases = [_base_of(s) for s in base]
    S, A, flag = [0] * d, [0] * d, False
    for a in range(0, len(terms), TILE_CAP):
        if not all(ok for ok, _, _ in bases):
            flag = True
            continue
        seg = np.asarray(terms[a:a + TILE_CAP], dtype=np.float64)
        for k in range(d):
            with np.errstate(all="ignore"):
                f = np.ldexp(seg[:, k], -bases[k][1])
                small = np.abs(f) < BIG  # False for NaN
            f = f[small]
            r = np.rint(f)
            if not small.all() or (np.abs(f - r) == 0.5).any():
                flag = True
            r = r.astype(np.int64)  # |r| <= 2^36, 512 of them: exact in int64
            S[k] += int(r.sum())
            A[k] += int(np.abs(r).sum())
    why = FLAG if flag else 0
    out = [None] * d
    for k in range(d):
        ok, uexp, P0 = bases[k]
        if not ok:
            why |= BASE
            continue
        m = abs(P0)
        if not (m - A[k] > T52 and m + A[k] < 2 * T52):
            why |= RANGE
            continue
        out[k] = float(np.ldexp(np.float64(P0 + S[k]), uexp))
    return (BINADE, np.array(out)) if why == 0 else (why, out)


def binade_formula_unchecked(base, terms):
    """(P0 + sum rint(t / u)) u with none of the four tests: what a pass without them
    would store.  Bases normal, terms finite."""
    seg = np.asarray(terms, dtype=np.float64)
    out = []
    for k, s0 in enumerate(base):
        ok, uexp, P0 = _base_of(s0)
        assert ok
        S = sum(int(r) for r in np.rint(np.ldexp(seg[:, k], -uexp)))
        out.append(float(np.ldexp(np.float64(P0 + S), uexp)))
    return np.array(out)


def same_bits(a, b):
    """Equal bit for bit, NaNs equal to NaNs of any payload."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# --------------------------------------------------------------------------
# structure: which loop, slot and remainder a row's length selects

def classify(deg, tiles=None, segments=True):
    """classify_rows restated for rows 0..len(deg)-1: dict(heavy, tiles (lists of rows),
    med, light, nseg)."""
    n = len(deg)
    if tiles is None:
        tiles = n >= TILE_MIN_ROWS
    med = 4 if n <= 65536 else MED_DEG
    cut = TILE_CAP if tiles else HEAVY_DEG
    heavy = sorted((q for q in range(n) if deg[q] > cut), key=lambda q: -deg[q])
    out = dict(heavy=heavy, tiles=[], med=[], light=[], nseg=0)
    if tiles:
        cur, ents = [], 0
        for q in range(n):
            if deg[q] > cut:
                continue
            if not cur or len(cur) == TILE_ROWS or ents + deg[q] > TILE_CAP:
                cur, ents = [], 0
                out["tiles"].append(cur)
            cur.append(q)
            ents += deg[q]
        if segments:
            out["nseg"] = sum(-(-int(deg[q]) // TILE_CAP) for q in heavy)
    else:
        out["med"] = [q for q in range(n) if med < deg[q] <= cut]
        out["light"] = [q for q in range(n) if deg[q] <= med and deg[q] <= cut]
    return out


def census(deg, tiles=None, segments=True):
    """What FaPlan.rows_info() must report for these rows."""
    c = classify(deg, tiles, segments)
    return dict(ntiles=len(c["tiles"]), nheavy=len(c["heavy"]), nmed=len(c["med"]),
                nlight=len(c["light"]), nseg=c["nseg"], seg_mode=1 if c["nseg"] else 0)


# Tiles in row order.  Each group is one intended tile (test_rows_cases.py proves it).
TILE_GROUPS = [
    ("exact-512", [0, 1, 7, 8, 9, 15, 16, 17, 256, 183]),  # closed at exactly 512 entries
    ("257+255", [257, 255]),        # the second entry slot of a thread; 512 again
    ("511", [511]),                 # closed by the entry limit: 511 + 512 > 512
    ("512", [512]),                 # a row that is a whole tile
    ("65th-row", [1] * 64),         # closed by the 65th row
    ("64-empty", [0] * 64),         # a tile of empty rows
    ("leading-empty", [0] * 5 + [3] * 59),
    ("trailing-empty", [500] + [0] * 10),
    ("last", [100, 9, 8, 7]),
]
TILE_HEAVY = [513, 1025]  # after the tiles' rows: heavy in tile mode (2 and 3 segments)
TILE_DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 256, 257, 511, 512, 513)
TILE_DIMS = (1, 2, 3, 4, 8)

# classed rows: light | medium at 4, the wave's stride of 64 (and two of them), the heavy
# cut, then chunk edges of ordered_edge_sum_split.  2304 = 3 x 768 = 6 x 384 = 12 x 192
# and 3072 = 4 x 768 = 8 x 384 = 16 x 192, so the same rows sit on a chunk edge at every
# dimension; +31 | +32 | +33 is lane_chain's first ping-pong pair with its remainder.
CLASSED_DEGREES = (0, 1, 4, 5, 63, 64, 65, 127, 128, 129, 2048, 2049,
                   2303, 2304, 2305, 2335, 2336, 2337, 3071, 3072, 3073, 3103, 3104, 3105)
CLASSED_DIMS = (3, 5, 8, 9, 16)


def random_rows_graph(degrees, n, seed):
    """A directed graph of n vertices whose row q has degrees[q] distinct neighbours
    (q + 1 + j step_q mod n with a random step per row, sorted; no diagonal; rows past
    the list are empty), weights in [0.5, 2)."""
    rs = np.random.RandomState(seed)
    deg = np.zeros(n, dtype=np.int64)
    deg[:len(degrees)] = degrees
    assert deg.max() < n - 1
    step = 1 + (rs.randint(0, 1 << 30, size=n) % np.maximum((n - 2) // np.maximum(deg, 1), 1))
    ip = np.concatenate([[0], np.cumsum(deg)])
    rows = np.repeat(np.arange(n), deg)
    j = np.arange(ip[-1]) - ip[rows]
    off = 1 + j * step[rows]  # distinct and in [1, n - 1]
    assert (off < n).all()
    ix = (rows + off) % n
    order = np.lexsort((ix, rows))
    return (ip.astype(np.int32), ix[order].astype(np.int32), rs.uniform(0.5, 2.0, len(ix)))


def structure_inputs(A, d, seed):
    """Random coordinates and frep = uniform (deg + 1) 1e6 for every row."""
    n = len(A[0]) - 1
    rs = np.random.RandomState(seed)
    X = rs.uniform(-1.0, 1.0, size=(n, d))
    frep = rs.uniform(-1.0, 1.0, size=(n, d)) * ((np.diff(A[0]) + 1.0) * 1e6)[:, None]
    return X, frep


def tiles_graph():
    degrees = [k for _, g in TILE_GROUPS for k in g] + TILE_HEAVY
    return random_rows_graph(degrees, 1100, seed=71), degrees


def classed_graph():
    return random_rows_graph(CLASSED_DEGREES, 3300, seed=72), list(CLASSED_DEGREES)


# Multilevel stored-term chains (kSegStore): member rows of a streamed aggregate in tile
# mode.  Rows of CHAIN_EARLY entries or more are "early" (heavy_chain_kernel<512, 16> on
# the side stream), shorter heavy rows "late" (<256, 8>): 513 is one entry past a tile,
# 767 | 768 | 769 the late chain's third chunk of 256, 8191 | 8192 | 8193 the early cut
# (and the early chain's chunk of 512), +31 | +32 | +33 lane_chain<16>'s first pair.
ML_LATE = (513, 767, 768, 769, 8191)
ML_EARLY = (8192, 8193, 8192 + 31, 8192 + 32, 8192 + 33)
ML_PLANS = {"late": ML_LATE, "early": ML_EARLY, "both": ML_LATE + ML_EARLY}
ML_SIZES = [1500] + [200] * 45  # under GE_FAML_RES_CAP=256: one streamed aggregate
ML_RES_CAP = "256"


def ml_case(which, dim=3):
    """A multilevel case (tests/ref_cases.py form) whose streamed aggregate holds member
    rows of exactly the degrees ML_PLANS[which], every other member row a tile row."""
    import graphs as G
    import ref_cases as C
    n = sum(ML_SIZES)
    rs = np.random.RandomState(31)  # a uniform random graph: no hub of its own
    src = rs.randint(0, n, size=2 * n)
    base = G.csr_from_edges(n, src, (src + 1 + rs.randint(0, n - 1, size=2 * n)) % n)
    case = C._ml(base, ML_SIZES, 7, dim, 2, 37)
    members = case["PT"][1][case["PT"][0][0]:case["PT"][0][1]]
    base_deg = np.diff(case["A"][0])
    quiet = [int(v) for v in members if base_deg[v] <= 8][:len(ML_PLANS[which])]
    A = G.with_degrees(case["A"], dict(zip(quiet, ML_PLANS[which])), seed=5)
    case["A"] = C._canon(C.symmetric_weights(A))
    case["targets"] = quiet
    return case


def ml_census(case, segments=True):
    """ntiles > 0, nheavy, nseg, seg_mode, nearly, nseg_early of the streamed members' rows."""
    deg = np.diff(case["A"][0])[case["PT"][1][case["PT"][0][0]:case["PT"][0][1]]]
    heavy = deg[deg > TILE_CAP]
    early = heavy[heavy >= CHAIN_EARLY]
    segs = lambda v: int(sum(-(-int(k) // TILE_CAP) for k in v))
    if not segments:
        return dict(nheavy=len(heavy), nseg=0, seg_mode=0, nearly=0, nseg_early=0)
    return dict(nheavy=len(heavy), nseg=segs(heavy), seg_mode=2, nearly=len(early),
                nseg_early=segs(early))


NATURAL_N = 65600
NATURAL_PLANS = (65535, 65536, 65537)


def natural_graph():
    """A little over 65 536 vertices, degrees 0..8 with a few medium and heavy rows:
    plans over [0, 65535) are classed (medium above 4), from 65 536 rows on tiled."""
    rs = np.random.RandomState(73)
    deg = rs.randint(0, 9, size=NATURAL_N)
    for q, k in ((10, 40), (50000, 50), (2000, 513), (30000, 600), (65530, 2049),
                 (100, 2100)):
        deg[q] = k
    return random_rows_graph(deg, NATURAL_N, seed=74), deg
