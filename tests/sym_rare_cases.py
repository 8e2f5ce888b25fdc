"""Inputs that send the sweeps' bulk loop (ge_sym.hpp tile_steps) through the fix-up of
its detect-then-fix denominators (ge_pair.hpp pair_den_detect), and a layout that
never does.

tile_steps evaluates the pair (row i, column j) of an aggregate, i in row tile
A = i // 64, exactly when 128 <= (i - 64 A) + (j - 64 A) < 64 ntiles, ntiles the column
tiles of the sweep (ceil((size - 64 A) / 64)): the step index is lane + column, and the
tiles 0 and 1 (the diagonal) and the drain run the branch-free form.  Every directed
pair below sits at such a place (in_tile_steps), with coordinates, in P_T storage order
(run_plan's / the oracle's init), whose distance is one of the rare cases:

  ones      significand all ones, numerators powers of two (math_cases geometries;
            at d = 1 the distance alone), joined by a heavy edge so that the pair's
            term dominates both rows: the fix-up must patch the reciprocal;
  low-ones  low word 0xFFFFFFFF, high significand bits not all ones: the fix-up is
            entered and must leave the reciprocal alone;
  same      coincident members (s == 0: the root is NaN);
  half-eps  members 0.5e-5 apart;
  eps       the distance exactly eps, the double below it and the double above it
            (zero extra components);
  step      two pairs of one step (equal i + j in one row tile), flagged for different
            reasons (low-ones and same), ordinary lanes beside them.

Outside `ones` only component 0 differs within a pair, so dis = |e_0| exactly
(sqrt(fl(d d)) == d for every double d).
"""
import functools

import numpy as np

import graphs as G
import math_cases as M
import ref_cases as C

SIZES = [321, 257]  # both streamed under GE_FAML_RES_CAP=256: 6 and 5 tiles, short last tiles
PT_SEED = 3
EPS = M.EPS
DETECT = EPS * (1.0 + 2.0 ** -20)  # ge_pair.hpp kFaDetect: the flag's threshold
DIMS = (1, 2, 3, 4)
REPELS = (1.0, 2.0 ** 70)  # 2^70: outside weight_ok, every tile takes the `/` forms


def from_bits(hi, lo):
    return float(np.array([(hi << 32) | lo], dtype=np.uint64).view(np.float64)[0])


def low_word(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0]) & 0xFFFFFFFF


def all_ones(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0]) & (2 ** 52 - 1) == 2 ** 52 - 1


# low word all ones, the 20 high significand bits not: 2^-10, 2^-3, 2^-1, 2^0 and 2^1 scale
LOW_ONES = tuple(from_bits(((1023 + e) << 20) | h, 0xFFFFFFFF)
                 for e, h in ((-10, 0x12345), (-3, 0xABCDE), (-1, 0x00000), (0, 0x7FFFF),
                              (1, 0xFFFFE)))
EPS_TRIO = (EPS, float(np.nextafter(EPS, 0.0)), float(np.nextafter(EPS, 1.0)))

# (kind, aggregate, i, j, distance or None): i, j local indices.  The `ones` pairs take
# their geometry from math_cases.HEAVY_PAIRS (hard pair p, edge weight).
_ONES = tuple(M.HEAVY_PAIRS.items())
PLACES = (
    [("ones", 0, 5 + 4 * t, 200 + 7 * t, p) for t, (p, _) in enumerate(_ONES)] +
    [("low-ones", 0, 20 + 3 * t, 150 + 11 * t, d) for t, d in enumerate(LOW_ONES)] +
    [("same", 0, 40, 300, 0.0), ("half-eps", 0, 43, 290, 0.5e-5)] +
    [("eps", 0, 46 + 2 * t, 250 + 5 * t, d) for t, d in enumerate(EPS_TRIO)] +
    # one step, two reasons: 60 + 130 == 62 + 128
    [("low-ones", 0, 60, 130, LOW_ONES[1]), ("same", 0, 62, 128, 0.0)] +
    # row tile 1 of the first aggregate, and the one member of the second's last tile
    [("low-ones", 0, 70, 262, LOW_ONES[3]), ("same", 1, 3, 256, 0.0),
     ("low-ones", 1, 9, 201, LOW_ONES[0])]
)


def in_tile_steps(size, i, j):
    A = i // 64
    ntiles = (size - 64 * A + 63) // 64
    return i < j < size and 128 <= (i - 64 * A) + (j - 64 * A) < 64 * ntiles


def pair_points(kind, val, dim, t):
    """The two members' coordinates: component 0 differs by `val` exactly (+val/2 and
    -val/2); the extra components are equal within the pair and differ between pairs
    (zero for the eps trio).  `ones`: math_cases.antipodal at dim >= 2."""
    if kind == "ones":
        g = M.HARD_PAIRS[val]
        if dim >= 2:
            return M.antipodal(g, dim)
        return np.array([g[0] / 2]), np.array([-g[0] / 2])
    a = np.full(dim, 0.0 if kind == "eps" else 0.03125 * (t + 1))
    b = a.copy()
    if kind == "same":
        a[0] = b[0] = 0.25 + 0.015625 * t
    else:
        a[0], b[0] = val / 2, -val / 2
    return a, b


def device_distance(a, b):
    """sqrt of the squared distance summed component by component, as rep_term does."""
    e = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    s = e[..., 0] * e[..., 0]
    for k in range(1, e.shape[-1]):
        s = s + e[..., k] * e[..., k]
    return np.sqrt(s)


@functools.lru_cache(maxsize=None)
def directed(dim, repel=1.0):
    """(case, init, pairs): pairs = [(kind, aggregate, i, j, storage c_i, storage c_j)]."""
    n = sum(SIZES)
    PT = C.block_partition(n, SIZES, seed=PT_SEED)
    init = np.random.RandomState(23 + dim).uniform(-1.0, 1.0, size=(n, dim))
    pairs, src, dst, heavy = [], [], [], []
    for t, (kind, a, i, j, val) in enumerate(PLACES):
        ci, cj = int(PT[0][a]) + i, int(PT[0][a]) + j
        init[ci], init[cj] = pair_points(kind, val, dim, t)
        pairs.append((kind, a, i, j, ci, cj))
        if kind == "ones":
            src.append(int(PT[1][ci]))
            dst.append(int(PT[1][cj]))
            heavy.append((src[-1], dst[-1], M.HEAVY_PAIRS[val]))
    R = G.rmat(n, 6 * n, seed=9)
    rows = np.repeat(np.arange(n), np.diff(R[0]))
    A = G.csr_from_edges(n, np.concatenate([rows, np.array(src, np.int64)]),
                         np.concatenate([R[1].astype(np.int64), np.array(dst, np.int64)]))
    A = C.symmetric_weights(A)
    for u, v, w in heavy:
        A = M.with_pair_weights(A, {0: w}, src_of=lambda p: (u, v))
    case = C._ml(A, SIZES, PT_SEED, dim, 1, 19, repel=repel)
    assert np.array_equal(case["PT"][1], PT[1])
    init.setflags(write=False)
    return case, init, tuple(pairs)


@functools.lru_cache(maxsize=None)
def plain(dim):
    """(case, init): the same aggregates on a uniform(-1, 1) start -- no pair and no
    member's distance to the origin (a short last tile's padding) near eps."""
    case, _, _ = directed(dim)
    n = sum(SIZES)
    init = np.random.RandomState(17).uniform(-1.0, 1.0, size=(n, dim))
    init.setflags(write=False)
    return case, init


def aggregate_distances(init, a):
    """Distances of all pairs i < j of aggregate a, and the members' norms."""
    lo = sum(SIZES[:a])
    X = np.asarray(init)[lo:lo + SIZES[a]]
    i, j = np.triu_indices(len(X), 1)
    return device_distance(X[i], X[j]), device_distance(X, np.zeros_like(X))
