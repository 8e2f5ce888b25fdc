"""Inputs for the steps between levels -- P^T A P (graph-embed_amd/csrc/ge_ptap.hip), the
device graph set-up (ge_graph.hip), modularity (ge_quality.hip) and the radius step
(ge_radius.hip) -- placed on the code's own thresholds.  tests/test_setup_cases.py proves
on the CPU that each input has the property it is named for and checks the host paths
against the oracle; tests/test_gpu_setup.py runs them on the device, bit for bit, with the
info queries (ge_ptap_info, ge_graph_info, ge_radius_info) saying which path ran.

Every builder is deterministic (numpy RandomState with a fixed seed) and returns plain
arrays: a CSR is (indptr, indices, data), a P_T is (indptr, indices).
"""
import ctypes

import numpy as np

# ---------------------------------------------------------------------------
# shared helpers


def bits_below(x):
    """ge_ptap.hip bits_below: bits needed for the values 0 .. x-1."""
    b = 0
    while b < 63 and (1 << b) < x:
        b += 1
    return b


def csr_from_rows(n, rows):
    """rows[i]: [(col, weight), ..] in stored order (unsorted and duplicates allowed)."""
    ip = np.zeros(n + 1, np.int32)
    ix, dx = [], []
    for i in range(n):
        for c, w in rows[i]:
            ix.append(c)
            dx.append(w)
        ip[i + 1] = len(ix)
    return ip, np.array(ix, np.int32), np.array(dx, np.float64)


def sym_csr(n, edges, weights=None):
    """Symmetric CSR with ascending columns from undirected edges (i, j), i != j or a
    self-loop; weights: one per direction (2 per edge, 1 per loop), default 1."""
    ent = []
    for i, j in edges:
        ent.append((i, j))
        if i != j:
            ent.append((j, i))
    w = np.ones(len(ent)) if weights is None else np.asarray(weights, np.float64)
    assert len(w) == len(ent)
    order = sorted(range(len(ent)), key=lambda q: ent[q])
    rows = [[] for _ in range(n)]
    for q in order:
        rows[ent[q][0]].append((ent[q][1], float(w[q])))
    return csr_from_rows(n, rows)


def pt_from_sizes(n, sizes, seed):
    """P_T with the given aggregate sizes (zeros allowed) over a permutation of 0..n-1:
    the members of every aggregate are interleaved over the vertex ids."""
    assert sum(sizes) == n
    perm = np.random.RandomState(seed).permutation(n).astype(np.int32)
    ip = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return ip, perm


def random_graph(n, p, seed):
    rs = np.random.RandomState(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rs.random_sample(len(iu)) < p
    return list(zip(iu[keep].tolist(), ju[keep].tolist()))


def mixed_weights(count, seed):
    """+-2^e (1 + k 2^-52), e in -30..30: sums whose value depends on the order."""
    rs = np.random.RandomState(seed)
    e = rs.randint(-30, 31, count)
    k = rs.randint(0, 1 << 20, count)
    s = np.where(rs.randint(0, 2, count) == 0, -1.0, 1.0)
    return s * np.ldexp(1.0 + k * 2.0 ** -52, e)


def uniform_weights(count, seed):
    return np.random.RandomState(seed).uniform(0.1, 2.0, count)


WEIGHTS = {"mixed": mixed_weights, "uniform": uniform_weights}


def slice_rows(C, a0, a1):
    """Rows [a0, a1) of a CSR, as ge_ptap_rows returns them."""
    ip, ix, dx = C
    lo, hi = ip[a0], ip[a1]
    return (ip[a0:a1 + 1] - lo).astype(np.int32), ix[lo:hi], dx[lo:hi]


def concat_rows(parts):
    ip = [np.zeros(1, np.int32)]
    tot = 0
    for p in parts:
        ip.append(p[0][1:] + tot)
        tot += p[0][-1]
    return (np.concatenate(ip).astype(np.int32), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]))


# ---------------------------------------------------------------------------
# P^T A P

SIZES96 = (1, 0, 17, 0, 0, 33, 2, 43, 0)
ORDERS = ("oracle", "flat_emission", "flat_j", "j_descending", "members_reversed")


def ptap_in_order(A, PT, order):
    """P_T A P_T^T in Python with one of five summation orders.  "oracle" is the pinned
    one (oracle/ge_oracle.cpp orc_ptap): B[a][j] adds the members of a in P_T order (a
    member's entries in stored order), C[a][b] adds B's columns j ascending.  The other
    four are the mistakes a sort-based kernel can make."""
    ip, ix, dx = A
    pip, pix = PT
    m = len(pip) - 1
    agg = np.empty(len(ip) - 1, np.int64)
    for a in range(m):
        agg[pix[pip[a]:pip[a + 1]]] = a
    oip, oix, odx = [0], [], []
    for a in range(m):
        members = list(pix[pip[a]:pip[a + 1]])
        if order == "members_reversed":
            members.reverse()
        ent = [(int(ix[e]), float(dx[e])) for i in members for e in range(ip[i], ip[i + 1])]
        C = {}
        if order == "flat_emission":
            for j, w in ent:
                C[agg[j]] = C.get(agg[j], 0.0) + w
        elif order == "flat_j":
            for j, w in sorted(ent, key=lambda t: t[0]):  # stable
                C[agg[j]] = C.get(agg[j], 0.0) + w
        else:
            B = {}
            for j, w in ent:
                B[j] = B.get(j, 0.0) + w
            for j in sorted(B, reverse=(order == "j_descending")):
                C[agg[j]] = C.get(agg[j], 0.0) + B[j]
        for b in sorted(C):
            oix.append(b)
            odx.append(C[b])
        oip.append(len(oix))
    return np.array(oip, np.int32), np.array(oix, np.int32), np.array(odx, np.float64)


def graph96(weights, sizes=SIZES96, seed=96):
    """96 vertices, G(96, 0.15), aggregates of the given sizes interleaved over the ids.
    SIZES96 has empty aggregates single (1) and doubled (3, 4), in the middle and at the
    very end (8), and a one-member aggregate 0."""
    n = 96
    edges = random_graph(n, 0.15, seed)
    A = sym_csr(n, edges, WEIGHTS[weights](2 * len(edges), seed + 1))
    return A, pt_from_sizes(n, sizes, seed + 2)


def empty_rows_graph():
    """48 vertices in 6 aggregates of 8; the rows of the vertices at P_T positions 0 (the
    first), 47 (the last), 20..22 (several in a row), 8 (first of aggregate 1) and 31 (last
    of aggregate 3) are empty, so the row range [1, 4) starts and ends on one.  Columns
    still point at them (A is not symmetric)."""
    n = 48
    PT = pt_from_sizes(n, [8] * 6, 5)
    empty = {int(PT[1][c]) for c in (0, 47, 20, 21, 22, 8, 31)}
    rs = np.random.RandomState(6)
    w = mixed_weights(n * 7, 7)
    rows = []
    for i in range(n):
        cols = sorted(rs.choice(n, 7, replace=False).tolist())
        rows.append([] if i in empty else [(c, float(w[i * 7 + q])) for q, c in enumerate(cols)])
    return csr_from_rows(n, rows), PT, empty, (1, 4)


HUB_DEG = 700  # more than two 256-thread blocks of expand_kernel


def hub_graph(where):
    """1024 vertices on a ring; vertex 300's row has 700 entries in all.  22 aggregates,
    two of them empty in a row (9, 10); the hub is the first or the last member of its
    aggregate in P_T order."""
    n, hub = 1024, 300
    rs = np.random.RandomState(11)
    others = [v for v in rs.permutation(n).tolist() if v not in (hub, hub - 1, hub + 1)]
    edges = [(i, (i + 1) % n) for i in range(n)] + [(hub, v) for v in others[:HUB_DEG - 2]]
    edges = [(min(i, j), max(i, j)) for i, j in edges]
    A = sym_csr(n, edges, mixed_weights(2 * len(edges), 12))
    sizes = [50] * 9 + [0, 0] + [50] * 10 + [74]
    pip, pix = pt_from_sizes(n, sizes, 13)
    a = 5
    pos = int(np.flatnonzero(pix == hub)[0])
    target = pip[a] if where == "first" else pip[a + 1] - 1
    pix[pos], pix[target] = pix[target], pix[pos]  # swap the hub into place
    return A, (pip, pix), hub


def one_aggregate(n=50):
    edges = random_graph(n, 0.2, 21)
    A = sym_csr(n, edges, mixed_weights(2 * len(edges), 22))
    return A, pt_from_sizes(n, [n], 23)


def identity_pt(n=40):
    """m = n: every vertex its own aggregate, in permuted order."""
    edges = random_graph(n, 0.2, 31)
    A = sym_csr(n, edges, uniform_weights(2 * len(edges), 32))
    return A, pt_from_sizes(n, [1] * n, 33)


def single_vertex():
    return ((np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5])),
            (np.array([0, 1], np.int32), np.array([0], np.int32)))


def pow2_graph(n, m):
    """n, m in {64, 65}: bits_below changes between them.  m = 65 with n = 64 has an
    empty aggregate."""
    edges = random_graph(n, 0.12, 41 + n)
    A = sym_csr(n, edges, mixed_weights(2 * len(edges), 42 + m))
    rs = np.random.RandomState(43 + n + m)
    sizes = np.bincount(rs.randint(0, m, n - min(n, m) + 1), minlength=m)
    sizes[:min(n, m) - 1] += 1
    assert sizes.sum() == n
    return A, pt_from_sizes(n, sizes.tolist(), 44)


def unsorted_dups_graph():
    """Rows with shuffled columns and duplicate columns of different weight: the oracle
    adds duplicates in stored order, and the stable sort must keep that order."""
    n = 60
    rs = np.random.RandomState(51)
    w = mixed_weights(n * 12, 52)
    rows = []
    for i in range(n):
        cols = rs.choice(n, 8, replace=False).tolist()
        cols += [cols[0], cols[0], cols[3], cols[5]]  # duplicates, one of them threefold
        rs.shuffle(cols)
        rows.append([(c, float(w[i * 12 + q])) for q, c in enumerate(cols)])
    return csr_from_rows(n, rows), pt_from_sizes(n, [7, 13, 0, 20, 20], 53)


def zeros_graph():
    """Zero, -0.0 and cancelling weights.  Aggregates {0,1}, {2,3}, {4,5} in order.
    (0 -> 1): entries 2.5 and -2.5 on members 0 and 1, column 2: the run sums to exactly
    0 and keeps its entry.  (1 -> 2): only -0.0 entries (the sum starts at +0.0, so the
    result is +0.0).  (2 -> 0): 0.0 and 1.5.  (2 -> 2): 1e300, -1e300, 3.0 on one column
    (stored order decides: 3.0, not 0.0)."""
    rows = [[(2, 2.5), (1, 0.0)], [(2, -2.5)], [(4, -0.0), (5, -0.0)], [(5, -0.0)],
            [(0, 0.0), (1, 1.5), (4, 1e300), (4, -1e300), (4, 3.0)], []]
    A = csr_from_rows(6, rows)
    return A, (np.array([0, 2, 4, 6], np.int32), np.arange(6, dtype=np.int32))


def ring_pairs(n):
    """Ring of n vertices (n even), uniform weights, consecutive pairs as aggregates;
    built vectorised.  n = 2^22: 22 + 21 + 21 = 64 key bits, the widest single sort;
    n = 2^22 + 2: 23 + 22 + 22 bits, the split sort by width.  No smaller shape of this
    kind reaches 65 bits."""
    i = np.arange(n, dtype=np.int64)
    lo, hi = (i - 1) % n, (i + 1) % n
    ix = np.stack([np.minimum(lo, hi), np.maximum(lo, hi)], axis=1).reshape(-1).astype(np.int32)
    ip = (2 * np.arange(n + 1, dtype=np.int64)).astype(np.int32)
    dx = np.random.RandomState(61).uniform(0.1, 2.0, 2 * n)
    PT = ((2 * np.arange(n // 2 + 1, dtype=np.int64)).astype(np.int32),
          np.arange(n, dtype=np.int32))
    return (ip, ix, dx), PT


KEY_WIDTH = ((1 << 22, False), ((1 << 22) + 2, True))  # (n, split sort by width)


def ptap_small_cases():
    """name -> (A, PT): every small P^T A P case, each compared whole with orc_ptap on
    the single sort and under GE_PTAP_SPLIT_SORT."""
    out = {}
    for wname in WEIGHTS:
        out["graph96_" + wname] = graph96(wname)
    out["first_aggregates_empty"] = graph96("mixed", (0, 0, 5, 40, 0, 51))
    out["only_aggregate0"] = graph96("mixed", (96, 0, 0, 0))
    A, PT, _, _ = empty_rows_graph()
    out["empty_rows"] = (A, PT)
    for where in ("first", "last"):
        out["hub_" + where] = hub_graph(where)[:2]
    out["one_aggregate"] = one_aggregate()
    out["identity"] = identity_pt()
    out["single_vertex"] = single_vertex()
    for n in (64, 65):
        for m in (64, 65):
            out[f"pow2_n{n}_m{m}"] = pow2_graph(n, m)
    out["unsorted_dups"] = unsorted_dups_graph()
    out["zeros"] = zeros_graph()
    return out


# ranges that start or end inside runs of empty aggregates (or both): SIZES96 has the run
# 3, 4 and the empty aggregate 8, hub_graph the run 9, 10
RANGES_IN_EMPTY = {"graph96": ((4, 9), (1, 4), (3, 5)), "hub": ((10, 15), (3, 10), (10, 11))}


def ptap_ranges(m, inside_empty):
    """Row ranges for ge_ptap_rows: the whole, the first and the last row, an empty range,
    and the given ones that start or end inside runs of empty aggregates."""
    return [(0, m), (0, 1), (m - 1, m), (m // 2, m // 2)] + list(inside_empty)


# ---------------------------------------------------------------------------
# graph set-up

# ge_rmat_csr(2, 6, seed): every draw has src == dst (scale 1, one quadrant draw each)
ALL_INVALID = dict(n=2, draws=6, seed=8)
RMAT = dict(n=4096, draws=40000, seed=7)


def rmat_keys(n, draws, seed):
    """Valid directed keys per row (duplicates included), as key_rows_kernel counts."""
    import graphs as G
    s, d = G.rmat_edges(n, draws, seed)
    return np.bincount(np.concatenate([s, d]), minlength=n)


def sort_segments(rowcnt, chunk):
    """rmat_device's greedy cut of the rows into segments of at most chunk valid keys:
    the first row of every segment (None: one row exceeds a chunk)."""
    bound, acc = [0], 0
    for r, c in enumerate(rowcnt.tolist()):
        if c > chunk:
            return None
        if acc + c > chunk:
            bound.append(r)
            acc = 0
        acc += c
    return bound


def scan_calls(count, chunk):
    """Library calls of one exclusive_scan over count items."""
    return 1 if count <= chunk else -(-count // chunk)


def rmat_chunks():
    """name -> chunk for the n = 4096, draws = 40000 R-MAT (80 000 keys)."""
    rc = rmat_keys(**RMAT)
    valid, keys = int(rc.sum()), 2 * RMAT["draws"]
    # all_keys: the single-call path exactly.  all_keys_minus_1: the segmented sort, which
    # drops the invalid keys, so one segment and one-call scans.  valid_minus_1: the valid
    # keys mod chunk is 1 -- two scan chunks, the second of one item (79754 - 1 =
    # 173 * 461 has no other divisor that holds row 0).  4096 also leaves the n + 1 =
    # 4097 row counts' scan a last chunk of one item.
    out = {"twenty": 4096, "all_keys": keys, "all_keys_minus_1": keys - 1,
           "valid_minus_1": valid - 1}
    # a segment that ends in rows without keys: the row before a segment's first has none
    for c in range(int(rc.max()), 8192):
        b = sort_segments(rc, c)
        if any(rc[r - 1] == 0 for r in b[1:]):
            out["boundary_after_empty_row"] = c
            break
    out["below_row0"] = int(rc[0]) - 1
    return out


def lcc_cases():
    """name -> (A, chunk): inputs of ge_largest_component_device, each run without and
    with GE_GRAPH_CHUNK = chunk (both scans in chunks)."""
    out = {}
    e = np.zeros(0, np.int32)
    out["n0"] = ((np.zeros(1, np.int32), e, np.zeros(0)), 1)
    out["n1"] = ((np.zeros(2, np.int32), e, np.zeros(0)), 1)
    out["edgeless5"] = ((np.zeros(6, np.int32), e, np.zeros(0)), 1)
    n = 4097  # 64 * 64 + 1: the last chunk of 64 has one item
    path = [(i, i + 1) for i in range(n - 1)]
    out["path_ascending"] = (sym_csr(n, path), 64)
    p = np.random.RandomState(71).permutation(n)
    out["path_permuted"] = (sym_csr(n, [(int(p[i]), int(p[i + 1])) for i in range(n - 1)]), 64)
    # {1,2,3} has the smaller edges; {0,8,9} holds vertex 0 and wins the tie
    out["tie_vertex0_second"] = (sym_csr(10, [(1, 2), (2, 3), (8, 9), (0, 9), (4, 5)]), 3)
    out["isolated_last"] = (sym_csr(7, [(0, 1), (1, 2), (3, 4)]), 2)
    out["self_loops"] = (sym_csr(6, [(0, 0), (0, 1), (2, 2), (3, 4), (4, 5), (5, 5), (3, 5)]), 2)
    edges = [(0, 3), (3, 5), (1, 2), (5, 6), (2, 4), (4, 1)]
    out["weights"] = (sym_csr(7, edges, np.arange(1, 13) * 0.37), 3)
    out["connected"] = (sym_csr(300, [(i, (i * 7 + 1) % 300) for i in range(300)
                                      if i != (i * 7 + 1) % 300] +
                                [(i, i + 1) for i in range(299)]), 50)
    return out


# ---------------------------------------------------------------------------
# modularity

def modularity_cases():
    """name -> (A, vertex_A, m).  Weights of 2^31 and above are left out: the reference's
    `int a_ij = D[k]` is undefined for them."""
    out = {}
    # -0.9 -> 0, -1.5 -> -1: aggregate 0's in sum and aggregate 1's out sum are negative
    rows = [[(1, -1.5), (2, 0.9)], [(0, -1.5), (3, -0.9)], [(0, -2.5), (3, 7.0)],
            [(2, 7.0), (1, -0.9), (0, -1.5)]]
    out["negative_fractional"] = (csr_from_rows(4, rows), np.array([0, 0, 1, 1], np.int32), 2)
    # 5000 entries of 2^30 inside aggregate 0: past 2^32, below 2^53
    n = 101
    edges = [(i, j) for i in range(n - 1) for j in range(i + 1, min(i + 26, n - 1))]
    w = np.full(2 * len(edges) + 2, 2.0 ** 30)
    w[-2:] = 3.0
    out["large_sums"] = (sym_csr(n, edges + [(0, n - 1)], w),
                         np.array([0] * (n - 1) + [1], np.int32), 2)
    # 2147483647.9 -> 2^31 - 1
    rows = [[(1, 2147483647.9), (2, 5.0)], [(0, 2147483647.9)], [(0, 5.0), (3, 2147483647.9)],
            [(2, 2147483646.5)]]
    out["int_limit"] = (csr_from_rows(4, rows), np.array([0, 0, 1, 1], np.int32), 2)
    edges = random_graph(30, 0.3, 81)
    A = sym_csr(30, edges, uniform_weights(2 * len(edges), 82) * 3)
    lab = np.random.RandomState(83).randint(0, 4, 30).astype(np.int32) * 2  # labels 0, 2, 4, 6
    out["unused_aggregates"] = (A, lab, 9)
    out["single_aggregate"] = (A, np.zeros(30, np.int32), 1)
    return out


# ---------------------------------------------------------------------------
# radius step

def equal_time_pairs(case):
    """Pairs of events with equal start times (what the (t, i, j) tie-break orders)."""
    cA, dim, base, PTc, cAc, rAc, Ac = case
    m = len(cA)
    if base:
        i, j = np.triu_indices(m, 1)
    else:
        grp = np.empty(m, np.int64)
        for b in range(len(PTc[0]) - 1):
            grp[PTc[1][PTc[0][b]:PTc[0][b + 1]]] = b
        i = np.repeat(np.arange(m), np.diff(Ac[0]))
        j = Ac[1].astype(np.int64)
        keep = (i < j) & (grp[i] == grp[j])
        i, j = i[keep], j[keep]
    d = np.sqrt(((cA[i] - cA[j]) ** 2).sum(axis=1))
    _, c = np.unique(d, return_counts=True)
    return int((c * (c - 1) // 2).sum()), len(d)


def _lattice(dim, side):
    g = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), -1).reshape(-1, dim)
    return g.astype(np.float64)


def _grouped(cA, groups, edges, seed, dim):
    """A non-base case: groups (lists of members in P_T order) over the graph `edges`."""
    m = len(cA)
    pip = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    pix = np.array([v for g in groups for v in g], np.int32)
    rs = np.random.RandomState(seed)
    cAc = rs.uniform(-1.0, 1.0, (len(groups), dim))
    rAc = rs.uniform(0.1, 1.0, len(groups))
    Ac = sym_csr(m, edges)
    return (cA, dim, False, (pip, pix), cAc, rAc, (Ac[0], Ac[1]))


def _grid(w, h, perm_seed=None):
    ids = np.arange(w * h)
    if perm_seed is not None:
        ids = np.random.RandomState(perm_seed).permutation(w * h)
    v = lambda x, y: int(ids[y * w + x])  # noqa: E731
    cA = np.zeros((w * h, 2))
    edges = []
    for y in range(h):
        for x in range(w):
            cA[v(x, y)] = (x, y)
            if x + 1 < w:
                edges.append((v(x, y), v(x + 1, y)))
            if y + 1 < h:
                edges.append((v(x, y), v(x, y + 1)))
    return cA, edges, v


def radius_tie_cases():
    """name -> (cA, dim, base, PTc, cAc, rAc, Ac): integer lattices, where hundreds of
    events start at equal times.  They guard progress and the handling of the (t, i, j)
    tuples; by the confluence of these inputs (which of two tied events pops first
    changes no bit) they do not guard the value against a different tie-break."""
    out = {}
    for dim, side in ((1, 24), (2, 5), (3, 3), (5, 2)):
        cA = _lattice(dim, side)
        cA = cA[np.random.RandomState(dim).permutation(len(cA))]
        out[f"lattice_d{dim}"] = (cA, dim, True, None, None, None, None)
    for perm in (None, 91):
        tag = "" if perm is None else "_permuted"
        cA, edges, v = _grid(12, 10, perm)
        out["grid_one_group" + tag] = _grouped(cA, [list(range(120))], edges, 92, 2)
        bands = [[v(x, y) for y in range(y0, y0 + 2) for x in range(12)] for y0 in range(0, 10, 2)]
        out["grid_bands" + tag] = _grouped(cA, bands, edges, 93, 2)
    # a star with equal spokes: the hub at the origin of 16 dimensions, leaves 0..31 at
    # +- e_k (distance 1) and 32..39 at 2 e_k (distance 2) -- two shells of equal spokes
    k = 40
    star = np.zeros((k + 1, 16))
    for q in range(k):
        star[q + 1, q % 16] = (1.0 if (q // 16) % 2 == 0 else -1.0) * (1 + q // 32)
    out["star_equal_spokes"] = _grouped(star, [list(range(k + 1))],
                                        [(0, q + 1) for q in range(k)], 94, 16)
    # duplicate CSR entries: every edge of a lattice path stored twice
    cA = _lattice(1, 30)
    Ac = csr_from_rows(30, [[(c, 1.0) for c in (i - 1, i - 1, i + 1, i + 1) if 0 <= c < 30]
                            for i in range(30)])
    rs = np.random.RandomState(95)
    out["duplicate_entries"] = (cA, 1, False, (np.array([0, 30], np.int32),
                                               np.arange(30, dtype=np.int32)),
                                rs.uniform(-1, 1, (1, 1)), rs.uniform(0.1, 1.0, 1),
                                (Ac[0], Ac[1]))
    return out


CLAMP = 0.000001  # the rescale's lower bound on alpha (ge_radius.hip rescale_kernel)


def radius_clamp_case():
    """Singleton groups whose member sits exactly on the group's centre, so alpha = r_Ac:
    0 (clamped), just below 1e-6 (clamped), 1e-6 itself and just above (not clamped);
    then a pair group as the ordinary case."""
    rAc = np.array([0.0, np.nextafter(CLAMP, 0.0), CLAMP, np.nextafter(CLAMP, 1.0), 0.5])
    cAc = np.random.RandomState(101).uniform(-1, 1, (5, 3))
    cA = np.vstack([cAc[:4], cAc[4] + [0.1, 0.2, 0.3], cAc[4] - [0.3, 0.1, 0.2]])
    pip = np.array([0, 1, 2, 3, 4, 6], np.int32)
    Ac = sym_csr(6, [(4, 5), (0, 1), (2, 4)])
    return (cA, 3, False, (pip, np.arange(6, dtype=np.int32)), cAc, rAc, (Ac[0], Ac[1]))


def radius_underflow_case(dim):
    """Two adjacent members of one group differ by 1e-170 in one coordinate: the square
    underflows, d == 0, and the device call hands over to the host loop."""
    m = 12
    cA = np.random.RandomState(111).uniform(-1, 1, (m, dim))
    cA[7] = cA[3]
    cA[7, dim - 1] = 0.0
    cA[3, dim - 1] = 1e-170
    edges = [(i, i + 1) for i in range(m - 1)] + [(3, 7)]
    return _grouped(cA, [list(range(6, 12)) + list(range(0, 6))], edges, 112, dim)


GROUP_SIZES = (1, 2, 63, 64, 65, 128, 129)  # on the wave's 64-lane stride
LAST_SETS_ALPHA, R_DECIDES = 4, 2           # groups (of 65 and of 63 members)


def radius_group_sizes_case(dim, extra_singleton):
    """One level with groups of GROUP_SIZES members (mc = 7; with one more singleton
    mc = 8, on either side of the four groups per block).  Group 4 (65 members: lane 0
    takes a second member): the last member in P_T order lies far out and sets alpha.
    Group 2: all members but one sit close together near (1, 0, ..), so their r is small;
    the odd one lies nearer to the centre but far from them, its r is large, and r
    rather than the distance decides the maximum."""
    sizes = list(GROUP_SIZES) + ([1] if extra_singleton else [])
    m = sum(sizes)
    rs = np.random.RandomState(121 + dim)
    perm = rs.permutation(m)
    groups, at = [], 0
    for s in sizes:
        groups.append([int(x) for x in perm[at:at + s]])
        at += s
    cA = rs.uniform(-1.0, 1.0, (m, dim))
    edges = []
    for g in groups:
        edges += [(g[q], g[q + 1]) for q in range(len(g) - 1)]
        edges += [(g[q], g[(q * 5 + 3) % len(g)]) for q in range(len(g))
                  if g[q] != g[(q * 5 + 3) % len(g)]]
    edges += [(groups[q][0], groups[q + 1][0]) for q in range(len(groups) - 1)]  # ignored
    edges = sorted({(min(a, b), max(a, b)) for a, b in edges})
    case = _grouped(cA, groups, edges, 122, dim)
    cAc = case[4]
    cAc[R_DECIDES] = 0.0
    g = groups[R_DECIDES]
    cA[g] = rs.uniform(-0.05, 0.05, (len(g), dim))
    cA[g, 0] += 1.0
    cA[g[10]] = 0.0
    cA[g[10], 0] = -0.9
    g = groups[LAST_SETS_ALPHA]
    cA[g[-1]] = cAc[LAST_SETS_ALPHA]
    cA[g[-1], 0] += 10.0
    return case, groups


def oracle_radius(oracle, cA, dim, base, PTc=None, cAc=None, rAc=None, Ac=None):
    """orc_radius_step: (r_A, coords_A after the rescale)."""
    m = cA.shape[0]
    cc = np.ascontiguousarray(cA.copy()).reshape(-1)
    rr = np.zeros(m)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if base:
        oracle.lib().orc_radius_step(m, cc, rr, dim, 1, 0, None, None, None, None,
                                     np.zeros(1, np.int32), np.zeros(1, np.int32))
    else:
        pip = np.ascontiguousarray(PTc[0], np.int32)
        pix = np.ascontiguousarray(PTc[1], np.int32)
        cAc = np.ascontiguousarray(cAc)
        rAc = np.ascontiguousarray(rAc)
        oracle.lib().orc_radius_step(m, cc, rr, dim, 0, len(pip) - 1, vp(pip), vp(pix), vp(cAc),
                                     vp(rAc), np.ascontiguousarray(Ac[0], np.int32),
                                     np.ascontiguousarray(Ac[1], np.int32))
    return rr, cc.reshape(m, dim)
