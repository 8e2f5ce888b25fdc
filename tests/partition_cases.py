"""Directed inputs for the device partition (graph-embed_amd/csrc/ge_partition_dev.hip):
one family per group of kernel classes, each sitting on the thresholds at which
the code takes another path.  numpy only; tests/test_partition_cases.py checks the
constructions on the CPU, tests/test_gpu_partition_paths.py runs them on the
device with the census (ge_partition_census) asserting which path ran.

What the constructions rest on:

  * a vertex's round-1 list is its CSR row without the diagonal, in order, so
    list position p holds the p-th neighbour by id;
  * the scan's order is (eta descending, index ascending), eta = 2 (a_ij / T -
    alpha_i alpha_j);
  * vertices with the same weights and weighted degrees have exactly equal eta;
  * the resolve walks the proposers in `used` order, which in round 1 is id order,
    so the vertex with the smallest id gets its choice;
  * of two merging vertices the one with the longer list keeps (ties: the proposer).

Star-like graphs merge one leaf per round for ever under stall = 1.0.  Every
family therefore gives the neighbours partners of their own (coupled by heavy
edges, so that they pair off in round 1) and is run with stall = 0.9 (STALL) or
for one round through partition_single(num_parts = n).
"""
import numpy as np

import partition_trace as T

STALL = 0.9
CF = 0.6  # the scan family halves in round 1: a level is recorded before round 2

# thresholds of ge_partition_dev.hip (kSmallLen .. kSpecMerges)
SMALL_LEN, MID_LEN, BIG_LEN, HUGE_CHUNKS = 16, 512, 16384, 64
WAVE_NEED, BLOCK_NEED, BLOCK_NEED_ORD = 64, 2048, 1024
PATCH_MIN, PATCH_GONE = 2048, 1024
LOCAL_CAND = 1024
SPEC_MERGES = 4096

W3 = T.W3
W_HEAVY = (1.1, 1.3, 1.7)


def csr(n, src, dst, w):
    """Symmetric CSR, rows ascending, of the undirected edges (src, dst, w), each
    given once."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    w = np.asarray(w, np.float64)
    assert len(src) == len(dst) == len(w) and (src != dst).all()
    r = np.concatenate([src, dst])
    c = np.concatenate([dst, src])
    ww = np.concatenate([w, w])
    order = np.lexsort((c, r))
    r, c, ww = r[order], c[order], ww[order]
    key = r * n + c
    assert (np.diff(key) > 0).all(), "duplicate edge"
    ip = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return ip, c.astype(np.int32), ww


def row(A, v):
    """Row v as (columns, weights)."""
    ip, ix, dx = A
    return ix[ip[v]:ip[v + 1]], dx[ip[v]:ip[v + 1]]


def lengths(A):
    """Round-1 list lengths: the row lengths without diagonal entries."""
    ip, ix, _ = A
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    return np.diff(ip) - np.bincount(rows[rows == ix], minlength=n)


def scan_class(length):
    if length <= SMALL_LEN:
        return "scan_small"
    if length <= MID_LEN:
        return "scan_mid"
    return "scan_big" if length <= BIG_LEN else "scan_huge"


# ---- scan family ----------------------------------------------------------------
# Hub 0 with the leaves 1..L: list position p holds leaf p + 1.  The ordinary
# leaves are coupled in consecutive pairs by a heavier edge (an odd one out gets
# a partner outside the hub's list), so each prefers its mate and all of them
# pair off in round 1.  The special leaves have the hub as their only neighbour:
# the smallest alpha among the hub's neighbours, so the largest eta; two of them
# have identical rows and exactly equal eta.  The hub proposes first and merges
# with the special leaf its scan returns, which shows in P_T.  Round 2 is a star
# (one merge), which ends the loop under STALL.

SCAN_LENGTHS = (16, 17, 512, 513, 16384, 16385, 64 * 4096 + 1)


def chunk_edge(L, k):
    """The positions on either side of the boundary between huge-scan chunks k - 1
    and k (scan_huge_part_kernel: chunk k is [L k / 64, L (k + 1) / 64))."""
    e = L * k // HUGE_CHUNKS
    return e - 1, e


def scan_ties(L):
    """Position pairs of the two maximal neighbours, by what the pair straddles;
    None: a single maximum in the last position."""
    out = {"ends": (0, L - 1), "last": None}
    if L > 64:
        out["waves"] = (63, 64)
    if L > 256:
        out["stride256"] = (255, 256)
    if L > 1024:
        out["stride1024"] = (1023, 1024)
    if L > BIG_LEN:
        out["chunks"] = chunk_edge(L, 37)
    return out


def scan_cases(real=False):
    """(label, L, tie) of every scan case: every tie of every length, the same
    with integer and with real weights (`real` only keeps the two call sites alike)."""
    return [(f"L{L}-{name}", L, tie) for L in SCAN_LENGTHS for name, tie in scan_ties(L).items()]


def scan_special(L, tie):
    return [L] if tie is None else [tie[0] + 1, tie[1] + 1]


def scan_case(L, tie, real=False):
    special = scan_special(L, tie)
    ordinary = np.setdiff1d(np.arange(1, L + 1), special)
    n = L + 1
    a, b = ordinary[0:-1:2], ordinary[1::2]
    if len(ordinary) % 2:
        b = np.append(b, n)  # the odd one out: a partner of its own outside the list
        a = np.append(a[:len(b) - 1], ordinary[-1])
        n += 1
    assert len(a) == len(b)
    hub_src = np.zeros(L, np.int64)
    hub_dst = np.arange(1, L + 1)
    A = csr(n, np.concatenate([hub_src, a]), np.concatenate([hub_dst, b]),
            np.concatenate([np.ones(L), np.full(len(a), 2.0)]))
    if not real:
        return A
    # real weights on the non-tied edges: light ones to the hub, heavy ones between
    # mates; the special leaves keep the largest light value, so their eta
    # 2 w (1 - alpha_hub) / T stays the strict maximum (every other neighbour has
    # w' <= w and a larger alpha)
    ip, ix, _ = A
    rows = np.repeat(np.arange(n), np.diff(ip))
    light, heavy = T.weights_from(A, W3)[2], T.weights_from(A, W_HEAVY)[2]
    to_hub = (rows == 0) | (ix == 0)
    w = np.where(to_hub, light, heavy)
    spec = to_hub & (np.isin(rows, special) | np.isin(ix, special))
    w[spec] = max(W3)
    return ip, ix, w


# ---- rebuild family -------------------------------------------------------------
# Coupled pairs (u, g) with private leaves: u has lu - 1 of them, g has lg - 1,
# lu > lg, so u keeps and the rebuild of its list needs lu + lg slots.  The
# coupling weight 4 (lu + lg) keeps eta(u, g) positive and far above the leaves'.
# g's leaves see their neighbour renamed and are rebuilt too (need 1); u's are not.

REBUILD_NEEDS = (WAVE_NEED, WAVE_NEED + 1, BLOCK_NEED, BLOCK_NEED + 1)
REBUILD_NEEDS_REAL = (WAVE_NEED, WAVE_NEED + 1, BLOCK_NEED_ORD, BLOCK_NEED_ORD + 1, BLOCK_NEED + 1)


def rebuild_case(needs, real=False):
    """Returns (A, pairs): pairs as (u, g, need)."""
    src, dst, w, pairs = [], [], [], []
    n = 0
    for need in needs:
        lg = need // 2 - 1
        lu = need - lg
        u, g = n, n + 1
        n += 2
        src.append(u), dst.append(g), w.append(4.0 * need)
        for v, cnt in ((u, lu - 1), (g, lg - 1)):
            for _ in range(cnt):
                src.append(v), dst.append(n), w.append(1.0)
                n += 1
        pairs.append((u, g, need))
    A = csr(n, src, dst, w)
    if real:
        ip, ix, dx = A
        A = ip, ix, np.where(dx == 1.0, T.weights_from(A, W3)[2], dx + 0.5)
    return A, pairs


def rebuild_class(need, ordered):
    if need <= WAVE_NEED:
        return "rebuilt_wave"
    return "rebuilt_block" if need <= (BLOCK_NEED_ORD if ordered else BLOCK_NEED) else "rebuilt_global"


def rebuild_classes(A, merges, ordered):
    """Lists per rebuild class of round 1's contraction, from its merges as
    (keeper, absorbed) pairs (partition_trace.trace(log=...)[0]): a keeper's table
    needs the sum of the two list lengths, every other alive neighbour of an
    absorbed vertex its own length (classify_kernel).  Hub patches are not
    subtracted."""
    ip, ix, _ = A
    ln = lengths(A)
    gone = {j for _, j in merges}
    need = {i: int(ln[i] + ln[j]) for i, j in merges}
    for _, j in merges:
        for k in ix[ip[j]:ip[j + 1]]:
            k = int(k)
            if k != j and k not in gone and k not in need:
                need[k] = int(ln[k])
    out = {"rebuilt_wave": 0, "rebuilt_block": 0, "rebuilt_global": 0}
    for v in need.values():
        out[rebuild_class(v, ordered)] += 1
    return out


# ---- patch family (integer weights) ----------------------------------------------
# Hub 0 with the neighbours 1..Lh, in list order:
#   g        (optional) the hub's own partner: the hub's argmax, and the hub g's
#            (glen = 1: a leaf; longer: a heavy edge, and glen - 1 of the hub's
#            `keeper` neighbours as g's other entries, so its renamed entries land
#            on keys the hub already has; private > 0 adds leaves of g's own, new
#            keys for the hub)
#   g2       (optional) a second such neighbour with a lighter edge and private
#            leaves: the hub's partner of round 2
#   mates    front pairs of neighbours coupled to each other: the second of each
#            pair is absorbed (a deletion without a new key)
#   absorbed K neighbours a, each coupled to b outside the list; b has three
#            leaves and the longer list, so b keeps and a is absorbed: the hub's
#            entry a is renamed to b (a deletion and a new key)
#   keepers  neighbours r coupled to a leaf outside: r keeps, the hub sees nothing
#   mates    back pairs, at the end of the list
# Every neighbour prefers its coupling (weight 4) to the hub (weight 1), so all of
# them merge in round 1, and the hub, whose best neighbour prefers another, does
# not merge unless it has g.

G_HEAVY, G2_HEAVY = 2000.0, 1500.0


def patch_case(Lh, K, glen=0, private=0, g2_private=0, front=0, back=0):
    """Returns (A, info): info["absorbed"] the hub neighbours absorbed in round 1,
    info["g"] the hub's partner or None."""
    src, dst, w = [], [], []
    nxt = [Lh + 1]

    def fresh():
        nxt[0] += 1
        return nxt[0] - 1

    def edge(a, b, x):
        src.append(a), dst.append(b), w.append(x)

    order = list(range(1, Lh + 1))
    g = order.pop(0) if glen else None
    g2 = order.pop(0) if g2_private else None
    fm = [order.pop(0) for _ in range(2 * front)]
    ab = [order.pop(0) for _ in range(K)]
    bm = [order.pop() for _ in range(2 * back)][::-1]
    keepers = order
    absorbed = list(ab)
    for v in range(1, Lh + 1):
        edge(0, v, 1.0)
    if g is not None and (glen > 1 or private):
        w[g - 1] = G_HEAVY
        assert glen - 1 <= len(keepers)
        for r in keepers[:glen - 1]:
            edge(g, r, 1.0)
        for _ in range(private):
            edge(g, fresh(), 1.0)
    if g2 is not None:
        w[g2 - 1] = G2_HEAVY
        for _ in range(g2_private):
            edge(g2, fresh(), 1.0)
    for m in (fm, bm):
        for a1, a2 in zip(m[0::2], m[1::2]):
            edge(a1, a2, 4.0)
            absorbed.append(a2)
    for a in ab:
        b = fresh()
        edge(a, b, 4.0)
        for _ in range(3):
            edge(b, fresh(), 1.0)
    for r in keepers:
        edge(r, fresh(), 4.0)
    A = csr(nxt[0], src, dst, w)
    return A, {"absorbed": sorted(absorbed), "g": g, "g2": g2}


# label -> (patch_case arguments, census fields the one-round run must show);
# fields not named among patched / patch_* must be 0
PATCH_ROUND1 = {
    # absorbed neighbours against kPatchGone, the hub not merging ...
    "K1023": (dict(Lh=2049, K=1023), dict(patched=1)),
    "K1024": (dict(Lh=2049, K=1024), dict(patched=1)),
    "K1025": (dict(Lh=2049, K=1025), dict(patch_size=1)),
    # ... and keeping a merge of its own (its partner's entry is one more deletion)
    "K1022-merging": (dict(Lh=2049, K=1022, glen=1), dict(patched=1)),
    "K1023-merging": (dict(Lh=2049, K=1023, glen=1), dict(patched=1)),
    "K1024-merging": (dict(Lh=2049, K=1024, glen=1), dict(patch_size=1)),
    # the partner's list against kPatchGone
    "partner1024": (dict(Lh=2100, K=8, glen=1024), dict(patched=1)),
    "partner1025": (dict(Lh=2100, K=8, glen=1025), dict(patch_size=1)),
    # the hub's list against kPatchMin: 2 048 entries are no hub (block table, or the
    # global one when the partner's entries come on top)
    "hub2048": (dict(Lh=2048, K=8), dict()),
    "hub2048-merging": (dict(Lh=2048, K=8, glen=1), dict(patch_short=1)),
    # deletions outnumber the new keys; the list shrinks by 16 to 2 084, with 8 holes
    # below the new end and 8 above it
    "holes": (dict(Lh=2100, K=40, front=8, back=8), dict(patched=1)),
    # new keys outnumber the deletions while the capacity is the row length
    "grow": (dict(Lh=2100, K=8, glen=1, private=3), dict(patch_fit=1)),
}
# the multi-round case: no room in round 1 (rebuilt with slack), patched past the
# old end in round 2, when the hub merges with g2 and takes its private leaves
PATCH_GROW = dict(Lh=2100, K=8, glen=1, private=3, g2_private=5)


# ---- matching family --------------------------------------------------------------

# (1 031 and 1 032 vertices hand exactly 1 024 and 1 025 candidates to the
# single-block matching, handed_to_resolve: the two sides of kLocalCand)
MATCH_PATHS = (1024, 1025, 1031, 1032, 2049, 5000)


def path_case(n):
    """Unit-weight path: vertex i proposes to i - 1, and the greedy matching
    depends on the whole chain."""
    return csr(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1))


def handed_to_resolve(A):
    """Candidates of round 1, pass 0 that the single-block matching receives: the
    candidate edges (i, max_ind[i]) with !(max_eta[i] < max_eta[j]) and a positive
    eta, less those that the first locally-dominant round over the whole grid
    (resolve_min / select / filter) takes or kills."""
    ip, ix, dx = (np.asarray(x).tolist() for x in A)
    n = len(ip) - 1
    T_ = 0.0
    for e in range(ip[n]):
        T_ += dx[e]
    alpha = [sum(dx[ip[i]:ip[i + 1]]) / T_ for i in range(n)]
    best, arg = [-T.INF] * n, [-1] * n
    for i in range(n):
        for e in range(ip[i], ip[i + 1]):
            j = ix[e]
            eta = 2 * (dx[e] / T_ - alpha[i] * alpha[j])
            if j != i and eta > best[i]:
                best[i], arg[i] = eta, j
    cand = [i for i in range(n) if arg[i] >= 0 and best[i] > 0 and not best[i] < best[arg[i]]]
    lock = {}
    for i in cand:  # rank = id in round 1
        for v in (i, arg[i]):
            lock[v] = min(lock.get(v, n), i)
    taken = set()
    for i in cand:
        if lock[i] == i and lock[arg[i]] == i:
            taken.update((i, arg[i]))
    return sum(1 for i in cand if i not in taken and arg[i] not in taken)


def crowd_case(hubs=4, leaves=1500):
    """`leaves` leaves on each of a few hubs (the hubs in a chain): every leaf is a
    candidate pointing at its hub."""
    src, dst = [], []
    n = hubs
    for h in range(hubs):
        if h:
            src.append(h - 1), dst.append(h)
        src += [h] * leaves
        dst += list(range(n, n + leaves))
        n += leaves
    return csr(n, src, dst, np.ones(len(src)))


# ---- pool family --------------------------------------------------------------------

def pool_case(n=20000, degree=8, seed=20):
    """n vertices, n degree / 2 uniformly drawn edges (duplicates dropped)."""
    import graphs as G
    rs = np.random.RandomState(seed)
    s, d = rs.randint(0, n, n * degree // 2), rs.randint(0, n, n * degree // 2)
    return G.csr_from_edges(n, s[s != d], d[s != d])


# ---- a scan shortcut on an equal bound ----------------------------------------------
# classify_scan_kernel keeps, for an untouched vertex whose argmax was touched, the
# runner-up k2 of its last pass-0 scan when eta(k2) now exceeds the bound b3 that
# scan recorded for the remaining entries.  On equality a remaining entry with a
# smaller id wins the rescan, so the comparison must be strict.  Here T is a power
# of two and the weights are integers, so every alpha and eta is exact:
#   round 1: u = 0 records argmax a, runner-up k2 (weighted degree 5) and
#            b3 = eta(u, x) (x: degree 8, id below k2's).  a pairs with a', k2
#            absorbs its leaf p (degree 5 + 3 = 8: eta(u, k2) now equals b3), x is
#            turned down by z and stays as it is; u is turned down by a and by x.
#   round 2: u keeps a by the pass-0 bound; a pairs with a''; in pass 1 u's runner-up
#            k2 is untouched with eta(u, k2) == b3: the rescan takes x, and u merges
#            with x.  A non-strict comparison would merge u with k2.

def equal_bound_case():
    u, a, x, k2, a1, a2, p, z, z2, z3, z4, pad0, pad1 = range(13)
    edges = [(u, a, 3), (u, x, 2), (u, k2, 2), (a, a1, 6), (a, a2, 5), (k2, p, 3), (x, z, 6),
             (z, z2, 9), (z2, z3, 12), (z, z4, 7)]
    total = 2 * sum(e[2] for e in edges)
    edges.append((pad0, pad1, (4096 - total) // 2))
    assert 2 * sum(e[2] for e in edges) == 4096
    s, d, w = zip(*edges)
    return csr(13, s, d, w)
