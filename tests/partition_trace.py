"""The reference's partition round loop (src/partitioner.cpp:1550-1893, and the
one-level overloads :970-1266 / :1272-1544) restated in Python, returning what
the compiled reference does not: the quotient graph and alpha the loop ends with.

Python floats are IEEE doubles and nothing here is contracted or reordered, so
every sum has the reference's expression tree: the row sums and T serially in
storage order (:1563-1596), eta = 2 * (a_ij / T - alpha_i * alpha_j) (:1715), and
the contraction's `a[i'][k] += a_jk; a[k][i'] += a_jk` in `merged` order
(:1756-1779).  tests/test_partition_real_weights.py pins the P_T arrays it
returns to the oracle's.

reverse=True processes the contraction's merges in reverse: the same terms in a
wrong grouping.  It exists only to show that a test can see the summation order.
tie_last=True lets the scan take the last of several maximal neighbours (`>=`):
a wrong index tie-break, to show that a test can see the right one.  log, a list,
receives each round's merges as (keeper, absorbed) pairs in `merged` order.
"""
import numpy as np

INF = float("inf")


def weights_from(A, values):
    """Symmetric weights from `values`, by hashing (min, max) as
    ref_cases.symmetric_weights does."""
    ip, ix, _ = A
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    pick = (np.minimum(rows, ix).astype(np.int64) * 7 + np.maximum(rows, ix) * 13) % len(values)
    return ip, ix, np.asarray(values, dtype=np.float64)[pick]


def _interpolation(num_cols, sets):
    ip = np.zeros(len(sets) + 1, dtype=np.int32)
    ip[1:] = np.cumsum([len(s) for s in sets])
    ix = np.array([y for s in sets for y in s], dtype=np.int32)
    return ip, ix, len(sets), num_cols


def trace(A, cf=None, num_parts=None, positive_merging=True, stall=1.0, matching=2,
          reverse=False, tie_last=False, log=None):
    """cf: the hierarchy overload; num_parts: the numParts overload; neither: the
    single-P_T overload.  Returns (levels, final_graph, final_alpha): levels as
    (indptr, indices, rows, cols); final_graph the CSR of a[i][k] over the alive
    vertices by `used` slot, columns ascending; final_alpha by `used` slot."""
    I, J, D = (np.asarray(x).tolist() for x in A)
    n = len(I) - 1
    N = M = n
    a = [dict() for _ in range(n)]
    alpha = [0.0] * n
    for i in range(n):
        s = 0.0
        for e in range(I[i], I[i + 1]):
            if J[e] != i:
                a[i].setdefault(J[e], D[e])
            s += D[e]
        alpha[i] = s
    T = 0.0
    for e in range(I[n]):
        T += D[e]
    for i in range(n):
        alpha[i] /= T

    basis = list(range(n))
    used = list(range(n))
    pointer = list(range(n))
    ident = list(range(n))

    def find(i):
        root = i
        while ident[root] != root:
            root = ident[root]
        while ident[i] != root:
            ident[i], i = root, ident[i]
        return root

    def snapshot():
        sets = [[] for _ in range(M)]
        for y, i in enumerate(basis):
            sets[pointer[find(i)]].append(y)
        return _interpolation(N, sets)

    max_eta = [-INF] * n
    max_ind = [-1] * n
    notouch = [False] * n
    levels = []
    while True:
        merged = []
        for _ in range(matching):
            for i in used:
                if not notouch[i] or max_eta[i] == -INF:
                    best, arg = -INF, -1
                    ai = alpha[i]
                    for j in sorted(a[i]):
                        if not notouch[j]:
                            eta = 2 * (a[i][j] / T - ai * alpha[j])
                            if eta > best or (tie_last and eta >= best):
                                best, arg = eta, j
                    max_eta[i], max_ind[i] = best, arg
            for i in used:
                if notouch[i]:
                    continue
                j = max_ind[i]
                if j != -1 and not notouch[j] and not (max_eta[i] < max_eta[j]):
                    if not positive_merging or max_eta[i] > 0:
                        merged.append((j, i) if len(a[i]) < len(a[j]) else (i, j))
                        notouch[i] = notouch[j] = True
        if log is not None:
            log.append(list(merged))
        for ip_, jp in (reversed(merged) if reverse else merged):
            for k in sorted(a[jp]):
                a_jk = a[jp][k]
                del a[k][jp]
                max_eta[k] = -INF
                if k == ip_:
                    alpha[ip_] = alpha[ip_] + alpha[jp]
                else:
                    a[ip_][k] = a[ip_].get(k, 0.0) + a_jk
                    a[k][ip_] = a[k].get(ip_, 0.0) + a_jk
        M_prev = M
        if cf is not None and 1.0 * M / N <= cf:
            levels.append(snapshot())
            basis = list(used)
            N = M
        for ip_, jp in merged:
            idx = pointer[jp]
            k = used[-1]
            used[idx], used[-1] = used[-1], used[idx]
            used.pop()
            pointer[k] = idx
            ident[jp] = ip_
            notouch[ip_] = False
            M -= 1
        more = 1.0 * M / M_prev < stall
        if cf is None and num_parts is not None:
            more = more and M > num_parts
        if not more:
            break
    levels.append(snapshot())

    fip = np.zeros(M + 1, dtype=np.int32)
    fix, fdx = [], []
    for x, i in enumerate(used):
        row = sorted((pointer[k], w) for k, w in a[i].items())
        fix += [c for c, _ in row]
        fdx += [w for _, w in row]
        fip[x + 1] = len(fix)
    final_graph = (fip, np.array(fix, dtype=np.int32), np.array(fdx, dtype=np.float64))
    final_alpha = np.array([alpha[i] for i in used], dtype=np.float64)
    return levels, final_graph, final_alpha


# -- the inputs of tests/test_partition_real_weights.py and its GPU counterpart ---

W3 = (0.1, 0.2, 0.3)
W5 = (0.1, 0.2, 0.3, 0.7, 1.1)
CF = 0.125
_cache = {}


def graph(name):
    import graphs as G
    if name not in _cache:
        _cache[name] = {
            "er600": lambda: G.erdos_renyi(600, 0.02, seed=3),
            "rmat1500": lambda: G.largest_component(G.rmat(1500, 9000, seed=9)),
            "rmat600": lambda: G.largest_component(G.rmat(600, 3000, seed=3)),
        }[name]()
    return _cache[name]


def with_diagonal(A, every, value):
    """A plus a diagonal entry `value` on every `every`-th vertex, rows ascending."""
    ip, ix, dx = A
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    assert not (rows == ix).any()
    dr = np.arange(0, n, every)
    r = np.concatenate([rows, dr])
    c = np.concatenate([ix, dr])
    w = np.concatenate([dx, np.full(len(dr), value)])
    order = np.lexsort((c, r))
    nip = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return nip, c[order].astype(np.int32), w[order]


def traced(name, values, reverse=False, **kw):
    """trace() of graph(name) with weights_from(values), computed once per case."""
    key = (name, values, reverse, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = trace(weights_from(graph(name), values), reverse=reverse, **kw)
    return _cache[key]
