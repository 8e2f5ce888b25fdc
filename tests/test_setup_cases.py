"""The inputs of tests/setup_cases.py have the properties they are named for, and the host
paths agree with the oracle on them (CPU only; tests/test_gpu_setup.py runs the same
inputs on the device).

P^T A P: the counts of empty aggregates and rows, the key widths from a restatement of
bits_below, duplicate columns, and -- for the two order-sensitive graphs -- that each of
four wrong summation orders differs from orc_ptap in at least one entry, so a device
result in a wrong order cannot pass.  Graph set-up: the pinned all-invalid seed, the
segment and chunk counts the chunked runs must report, host R-MAT against its numpy
definition, host LCC against the DFS of tests/graphs.py.  Modularity: the truncated sums
the cases are built for, host against oracle.  Radius: how many equal-time pairs each
tie input has, which member sets alpha, and the host loop against the oracle on every
case (it is what the underflow case falls back to).
"""
import numpy as np
import pytest

import ge_amd as ge
import graphs as G
import setup_cases as S
from setup_cases import oracle_radius

_small = S.ptap_small_cases()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# P^T A P

def _check_pt(A, PT):
    n, m = len(A[0]) - 1, len(PT[0]) - 1
    assert PT[0][0] == 0 and PT[0][m] == n and (np.diff(PT[0]) >= 0).all()
    assert sorted(PT[1].tolist()) == list(range(n))


@pytest.mark.parametrize("name", sorted(_small))
def test_ptap_case_is_wellformed_and_restated(oracle, name):
    """Every small case is a valid (A, P_T), and the Python restatement of the pinned
    order gives orc_ptap's bits on it (so the restated wrong orders differ from the
    oracle by their order alone)."""
    A, PT = _small[name]
    _check_pt(A, PT)
    if len(A[0]) - 1 <= 128:
        assert _same(S.ptap_in_order(A, PT, "oracle"), oracle.ptap(A, PT))


@pytest.mark.parametrize("weights", sorted(S.WEIGHTS))
def test_ptap_wrong_orders_cannot_pass(oracle, weights):
    A, PT = S.graph96(weights)
    want = oracle.ptap(A, PT)
    for order in S.ORDERS[1:]:
        got = S.ptap_in_order(A, PT, order)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (got[2] != want[2]).sum() >= 1, order


def test_ptap_empty_aggregates():
    sizes = np.diff(S.graph96("mixed")[1][0])
    assert tuple(sizes) == S.SIZES96 == (1, 0, 17, 0, 0, 33, 2, 43, 0)
    # (the last aggregate is empty: a head at position n)
    assert (sizes == 0).sum() == 4 and sizes[0] == 1 and sizes[-1] == 0
    assert tuple(np.diff(_small["first_aggregates_empty"][1][0])[:3]) == (0, 0, 5)
    assert tuple(np.diff(_small["only_aggregate0"][1][0])) == (96, 0, 0, 0)
    assert (0, 0) == tuple(np.diff(S.hub_graph("first")[1][0])[9:11])
    # the ranges whose first or last rows (at least once both) are empty aggregates
    for key, sz in (("graph96", sizes), ("hub", np.diff(S.hub_graph("first")[1][0]))):
        ends = [(sz[a0] == 0, sz[a1 - 1] == 0) for a0, a1 in S.RANGES_IN_EMPTY[key]]
        assert all(a or b for a, b in ends) and any(a and b for a, b in ends)


def test_ptap_empty_rows():
    A, PT, empty, (a0, a1) = S.empty_rows_graph()
    length = np.diff(A[0])
    pos_len = length[PT[1]]  # row length by P_T position
    assert (length == 0).sum() == len(empty) == 7
    assert pos_len[0] == 0 and pos_len[-1] == 0 and (pos_len[20:23] == 0).all()
    assert pos_len[PT[0][a0]] == 0 and pos_len[PT[0][a1] - 1] == 0
    assert np.isin(A[1], list(empty)).any()  # columns still reach the empty rows


@pytest.mark.parametrize("where", ["first", "last"])
def test_ptap_hub(where):
    A, PT, hub = S.hub_graph(where)
    assert np.diff(A[0])[hub] == S.HUB_DEG > 2 * 256
    a = int(np.searchsorted(PT[0], np.flatnonzero(PT[1] == hub)[0], side="right")) - 1
    seg = PT[1][PT[0][a]:PT[0][a + 1]]
    assert len(seg) == 50 and (seg[0] if where == "first" else seg[-1]) == hub


def test_ptap_shapes_and_key_widths():
    assert [S.bits_below(x) for x in (0, 1, 2, 3, 64, 65, 1 << 21, (1 << 21) + 1, 1 << 22,
                                      (1 << 22) + 2)] == [0, 0, 1, 2, 6, 7, 21, 22, 22, 23]
    shapes = {k: (len(A[0]) - 1, len(PT[0]) - 1) for k, (A, PT) in _small.items()}
    assert shapes["one_aggregate"] == (50, 1) and shapes["identity"] == (40, 40)
    assert shapes["single_vertex"] == (1, 1) and _small["single_vertex"][0][1][0] == 0
    for n in (64, 65):
        for m in (64, 65):
            assert shapes[f"pow2_n{n}_m{m}"] == (n, m)
    # the two key-width shapes: 64 bits exactly, and more
    (n0, w0), (n1, w1) = S.KEY_WIDTH
    assert S.bits_below(n0) + 2 * S.bits_below(n0 // 2) == 64 and not w0
    assert S.bits_below(n1) + 2 * S.bits_below(n1 // 2) == 67 and w1
    assert n1 == n0 + 2  # the next even ring


def test_ptap_ring_builder(oracle):
    """ring_pairs at a small size (the builder the key-width cases use at 2^22)."""
    A, PT = S.ring_pairs(64)
    _check_pt(A, PT)
    assert (np.diff(A[0]) == 2).all() and (np.diff(PT[0]) == 2).all()
    C = oracle.ptap(A, PT)
    assert (np.diff(C[0]) == 3).all()  # itself and both neighbouring pairs
    assert _same(S.ptap_in_order(A, PT, "oracle"), C)


def test_ptap_unsorted_dups_and_zeros(oracle):
    A, PT = _small["unsorted_dups"]
    unsorted = dups = 0
    for i in range(len(A[0]) - 1):
        cols = A[1][A[0][i]:A[0][i + 1]]
        w = A[2][A[0][i]:A[0][i + 1]]
        unsorted += bool((np.diff(cols) < 0).any())
        for c in set(cols.tolist()):
            if (cols == c).sum() > 1:
                dups += 1
                assert len(set(w[cols == c].tolist())) == (cols == c).sum()  # different weights
    assert unsorted == 60 and dups >= 60
    A, PT = _small["zeros"]
    C = oracle.ptap(A, PT)
    dense = {(a, int(C[1][e])): C[2][e] for a in range(3) for e in range(C[0][a], C[0][a + 1])}
    assert dense[(0, 1)] == 0.0 and dense[(0, 0)] == 0.0  # cancelling run keeps its entry
    assert dense[(1, 2)] == 0.0 and not np.signbit(dense[(1, 2)])
    assert dense[(2, 0)] == 1.5 and dense[(2, 2)] == 3.0
    assert len(C[1]) == 5


# ---------------------------------------------------------------------------
# graph set-up

def test_rmat_all_invalid_seed_and_empty():
    s, d = G.rmat_edges(S.ALL_INVALID["n"], S.ALL_INVALID["draws"], S.ALL_INVALID["seed"])
    assert len(s) == 0
    assert _same(ge.rmat_csr(**S.ALL_INVALID), (np.zeros(3, np.int32), [], []))
    for n in (2, 37):
        assert _same(ge.rmat_csr(n, 0, seed=1), (np.zeros(n + 1, np.int32), [], []))


def test_rmat_chunks_reach_their_paths():
    rc = S.rmat_keys(**S.RMAT)
    valid, keys = int(rc.sum()), 2 * S.RMAT["draws"]
    ch = S.rmat_chunks()
    assert keys == 80000 and valid == 79754 and rc[0] == rc.max() == 2896
    assert len(S.sort_segments(rc, ch["twenty"])) == 21
    assert S.scan_calls(valid, ch["twenty"]) == 20 and S.scan_calls(4097, ch["twenty"]) == 2
    assert ch["all_keys"] == keys  # L <= chunk: the single call
    assert keys > ch["all_keys_minus_1"] >= valid and \
        S.sort_segments(rc, ch["all_keys_minus_1"]) == [0]
    assert valid % ch["valid_minus_1"] == 1 and S.scan_calls(valid, ch["valid_minus_1"]) == 2
    b = S.sort_segments(rc, ch["boundary_after_empty_row"])
    assert any(rc[r - 1] == 0 for r in b[1:]) and all(rc[r] > 0 for r in b[1:])
    assert S.sort_segments(rc, ch["below_row0"]) is None and ch["below_row0"] == rc[0] - 1
    assert _same(ge.rmat_csr(**S.RMAT), G.rmat(S.RMAT["n"], S.RMAT["draws"], S.RMAT["seed"]))


_lcc = S.lcc_cases()


@pytest.mark.parametrize("name", sorted(_lcc))
def test_lcc_host_matches_definition(name):
    A, chunk = _lcc[name]
    n = len(A[0]) - 1
    got = ge.largest_component(A)
    if n:
        assert _same(got, G.largest_component(A))
    else:
        assert _same(got, (np.zeros(1, np.int32), [], []))
    k = len(got[0]) - 1
    if n > 1:  # both scans (n and k + 1 items) run in chunks under the case's chunk
        assert S.scan_calls(n, chunk) > 1 and S.scan_calls(k + 1, chunk) > 1
    want_k = {"n0": 0, "n1": 1, "edgeless5": 1, "path_ascending": 4097, "path_permuted": 4097,
              "tie_vertex0_second": 3, "isolated_last": 3, "self_loops": 3, "weights": 4,
              "connected": 300}[name]
    assert k == want_k
    if name == "tie_vertex0_second":  # {0, 8, 9}, not {1, 2, 3}
        assert _same(got, S.sym_csr(3, [(0, 2), (1, 2)]))
    if name == "weights":
        assert len(set(got[2].tolist())) == len(got[2]) > 0
    if name == "self_loops":
        assert (got[1] == np.repeat(np.arange(k), np.diff(got[0]))).sum() == 1


# ---------------------------------------------------------------------------
# modularity

_mod = S.modularity_cases()


def _int_sums(A, vA, m):
    """d_in, d_out per aggregate and T with the reference's truncation, in Python ints."""
    din, dout, T = [0] * m, [0] * m, 0
    for i in range(len(A[0]) - 1):
        for e in range(A[0][i], A[0][i + 1]):
            w = int(A[2][e])  # toward zero, as the C conversion
            if vA[i] == vA[A[1][e]]:
                din[vA[i]] += w
            else:
                dout[vA[i]] += w
            T += w
    return din, dout, T


@pytest.mark.parametrize("name", sorted(_mod))
def test_modularity_case(oracle, name):
    A, vA, m = _mod[name]
    din, dout, T = _int_sums(A, vA, m)
    assert T != 0 and np.abs(A[2]).max() < 2.0 ** 31
    if name == "negative_fractional":
        assert din == [-2, 14] and dout == [0, -3] and T == 9
    elif name == "large_sums":
        assert 2 ** 32 < din[0] < 2 ** 53 and din[0] == 4350 * 2 ** 30 and dout == [3, 3]
    elif name == "int_limit":
        assert din[0] == 2 * (2 ** 31 - 1) and din[1] == 2 ** 31 - 1 + 2 ** 31 - 2
    elif name == "unused_aggregates":
        assert m == 9 and set(vA.tolist()) == {0, 2, 4, 6}
    else:
        assert m == 1 and dout == [0]
    q = ge.modularity(A, vA, m)
    assert q == oracle.modularity(A, vA, m) and np.isfinite(q)


# ---------------------------------------------------------------------------
# radius step

_ties = S.radius_tie_cases()
EQUAL_PAIRS = {  # (pairs of events with equal start times, events)
    "lattice_d1": (2024, 276), "lattice_d2": (4242, 300), "lattice_d3": (8953, 351),
    "lattice_d5": (31880, 496), "grid_one_group": (23653, 218),
    "grid_one_group_permuted": (23653, 218), "grid_bands": (14365, 170),
    "grid_bands_permuted": (14365, 170), "star_equal_spokes": (524, 40),
    "duplicate_entries": (1653, 58)}


def _host_equals_oracle(oracle, case):
    cA, dim, base, PTc, cAc, rAc, Ac = case
    r1, c1 = ge.radius_step(cA, dim, base, PTc=PTc, coords_Ac=cAc, r_Ac=rAc, Ac=Ac)
    r2, c2 = oracle_radius(oracle, cA, dim, base, PTc, cAc, rAc, Ac)
    assert np.array_equal(r1, r2) and np.array_equal(c1, c2)
    return r2, c2


@pytest.mark.parametrize("name", sorted(_ties))
def test_radius_tie_case(oracle, name):
    """The lattice inputs start with hundreds of equal event times; the host loop gives the
    oracle's bits on them."""
    case = _ties[name]
    assert S.equal_time_pairs(case) == EQUAL_PAIRS[name]
    assert EQUAL_PAIRS[name][0] >= 500
    _host_equals_oracle(oracle, case)


def test_radius_clamp_case(oracle):
    case = S.radius_clamp_case()
    cA, dim, _, PTc, cAc, rAc, _ = case
    assert (cA[:4] == cAc[:4]).all() and (np.diff(PTc[0])[:4] == 1).all()
    assert rAc[0] == 0.0 and rAc[1] < S.CLAMP == rAc[2] < rAc[3]
    r, c = _host_equals_oracle(oracle, case)
    # alpha = r_Ac for these singletons: clamped below 1e-6, r_Ac / r_Ac = 1 from it on
    assert r[0] == 0.0 and r[1] == (rAc[1] / S.CLAMP) * rAc[1] < rAc[1]
    assert r[2] == rAc[2] and r[3] == rAc[3] and (c[:4] == cAc[:4]).all()


@pytest.mark.parametrize("dim", [1, 16])
def test_radius_underflow_case(oracle, dim):
    case = S.radius_underflow_case(dim)
    cA = case[0]
    diff = cA[3] - cA[7]
    assert (diff[:-1] == 0).all() and diff[-1] == 1e-170 and diff[-1] * diff[-1] == 0.0
    grp0 = case[3][1][:case[3][0][1]]
    assert 3 in grp0 and 7 in grp0 and 7 in case[6][1][case[6][0][3]:case[6][0][4]]
    _host_equals_oracle(oracle, case)


@pytest.mark.parametrize("dim", [1, 3, 16])
@pytest.mark.parametrize("extra", [False, True])
def test_radius_group_sizes_case(oracle, dim, extra):
    case, groups = S.radius_group_sizes_case(dim, extra)
    cA, _, _, PTc, cAc, rAc, Ac = case
    assert tuple(len(g) for g in groups[:7]) == S.GROUP_SIZES == (1, 2, 63, 64, 65, 128, 129)
    assert len(groups) == (8 if extra else 7) and (len(groups) % 4 == 0) == extra
    r, c = _host_equals_oracle(oracle, case)
    # after the rescale every member's reach dist(c_b, x_a) + r_a is s times the one
    # before it, so the member that set alpha is the one whose reach is r_Ac now
    def reach(b):
        g = groups[b]
        d = np.sqrt(((c[g] - cAc[b]) ** 2).sum(axis=1))
        return d, d + r[g]
    d, full = reach(S.LAST_SETS_ALPHA)
    assert np.argmax(full) == len(full) - 1 == 64 and full[-1] > 1.5 * np.sort(full)[-2]
    assert abs(full[-1] / rAc[S.LAST_SETS_ALPHA] - 1) < 1e-12
    d, full = reach(S.R_DECIDES)
    assert np.argmax(full) == 10 and np.argmax(d) != 10 and full[10] > 1.5 * np.sort(full)[-2]
    assert d[10] < d.max()
