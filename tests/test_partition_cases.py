"""tests/partition_cases.py on the CPU: every generator builds what it says, the
references agree on it (oracle, the library's host path, tests/partition_trace.py),
and every tie case can see the scan's index tie-break.  The device runs are in
tests/test_gpu_partition_paths.py.
"""
import numpy as np
import pytest

import ge_amd as ge
import partition_cases as P
import partition_trace as T
import ref_cases as C
from test_partition_real_weights import check_against_trace

SMALL = 20000  # vertices up to which the Python trace runs the whole loop

SCAN = [(label, L, tie, real) for real in (False, True) for label, L, tie in P.scan_cases(real)]
SCAN_IDS = [("real-" if real else "") + label for label, _, _, real in SCAN]
_cache = {}


def scan_graph(L, tie, real):
    key = ("scan", L, tie, real)
    if key not in _cache:
        _cache[key] = P.scan_case(L, tie, real)
    return _cache[key]


def one_round(A, **kw):
    n = len(A[0]) - 1
    return T.trace(A, num_parts=n, **kw)


# ---- structure ---------------------------------------------------------------------

@pytest.mark.parametrize("label,L,tie,real", SCAN, ids=SCAN_IDS)
def test_scan_case_structure(label, L, tie, real):
    A = scan_graph(L, tie, real)
    ln = P.lengths(A)
    cols, w = P.row(A, 0)
    assert ln[0] == L and np.array_equal(cols, np.arange(1, L + 1))  # position p: leaf p + 1
    special = P.scan_special(L, tie)
    if tie is not None:
        assert [s - 1 for s in special] == list(tie)
    for s in special:  # the hub is their only neighbour, with the same weight
        assert np.array_equal(P.row(A, s)[0], [0])
        assert P.row(A, s)[1].tobytes() == P.row(A, special[0])[1].tobytes()
    others = np.setdiff1d(np.arange(1, len(ln)), special)
    assert (ln[others[others <= L]] == 2).all() and (ln[others[others > L]] == 1).all()
    assert w.max() == w[special[0] - 1]
    integer = bool((A[2] == np.trunc(A[2])).all())
    assert integer != real


def test_scan_cases_cover_every_class_and_boundary():
    assert [P.scan_class(L) for L in P.SCAN_LENGTHS] == [
        "scan_small", "scan_mid", "scan_mid", "scan_big", "scan_big", "scan_huge", "scan_huge"]
    L = P.SCAN_LENGTHS[-1]
    # every thread of a chunk block (1 024 threads) enters the unrolled loop of scan_range
    assert L // P.HUGE_CHUNKS > 3 * 1024 + 1023 and (L - 1) // P.HUGE_CHUNKS == 4096
    for L in (16385, L):
        lo, hi = P.scan_ties(L)["chunks"]
        assert hi == lo + 1 and any(hi == L * k // 64 for k in range(1, 64))


def test_rebuild_case_structure():
    for real, needs in ((False, P.REBUILD_NEEDS), (True, P.REBUILD_NEEDS_REAL)):
        A, pairs = P.rebuild_case(needs, real)
        ln = P.lengths(A)
        assert [int(ln[u] + ln[g]) for u, g, _ in pairs] == list(needs)
        assert all(ln[u] > ln[g] for u, g, _ in pairs)
        assert bool((A[2] == np.trunc(A[2])).all()) != real
        assert len(ln) < 5000


@pytest.mark.parametrize("label", list(P.PATCH_ROUND1) + ["GROW"])
def test_patch_case_structure(label):
    kw = P.PATCH_GROW if label == "GROW" else P.PATCH_ROUND1[label][0]
    A, info = P.patch_case(**kw)
    ln = P.lengths(A)
    assert ln[0] == kw["Lh"] and np.array_equal(P.row(A, 0)[0], np.arange(1, kw["Lh"] + 1))
    if info["g"] is not None:
        assert ln[info["g"]] == kw["glen"] + kw.get("private", 0)
    assert len(info["absorbed"]) == kw["K"] + kw.get("front", 0) + kw.get("back", 0)
    # round 1 absorbs exactly these neighbours of the hub, and the hub merges with g only
    log = []
    one_round(A, log=log)
    gone = sorted(j for i, j in log[0] if 0 < j <= kw["Lh"] and i != 0)
    assert gone == info["absorbed"]
    assert [m for m in log[0] if 0 in m] == ([(0, info["g"])] if info["g"] is not None else [])
    if label == "holes":  # holes on both sides of the new end of the list
        end = kw["Lh"] - (kw["front"] + kw["back"])
        pos = np.array(info["absorbed"][-kw["back"]:]) - 1
        assert (pos >= end).all() and sum(a - 1 < end for a in info["absorbed"]) == 48


def test_patch_grow_case_rounds():
    """Round 1: three new keys against one deletion; round 2: the hub merges with
    g2 and takes its remaining private leaves."""
    A, info = P.patch_case(**P.PATCH_GROW)
    log = []
    T.trace(A, cf=P.CF, stall=P.STALL, log=log)
    assert len(log) == 2
    assert (0, info["g"]) in log[0] and (0, info["g2"]) in log[1]
    assert sum(1 for i, _ in log[0] if i == info["g2"]) == 1  # g2 absorbed one leaf of its own


def test_matching_case_structure():
    for n in P.MATCH_PATHS:
        A = P.path_case(n)
        assert len(A[0]) - 1 == n and len(A[1]) == 2 * (n - 1) and (A[2] == 1.0).all()
    got = {n: P.handed_to_resolve(P.path_case(n)) for n in P.MATCH_PATHS}
    assert got[1031] == P.LOCAL_CAND and got[1032] == P.LOCAL_CAND + 1
    assert got[1025] < P.LOCAL_CAND < got[2049] < got[5000]
    A = P.crowd_case()
    assert (np.sort(P.lengths(A))[-4:] > P.LOCAL_CAND).all()


def test_equal_bound_case_is_exact():
    A = P.equal_bound_case()
    total = float(A[2].sum())
    assert total == 4096.0 and (A[2] == np.trunc(A[2])).all()
    log = []
    T.trace(A, cf=P.CF, log=log)
    assert (3, 6) in log[0] and (0, 2) in log[1]  # k2 absorbs p; u merges with x, not k2
    # after round 1 k2's weighted degree is x's: eta(u, k2) == eta(u, x) exactly
    deg = np.add.reduceat(A[2], A[0][:-1])
    assert deg[3] + deg[6] == deg[2]


# ---- the references agree ------------------------------------------------------------

def agree(oracle, A, stall, whole):
    want = oracle.partition(A, P.CF, stall=stall)
    got, info = ge.partition(A, P.CF, stall=stall, info=True)
    assert info["path"] == ge.PATH_HOST
    assert C.same_hier(got, want)
    if whole:
        check_against_trace(got, info, T.trace(A, cf=P.CF, stall=stall))


@pytest.mark.parametrize("label,L,tie,real", SCAN, ids=SCAN_IDS)
def test_scan_case_references_agree(oracle, label, L, tie, real):
    agree(oracle, scan_graph(L, tie, real), P.STALL, L < SMALL)


@pytest.mark.parametrize("label", list(P.PATCH_ROUND1) + ["GROW"])
def test_patch_case_references_agree(oracle, label):
    kw = P.PATCH_GROW if label == "GROW" else P.PATCH_ROUND1[label][0]
    agree(oracle, P.patch_case(**kw)[0], P.STALL, True)


def test_other_case_references_agree(oracle):
    for real, needs in ((False, P.REBUILD_NEEDS), (True, P.REBUILD_NEEDS_REAL)):
        agree(oracle, P.rebuild_case(needs, real)[0], P.STALL, True)
    for n in P.MATCH_PATHS:
        agree(oracle, P.path_case(n), 1.0, True)
    agree(oracle, P.crowd_case(), P.STALL, True)
    agree(oracle, P.equal_bound_case(), 1.0, True)


def test_pool_case(oracle):
    """Seeded, symmetric, about 20 000 vertices of mean degree 8; its first round
    merges more pairs than the speculative record copy holds and shrinks the alive
    list past its compaction rule; the references agree on the whole loop."""
    A = P.pool_case()
    B = P.pool_case()
    assert all(np.array_equal(a, b) for a, b in zip(A, B))
    ip, ix, dx = A
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    assert n == 20000 and 7.5 < len(ix) / n < 8.0 and (dx == 1.0).all() and not (rows == ix).any()
    fwd = set(zip(rows.tolist(), ix.tolist()))
    assert all((c, r) in fwd for r, c in fwd)
    log = []
    want = T.trace(A, cf=P.CF, log=log)
    merges = len(log[0])
    assert merges > P.SPEC_MERGES
    left = n - merges
    assert n > left + left // 4 + 1024  # alist_len > M + M / 4 + 1024
    got, info = ge.partition(A, P.CF, info=True)
    assert C.same_hier(got, oracle.partition(A, P.CF))
    check_against_trace(got, info, want)


# ---- every tie case sees the tie-break --------------------------------------------------

@pytest.mark.parametrize("label,L,tie,real", [c for c in SCAN if c[2] is not None],
                         ids=[i for i, c in zip(SCAN_IDS, SCAN) if c[2] is not None])
def test_tie_cases_see_the_index_tie_break(oracle, label, L, tie, real):
    """The scan taking the last of the two maximal neighbours merges the hub with
    the other one: another P_T.  One round (num_parts = n), against the host path's
    one-level overload; on the small cases also the whole loop against the oracle."""
    A = scan_graph(L, tie, real)
    n = len(A[0]) - 1
    right = ge.partition_single(A, n)
    wrong = one_round(A, tie_last=True)[0]
    assert not C.same_hier(wrong, [right])
    if L < SMALL:
        assert C.same_hier(one_round(A)[0], [right])
        want = oracle.partition(A, P.CF, stall=P.STALL)
        assert not C.same_hier(T.trace(A, cf=P.CF, stall=P.STALL, tie_last=True)[0], want)


# ---- the rebuild classes of a round ---------------------------------------------------------

@pytest.mark.parametrize("real", [False, True])
def test_rebuild_classes_from_the_trace(real):
    needs = P.REBUILD_NEEDS_REAL if real else P.REBUILD_NEEDS
    A, pairs = P.rebuild_case(needs, real)
    log = []
    one_round(A, log=log)
    assert sorted(log[0]) == [(u, g) for u, g, _ in pairs]
    got = P.rebuild_classes(A, log[0], real)
    ln = P.lengths(A)
    want = {"rebuilt_wave": 0, "rebuilt_block": 0, "rebuilt_global": 0}
    for u, g, need in pairs:
        want[P.rebuild_class(need, real)] += 1
        want["rebuilt_wave"] += int(ln[g]) - 1  # g's leaves: one renamed entry each
    assert got == want
    block = P.BLOCK_NEED_ORD if real else P.BLOCK_NEED
    assert [P.rebuild_class(x, real) for x in (64, 65, block, block + 1)] == [
        "rebuilt_wave", "rebuilt_block", "rebuilt_block", "rebuilt_global"]
