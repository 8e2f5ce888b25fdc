"""The steps between levels on the device -- P^T A P (csrc/ge_ptap.hip), graph set-up
(ge_graph.hip), modularity (ge_quality.hip) and the radius step (ge_radius.hip) -- on the
inputs of tests/setup_cases.py (proved on the CPU by tests/test_setup_cases.py), against
the oracle (orc_ptap, orc_radius_step) and the host library (ge.rmat_csr,
ge.largest_component, ge.modularity).  Every comparison is np.array_equal on every
returned array, or == on the double; the info queries say which path ran.
"""
import numpy as np
import pytest

import ge_amd as ge
import setup_cases as S
from setup_cases import oracle_radius

pytestmark = pytest.mark.gpu

_small = S.ptap_small_cases()
_wants = {}


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _want(oracle, key, A, PT):
    """orc_ptap, computed once per case and never modified."""
    if key not in _wants:
        C = oracle.ptap(A, PT)
        for a in C:
            a.setflags(write=False)
        _wants[key] = C
    return _wants[key]


# ---------------------------------------------------------------------------
# P^T A P

def _check_info(info, n, m, R, split, entries, runs):
    """ge_ptap_info of a call that sorted: the widths, the path and the counts."""
    assert (info["bn"], info["bb"], info["ba"]) == (S.bits_below(n), S.bits_below(m),
                                                    S.bits_below(R))
    wide = info["bn"] + info["bb"] + info["ba"] > 64
    assert info["sort"] == (ge.PTAP_SORT_SPLIT_WIDTH if wide else
                            ge.PTAP_SORT_SPLIT_OVERRIDE if split else ge.PTAP_SORT_SINGLE)
    assert (info["entries"], info["runs"]) == (entries, runs)


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("name", sorted(_small))
def test_ptap_case(ctx, oracle, monkeypatch, name, split):
    """Every structural case whole, on the single sort and under GE_PTAP_SPLIT_SORT."""
    A, PT = _small[name]
    if split:
        monkeypatch.setenv("GE_PTAP_SPLIT_SORT", "1")
    else:
        monkeypatch.delenv("GE_PTAP_SPLIT_SORT", raising=False)
    want = _want(oracle, name, A, PT)
    got = ctx.ptap(A, PT)
    assert _same(got, want)
    n, m = len(A[0]) - 1, len(PT[0]) - 1
    _check_info(ctx.ptap_info(), n, m, m, split, len(A[1]), len(want[1]))


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("name", ["graph96_mixed", "graph96_uniform", "hub_first", "hub_last",
                                  "empty_rows"])
def test_ptap_row_ranges(ctx, oracle, monkeypatch, name, split):
    """ge_ptap_rows: the whole, single rows, ranges that start or end in runs of empty
    aggregates (or on empty fine rows), an empty range, and every [a, a + 1) put together."""
    A, PT = _small[name]
    if split:
        monkeypatch.setenv("GE_PTAP_SPLIT_SORT", "1")
    else:
        monkeypatch.delenv("GE_PTAP_SPLIT_SORT", raising=False)
    want = _want(oracle, name, A, PT)
    n, m = len(A[0]) - 1, len(PT[0]) - 1
    inside = (S.RANGES_IN_EMPTY["graph96"] if name.startswith("graph96") else
              S.RANGES_IN_EMPTY["hub"] if name.startswith("hub") else
              (S.empty_rows_graph()[3],))
    length = np.diff(A[0])
    for a0, a1 in S.ptap_ranges(m, inside):
        got = ctx.ptap(A, PT, rows=(a0, a1))
        part = S.slice_rows(want, a0, a1)
        assert _same(got, part), (a0, a1)
        entries = int(length[PT[1][PT[0][a0]:PT[0][a1]]].sum())
        info = ctx.ptap_info()
        if entries:
            _check_info(info, n, m, a1 - a0, split, entries, len(part[1]))
        else:  # nothing to emit: the call returns before it sorts
            assert info["sort"] == ge.PTAP_SORT_NONE and info["entries"] == info["runs"] == 0
    parts = [ctx.ptap(A, PT, rows=(a, a + 1)) for a in range(m)]
    assert _same(S.concat_rows(parts), want)


def test_ptap_rows_rejects_bad_ranges(ctx):
    A, PT = _small["zeros"]
    for rows in ((-1, 2), (2, 1), (0, 4)):
        with pytest.raises(ge.GeError, match="row range"):
            ctx.ptap(A, PT, rows=rows)


@pytest.mark.parametrize("n,wide", S.KEY_WIDTH, ids=["64_bits", "67_bits"])
def test_ptap_key_width(ctx, oracle, monkeypatch, n, wide):
    """The composite key at 64 bits takes the single sort; above it the split sort is
    chosen by the width itself, with no override.  A ring of n vertices in n / 2 pairs:
    the smallest shapes that sit on either side of the threshold."""
    monkeypatch.delenv("GE_PTAP_SPLIT_SORT", raising=False)
    A, PT = S.ring_pairs(n)
    want = oracle.ptap(A, PT)
    got = ctx.ptap(A, PT)
    info = ctx.ptap_info()
    assert info["bn"] + info["bb"] + info["ba"] == (67 if wide else 64)
    assert info["sort"] == (ge.PTAP_SORT_SPLIT_WIDTH if wide else ge.PTAP_SORT_SINGLE)
    _check_info(info, n, n // 2, n // 2, False, 2 * n, 3 * (n // 2))
    assert _same(got, want)


# ---------------------------------------------------------------------------
# graph set-up

def _empty(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0)


@pytest.mark.parametrize("n", [2, 37])
@pytest.mark.parametrize("lcc", [False, True])
def test_rmat_no_draws(ctx, monkeypatch, n, lcc):
    """draws = 0 is the host's empty graph, not a launch with an empty grid; its largest
    component is vertex 0 alone."""
    monkeypatch.delenv("GE_GRAPH_CHUNK", raising=False)
    got = ctx.rmat_csr(n, 0, seed=1, lcc=lcc)
    assert _same(got, ge.largest_component(ge.rmat_csr(n, 0, seed=1)) if lcc
                 else ge.rmat_csr(n, 0, seed=1))
    assert _same(got, _empty(1 if lcc else n))


@pytest.mark.parametrize("chunk", [None, 5])
def test_rmat_every_draw_invalid(ctx, monkeypatch, chunk):
    """Twelve keys, none valid: an empty graph on the single sort, and on the segmented
    one, which drops them all before it sorts."""
    if chunk is None:
        monkeypatch.delenv("GE_GRAPH_CHUNK", raising=False)
    else:
        monkeypatch.setenv("GE_GRAPH_CHUNK", str(chunk))
    assert _same(ctx.rmat_csr(**S.ALL_INVALID), ge.rmat_csr(**S.ALL_INVALID))
    assert _same(ctx.rmat_csr(**S.ALL_INVALID), _empty(2))
    info = ctx.graph_info()
    assert info["sort_segments"] == (0 if chunk is None else 1)
    assert info["chunk"] == (1 << 28 if chunk is None else chunk)


_chunks = S.rmat_chunks()
_rmat = {}


def _rmat_want():
    if not _rmat:
        A = ge.rmat_csr(**S.RMAT)
        _rmat["A"], _rmat["lcc"] = A, ge.largest_component(A)
        _rmat["rc"] = S.rmat_keys(**S.RMAT)
    return _rmat


@pytest.mark.parametrize("name", [k for k in sorted(_chunks) if k != "below_row0"])
def test_rmat_chunked(ctx, monkeypatch, name):
    """The segmented sort and the chunked scan with its carry chain, on 80 000 keys: the
    host's CSR and its LCC, and the segment and chunk counts the chunk must give."""
    chunk = _chunks[name]
    monkeypatch.setenv("GE_GRAPH_CHUNK", str(chunk))
    w = _rmat_want()
    n, keys, valid = S.RMAT["n"], 2 * S.RMAT["draws"], int(w["rc"].sum())
    assert _same(ctx.rmat_csr(**S.RMAT), w["A"])
    info = ctx.graph_info()
    single = keys <= chunk
    assert info["chunk"] == chunk
    assert info["sort_segments"] == (0 if single else len(S.sort_segments(w["rc"], chunk)))
    scanned = [keys if single else valid, n + 1]
    assert info["scans"] == 2
    assert info["scan_calls"] == sum(S.scan_calls(c, chunk) for c in scanned)
    assert _same(ctx.rmat_csr(lcc=True, **S.RMAT), w["lcc"])
    info = ctx.graph_info()
    k = len(w["lcc"][0]) - 1
    assert info["scans"] == 4
    assert info["scan_calls"] == sum(S.scan_calls(c, chunk) for c in scanned + [n, k + 1])


def test_rmat_row_exceeds_chunk(ctx, monkeypatch):
    """A chunk smaller than row 0's key count is refused with a status (a host-side
    check before the keys are scattered), and so is a chunk that is no item count."""
    monkeypatch.setenv("GE_GRAPH_CHUNK", str(_chunks["below_row0"]))
    with pytest.raises(ge.GeError, match="one row exceeds a sort chunk"):
        ctx.rmat_csr(**S.RMAT)
    for bad in ("0", "-4", "12x", str((1 << 28) + 1)):
        monkeypatch.setenv("GE_GRAPH_CHUNK", bad)
        with pytest.raises(ge.GeError, match="GE_GRAPH_CHUNK"):
            ctx.rmat_csr(2, 1, seed=1)


_lcc = S.lcc_cases()


@pytest.mark.parametrize("chunked", [False, True], ids=["one_call", "chunked"])
@pytest.mark.parametrize("name", sorted(_lcc))
def test_lcc_case(ctx, monkeypatch, name, chunked):
    A, chunk = _lcc[name]
    if chunked:
        monkeypatch.setenv("GE_GRAPH_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("GE_GRAPH_CHUNK", raising=False)
        chunk = 1 << 28
    want = ge.largest_component(A)
    assert _same(ctx.largest_component(A), want)
    n, k = len(A[0]) - 1, len(want[0]) - 1
    info = ctx.graph_info()
    assert info["chunk"] == chunk and info["sort_segments"] == 0
    if n == 0:
        assert info["scans"] == info["scan_calls"] == 0
    else:
        assert info["scans"] == 2
        assert info["scan_calls"] == S.scan_calls(n, chunk) + S.scan_calls(k + 1, chunk)
        if chunked and n > 1:
            assert info["scan_calls"] >= 4  # both scans ran in chunks


# ---------------------------------------------------------------------------
# modularity

_mod = S.modularity_cases()


@pytest.mark.parametrize("name", sorted(_mod))
def test_modularity_case(ctx, name):
    """Weights truncated to int and summed in 64-bit atomics: negative sums, a sum past
    2^32, weights next to the int limit, unused aggregates, one aggregate.  Weights of
    2^31 and above are not tested: the reference's own conversion is undefined there."""
    A, vA, m = _mod[name]
    assert ctx.modularity(A, vA, m) == ge.modularity(A, vA, m)


# ---------------------------------------------------------------------------
# radius step

def _radius(ctx, oracle, case, device=True, repeats=2):
    cA, dim, base, PTc, cAc, rAc, Ac = case
    r2, c2 = oracle_radius(oracle, cA, dim, base, PTc, cAc, rAc, Ac)
    rounds = None
    for rep in range(repeats):
        r1, c1, dev = ctx.radius_step(cA, dim, base, PTc=PTc, coords_Ac=cAc, r_Ac=rAc, Ac=Ac)
        assert dev == device
        assert np.array_equal(r1, r2) and np.array_equal(c1, c2), rep
        rounds = ctx.radius_info()
    return rounds


_ties = S.radius_tie_cases()


@pytest.mark.parametrize("name", sorted(_ties))
def test_radius_ties(ctx, oracle, name):
    """Integer lattices: hundreds of events start at equal times, so best_pair_kernel's
    (t, i, j) tie-break and the asg_ij comparison decide which events pop.  These cases
    guard progress (the rounds end within the bound) and the handling of the tuples.  They
    do not guard the value against another tie-break: on these inputs the result does not
    depend on which of two tied events pops first (a restatement of the rounds with the
    tie-break changed gives the same bits).  Nor can any input reach shift_kernel's
    `si && sj` value: an event shifted from both ends in one round has both endpoints
    assigned in that round, so its time is never read again."""
    case = _ties[name]
    events = S.equal_time_pairs(case)[1]
    rounds, max_pops = _radius(ctx, oracle, case)
    assert 1 <= rounds <= events and 1 <= max_pops <= events


def test_radius_rescale_clamp(ctx, oracle):
    """alpha = 0, just below 1e-6 (both clamped), 1e-6 and just above."""
    rounds, max_pops = _radius(ctx, oracle, S.radius_clamp_case())
    assert (rounds, max_pops) == (1, 1)  # the pair group's one event


@pytest.mark.parametrize("dim", [1, 16])
def test_radius_underflow_uses_host(ctx, oracle, dim):
    """A difference of 1e-170 squares to 0, d == 0, and the host loop runs instead."""
    assert _radius(ctx, oracle, S.radius_underflow_case(dim), device=False) == (0, 0)


@pytest.mark.parametrize("dim", [1, 3, 16])
@pytest.mark.parametrize("extra", [False, True], ids=["mc7", "mc8"])
def test_radius_group_sizes(ctx, oracle, dim, extra):
    """Groups of 1, 2, 63, 64, 65, 128 and 129 members on the rescale's 64-lane stride,
    mc on either side of a multiple of the four groups per block; the last member in P_T
    order sets one group's alpha, r rather than the distance another's."""
    case, groups = S.radius_group_sizes_case(dim, extra)
    events = S.equal_time_pairs(case)[1]
    rounds, max_pops = _radius(ctx, oracle, case)
    assert 1 <= rounds <= events and max_pops > 1
