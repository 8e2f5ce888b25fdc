"""Every kernel class and threshold of the device partition
(graph-embed_amd/csrc/ge_partition_dev.hip) on the directed inputs of
tests/partition_cases.py (checked on the CPU in tests/test_partition_cases.py).

Every case asserts that P_T equals oracle.partition on bits, that the final
quotient graph and alpha equal the library's host path on bits (pinned to the trace
in tests/test_partition_real_weights.py), and that the census
(GE_PARTITION_CENSUS=1, info["census"]) shows the path the case was built for:
exact counts where the construction fixes them (a one-round run through
partition_single(num_parts = n), also against the host path), at least one
elsewhere.  The scan and patch families run again with GE_PARTITION_NO_PATCH and
GE_PARTITION_FULL_SCANS: the same bits, no patch and no shortcut.

GE_PARTITION_CENSUS_LOG=<file> appends every census taken here to that file.
"""
import os

import pytest

import ge_amd as ge
import partition_cases as P
import partition_trace as T
import ref_cases as C
from test_gpu_partition_real_weights import same_result

pytestmark = pytest.mark.gpu

MODES = [None, "GE_PARTITION_NO_PATCH", "GE_PARTITION_FULL_SCANS"]
MODE_IDS = ["default", "no_patch", "full_scans"]
SCAN = [(label, L, tie, real) for real in (False, True) for label, L, tie in P.scan_cases(real)]
SCAN_IDS = [("real-" if real else "") + label for label, _, _, real in SCAN]
KEPT = ("kept_bound", "kept_runner_up", "kept_nonpositive")
PATCH = ("patched", "patch_short", "patch_size", "patch_fit")
_cache = {}


@pytest.fixture(autouse=True)
def device_required_with_census(monkeypatch):
    monkeypatch.setenv("GE_PARTITION_DEVICE_REQUIRE", "1")
    monkeypatch.setenv("GE_PARTITION_CENSUS", "1")


@pytest.fixture
def mode_env(monkeypatch):
    def set_mode(mode):
        if mode:
            monkeypatch.setenv(mode, "1")
    return set_mode


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def record(request, what, census):
    path = os.environ.get("GE_PARTITION_CENSUS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{request.node.name} {what}: " +
                    " ".join(f"{k}={v}" for k, v in census.items() if v) + "\n")


def whole_loop(request, ctx, oracle, key, A, stall, ordered=False):
    """The whole loop on the device against the oracle (P_T) and the host path
    (P_T, final graph, final alpha); returns the census."""
    want = cached(("oracle", key), lambda: oracle.partition(A, P.CF, stall=stall))
    host = cached(("host", key), lambda: ge.partition(A, P.CF, stall=stall, info=True))
    assert host[1]["path"] == ge.PATH_HOST and not any(host[1]["census"].values())
    dev = ctx.partition(A, P.CF, stall=stall, info=True)
    assert dev[1]["path"] == (ge.PATH_DEVICE_ORDERED if ordered else ge.PATH_DEVICE_EXACT)
    assert dev[1]["rounds"] == host[1]["rounds"]
    record(request, "loop", dev[1]["census"])
    assert C.same_hier(dev[0], want)
    same_result(dev, host)
    check_census(dev[1])
    return dev[1]["census"]


def one_round(request, ctx, key, A):
    """Round 1 alone on the device against the host path; returns the census."""
    n = len(A[0]) - 1
    host = cached(("host1", key), lambda: ge.partition_single(A, n, info=True))
    dev = ctx.partition_single(A, n, info=True)
    assert dev[1]["rounds"] == host[1]["rounds"] == 1
    record(request, "round 1", dev[1]["census"])
    same_result(([dev[0]], dev[1]), ([host[0]], host[1]))
    check_census(dev[1])
    return dev[1]["census"]


def check_census(info):
    """What holds for every census."""
    c = info["census"]
    assert list(c) == list(ge.CENSUS_FIELDS) and all(v >= 0 for v in c.values())
    assert [c["rebuilt_wave"], c["rebuilt_block"], c["rebuilt_global"]] == info["rebuilt"]
    assert c["rebuilt_in_place"] + c["rebuilt_moved"] == sum(info["rebuilt"])
    assert (c["match_global_rounds"] > 0) == (c["match_max_candidates"] > P.LOCAL_CAND)
    if os.environ.get("GE_PARTITION_NO_PATCH"):
        assert not any(c[k] for k in PATCH)
    if os.environ.get("GE_PARTITION_FULL_SCANS"):
        assert not any(c[k] for k in KEPT) and c["rescan_bound"] == 0


def test_census_is_off_by_default(ctx, monkeypatch):
    monkeypatch.delenv("GE_PARTITION_CENSUS")
    A = P.path_case(1025)
    got, info = ctx.partition(A, P.CF, info=True)
    assert info["path"] == ge.PATH_DEVICE_EXACT and sum(info["rebuilt"]) > 0
    assert list(info["census"]) == list(ge.CENSUS_FIELDS) and not any(info["census"].values())


# ---- scans ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("label,L,tie,real", SCAN, ids=SCAN_IDS)
def test_scan_classes_and_ties(request, ctx, oracle, mode_env, label, L, tie, real, mode):
    """The hub's list in each scan class and on each side of its threshold, the two
    maximal entries across lanes, waves, strides and chunks, or the single maximum
    last: the hub's merge shows the argmax in P_T."""
    key = ("scan", L, tie, real)
    A = cached(key, lambda: P.scan_case(L, tie, real))
    n = len(A[0]) - 1
    mode_env(mode)
    whole_loop(request, ctx, oracle, key, A, P.STALL, ordered=real)
    c = one_round(request, ctx, key, A)
    # pass 0 scans every list; in pass 1 only the second maximal leaf is untouched:
    # its argmax, the hub, is touched and its recorded bound is -inf, so it keeps
    # its result (the last-pass shortcut) unless every scan is forced
    left = 1 if tie is not None else 0
    forced = mode == "GE_PARTITION_FULL_SCANS"
    want = {"scan_small": n - 1 + (left if forced else 0), "scan_mid": 0, "scan_big": 0,
            "scan_huge": 0}
    want[P.scan_class(L)] += 1
    assert {k: c[k] for k in want} == want
    assert [c[k] for k in KEPT] == [0, 0, 0 if forced else left]
    assert c["rescan_changed"] == (1 if L > P.SMALL_LEN else 0)
    assert c["rescan_bound"] == c["rescan_touched"] == 0
    # the hub keeps its merge: its rebuild needs L + 1 slots
    assert c[P.rebuild_class(L + 1, real)] >= 1
    if L + 1 > (P.BLOCK_NEED_ORD if real else P.BLOCK_NEED):
        # a hub, but with L / 2 - 1 absorbed neighbours: too many for the patch's sets
        tried = int(not real and mode != "GE_PARTITION_NO_PATCH")
        assert [c[k] for k in PATCH] == [0, 0, tried, 0] and c["rebuilt_global"] == 1


# ---- rebuilds -------------------------------------------------------------------------------

@pytest.mark.parametrize("real", [False, True], ids=["integer", "real"])
def test_rebuild_classes(request, ctx, oracle, real):
    """Pairs whose tables need exactly 64, 65, 2 048 and 2 049 slots (1 024 and
    1 025 with real weights): the lists per class are those the trace's merges give."""
    needs = P.REBUILD_NEEDS_REAL if real else P.REBUILD_NEEDS
    A, pairs = P.rebuild_case(needs, real)
    key = ("rebuild", real)
    whole_loop(request, ctx, oracle, key, A, P.STALL, ordered=real)
    c = one_round(request, ctx, key, A)
    log = []
    T.trace(A, num_parts=len(A[0]) - 1, log=log)
    want = P.rebuild_classes(A, log[0], real)
    assert {k: c[k] for k in want} == want
    # a keeper's merged list outgrows its row; the renamed leaves stay in place
    assert c["rebuilt_moved"] == len(pairs)
    assert c["patched"] == 0 and c["patch_size"] == c["patch_fit"] == 0
    assert c["patch_short"] == (0 if real else want["rebuilt_global"])


# ---- hub patches ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("label", list(P.PATCH_ROUND1))
def test_patch_thresholds(request, ctx, oracle, mode_env, label, mode):
    """Absorbed neighbours, the partner's list and the hub's own list on either side
    of the patch's limits: patched, or rebuilt for the reason the case was built for."""
    kw, want = P.PATCH_ROUND1[label]
    key = ("patch", label)
    A = cached(key, lambda: P.patch_case(**kw)[0])
    mode_env(mode)
    whole_loop(request, ctx, oracle, key, A, P.STALL)
    c = one_round(request, ctx, key, A)
    if mode == "GE_PARTITION_NO_PATCH":
        want = {}
    assert {k: c[k] for k in PATCH} == {k: want.get(k, 0) for k in PATCH}
    # the hub is the only list of the global class, unless its table fits a block
    in_block = kw["Lh"] + kw.get("glen", 0) <= P.BLOCK_NEED
    assert c["rebuilt_global"] == (0 if in_block else 1 - c["patched"])
    # scans of more than 512 entries: the hub in pass 0, and again in pass 1 when it
    # did not merge (its argmax did); a partner with a long list
    glen = kw.get("glen", 0)
    assert c["scan_big"] == 1 + (0 if glen else 1) + (1 if glen > P.MID_LEN else 0)
    assert c["scan_huge"] == 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_patch_grows_past_the_old_end(request, ctx, oracle, mode_env, mode):
    """Round 1: the hub's new keys outnumber its deletions and its capacity is still
    the row length, so the list is rebuilt into fresh space with slack; round 2: it
    is patched past its old end."""
    A = cached("grow", lambda: P.patch_case(**P.PATCH_GROW)[0])
    mode_env(mode)
    c = whole_loop(request, ctx, oracle, "grow", A, P.STALL)
    on = mode != "GE_PARTITION_NO_PATCH"
    assert [c[k] for k in PATCH] == ([1, 0, 0, 1] if on else [0, 0, 0, 0])
    assert c["rebuilt_global"] == (1 if on else 2) and c["rebuilt_moved"] >= 1


# ---- matching ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", P.MATCH_PATHS)
def test_matching_on_paths(request, ctx, oracle, n):
    """The greedy matching of a chain, on global memory while more than 1 024
    candidates live and in LDS below."""
    A = P.path_case(n)
    c = whole_loop(request, ctx, oracle, ("path", n), A, 1.0)
    handed = P.handed_to_resolve(A)
    assert c["match_max_candidates"] == handed
    assert (c["match_global_rounds"] > 0) == (handed > P.LOCAL_CAND)
    assert c["match_lds_rounds"] > 0
    if handed > P.LOCAL_CAND:  # the smallest live rank is taken each round, not many more
        assert c["match_global_rounds"] >= (handed - P.LOCAL_CAND) // 2


def test_matching_crowded_hubs(request, ctx, oracle):
    """1 500 candidates point at each of four hubs: the first locally-dominant round
    takes one per hub and kills the rest.  No census field counts the hub minima
    that resolve_min_kernel takes in its LDS table or past it, so that path rests on
    the agreement of the bits alone; the census only shows that nothing was left
    for the single-block matching."""
    A = P.crowd_case()
    c = whole_loop(request, ctx, oracle, "crowd", A, P.STALL)
    assert c["match_max_candidates"] == 0 and c["match_global_rounds"] == 0
    assert c["scan_big"] == 4 and c["rebuilt_block"] == 4


# ---- bookkeeping and shortcuts ------------------------------------------------------------------

@pytest.mark.parametrize("mode", [None, "GE_PARTITION_FULL_SCANS"], ids=["default", "full_scans"])
def test_pool_and_alive_list_compaction(request, ctx, oracle, mode_env, mode):
    """A sparse random graph run to the end: more merges in round 1 than the
    speculative record copy holds, the alive list compacted, the list pool
    compacted, and every scan shortcut taken."""
    A = cached("pool", P.pool_case)
    mode_env(mode)
    c = whole_loop(request, ctx, oracle, "pool", A, 1.0)
    assert c["record_refetches"] >= 1
    assert c["alive_compactions"] >= 1
    assert c["pool_compactions"] >= 1
    if mode is None:
        assert all(c[k] >= 1 for k in KEPT), c


@pytest.mark.parametrize("mode", [None, "GE_PARTITION_FULL_SCANS"], ids=["default", "full_scans"])
def test_runner_up_shortcut_on_an_equal_bound(request, ctx, oracle, mode_env, mode):
    """eta of the recorded runner-up equals the recorded bound of the remaining
    entries, one of which has a smaller id: the comparison must be strict
    (partition_cases.equal_bound_case)."""
    A = P.equal_bound_case()
    mode_env(mode)
    c = whole_loop(request, ctx, oracle, "equal_bound", A, 1.0)
    if mode is None:
        assert c["kept_bound"] >= 1 and c["kept_runner_up"] >= 1
