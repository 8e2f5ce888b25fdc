"""The device partition on real-weighted graphs (the ordered contraction of
graph-embed_amd/csrc/ge_partition_dev.hip) and the one-level overloads on the
device.

Ground truth is tests/partition_trace.py (pinned to the oracle and shown to see
the summation order in tests/test_partition_real_weights.py) on the small graphs,
and the library's host path, pinned to the trace there, on the graph large enough
to reach every rebuild class.  Equality is on bits: P_T, the final quotient
graph's weights and the final alpha.
"""
import subprocess

import numpy as np
import pytest

import ge_amd as ge
import graphs as G
import partition_trace as T
import ref_cases as C
from test_partition_real_weights import (CASES, ONE_LEVEL_KW, build_overload_driver,
                                         check_against_trace, ineligible_inputs,
                                         one_level_cases, one_level_graphs, one_level_want,
                                         resolve_parts, same_bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def device_required(monkeypatch):
    """A device-path failure of any kind fails the test instead of falling back."""
    monkeypatch.setenv("GE_PARTITION_DEVICE_REQUIRE", "1")


def same_result(a, b):
    (ha, ia), (hb, ib) = a, b
    assert C.same_hier(ha, hb)
    for q in (0, 1):
        assert np.array_equal(ia["final_graph"][q], ib["final_graph"][q])
    assert same_bits(ia["final_graph"][2], ib["final_graph"][2])
    assert same_bits(ia["final_alpha"], ib["final_alpha"])


@pytest.mark.parametrize("name,values,stall", CASES)
def test_ordered_path_small_graphs(ctx, name, values, stall):
    A = T.weights_from(T.graph(name), values)
    got, info = ctx.partition(A, T.CF, stall=stall, info=True)
    assert info["path"] == ge.PATH_DEVICE_ORDERED
    assert sum(info["rebuilt"]) > 0
    check_against_trace(got, info, T.traced(name, values, cf=T.CF, stall=stall))


_big = {}


def big_graph():
    if "A" not in _big:
        _big["A"] = T.weights_from(G.largest_component(G.rmat(30000, 240000, seed=17)), T.W3)
    return _big["A"]


def big_device(ctx, stall):
    if ("dev", stall) not in _big:
        _big["dev", stall] = ctx.partition(big_graph(), 0.125, stall=stall, info=True)
    return _big["dev", stall]


@pytest.mark.parametrize("stall", [1.0, 0.9])
def test_ordered_path_every_rebuild_class(ctx, monkeypatch, stall):
    """Lists rebuilt by the wave, block and global-table kernels, against the host path."""
    got = big_device(ctx, stall)
    assert got[1]["path"] == ge.PATH_DEVICE_ORDERED
    assert all(r > 0 for r in got[1]["rebuilt"]), got[1]["rebuilt"]
    monkeypatch.setenv("GE_PARTITION_HOST", "1")
    host = ctx.partition(big_graph(), 0.125, stall=stall, info=True)
    assert host[1]["path"] == ge.PATH_HOST
    assert host[1]["rounds"] == got[1]["rounds"]
    same_result(got, host)


def test_ordered_path_incremental_scans(ctx, monkeypatch):
    """All-positive real weights keep the recorded-bound scan skips; every vertex
    rescanned in every pass gives the same bits."""
    want = big_device(ctx, 1.0)
    monkeypatch.setenv("GE_PARTITION_FULL_SCANS", "1")
    full = ctx.partition(big_graph(), 0.125, info=True)
    assert full[1]["path"] == ge.PATH_DEVICE_ORDERED
    same_result(full, want)


@pytest.mark.parametrize("stall", [1.0, 0.9])
def test_ordered_path_mixed_signs_and_self_loops(ctx, stall):
    """Weights of both signs (no incremental scans) and diagonal entries; stall 1.0
    merges this graph down to one vertex, 0.9 leaves a quotient graph to compare."""
    A = T.with_diagonal(T.weights_from(T.graph("rmat1500"), (-0.3, 0.1, 0.2, 0.7)), 7, 0.3)
    got, info = ctx.partition(A, T.CF, positive_merging=False, stall=stall, info=True)
    assert info["path"] == ge.PATH_DEVICE_ORDERED
    want = T.trace(A, cf=T.CF, positive_merging=False, stall=stall)
    assert stall == 1.0 or len(want[1][1]) > 0
    check_against_trace(got, info, want)


@pytest.mark.parametrize("matching", [1, 3])
def test_ordered_path_matching_iterations(ctx, matching):
    """Three passes: the merge order key covers (pass, `used` slot)."""
    A = T.weights_from(T.graph("rmat1500"), T.W3)
    got, info = ctx.partition(A, T.CF, matching_iterations=matching, info=True)
    assert info["path"] == ge.PATH_DEVICE_ORDERED
    check_against_trace(got, info, T.traced("rmat1500", T.W3, cf=T.CF, matching=matching))


def test_integer_weights_keep_the_exact_path(ctx, monkeypatch):
    A = G.largest_component(G.rmat(4096, 40000, seed=4096))
    dev = ctx.partition(A, 0.125, info=True)
    assert dev[1]["path"] == ge.PATH_DEVICE_EXACT
    assert sum(dev[1]["rebuilt"]) > 0
    monkeypatch.setenv("GE_PARTITION_HOST", "1")
    host = ctx.partition(A, 0.125, info=True)
    assert host[1]["path"] == ge.PATH_HOST
    same_result(dev, host)


@pytest.mark.parametrize("name,p", one_level_cases())
def test_partition_single_on_the_device(ctx, golden, name, p):
    A = one_level_graphs()[name]
    p = resolve_parts(A, p)
    want = one_level_want(golden("ref_partition_one_level"), name, A, p)
    got, info = ctx.partition_single(A, p, info=True, **ONE_LEVEL_KW)
    assert info["path"] == (ge.PATH_DEVICE_EXACT if name == "rmat600" else ge.PATH_DEVICE_ORDERED)
    assert got[2] == len(want[0]) - 1 and got[3] == len(A[0]) - 1
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    want_t = T.trace(A, num_parts=p, positive_merging=False, stall=0.9, matching=1)
    check_against_trace([got], info, want_t)


@pytest.mark.parametrize("label", ["negative_zero", "nan", "inf", "asymmetric"])
def test_ineligible_inputs_take_the_host_path(ctx, oracle, label):
    A = ineligible_inputs()[label]
    got, info = ctx.partition(A, T.CF, info=True)
    assert info["path"] == ge.PATH_HOST
    assert C.same_hier(got, oracle.partition(A, T.CF))


def test_dropin_one_level_overloads(tmp_path, golden):
    """partition::partition(A), (A, bools...) and (A, numParts, ...) through the
    drop-in header, against the reference's fixtures."""
    exe = build_overload_driver(tmp_path)
    fix = golden("ref_partition_one_level")
    name, A = "er600w", one_level_graphs()["er600w"]
    inp = str(tmp_path / "a.bin")
    with open(inp, "wb") as f:
        np.array([len(A[0]) - 1, len(A[1])], np.int32).tofile(f)
        np.asarray(A[0], np.int32).tofile(f)
        np.asarray(A[1], np.int32).tofile(f)
        np.asarray(A[2], np.float64).tofile(f)

    def run(*args):
        out = str(tmp_path / "p.bin")
        r = subprocess.run([exe, inp, out, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        buf = np.fromfile(out, dtype=np.int32)
        rows, cols = int(buf[0]), int(buf[1])
        return buf[2:3 + rows], buf[3 + rows:3 + rows + cols]

    for args, p in ((("bool", "0", "0.9", "1"), None), (("parts", "40", "0", "0.9", "1"), 40),
                    (("parts", "200", "0", "0.9", "1"), 200)):
        want = one_level_want(fix, name, A, p)
        got = run(*args)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # no argument: the defaults of the signature, as the library's own entry point
    got = run("single")
    want = ge.partition_single(A)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
