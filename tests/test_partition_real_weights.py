"""partition::partition on real-weighted graphs and its one-level overloads: the
library's host path (no device) against

  * tests/partition_trace.py, a Python restatement of the reference round loop
    that also returns the quotient graph and alpha the loop ends with.  P_T cannot
    show a wrong summation order (the restatement with its contraction's merges
    reversed gives the same P_T and other final weights), so the final graph's
    weight bits are the test; each case first asserts that it can see the order.
  * tests/golden/ref_partition_one_level.npz, recorded from the reference binary
    by tests/golden/make_ref_partition_one_level.py, for partition(A, numParts,
    ...) and partition(A, printing, ...); live against the binary where it exists.

The device paths are in tests/test_gpu_partition_real_weights.py.
"""
import os
import subprocess

import numpy as np
import pytest

import ge_amd as ge
import partition_trace as T
import ref_cases as C
import ref_lib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "graph-embed_amd")

CASES = [(g, w, s) for g in ("er600", "rmat1500") for w in (T.W3, T.W5) for s in (1.0, 0.9)]
ONE_LEVEL_KW = dict(positive_merging=False, matching_iterations=1, stall=0.9)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_against_trace(got, info, want):
    levels, fg, fa = want
    assert C.same_hier(got, levels)
    assert np.array_equal(info["final_graph"][0], fg[0])
    assert np.array_equal(info["final_graph"][1], fg[1])
    assert same_bits(info["final_graph"][2], fg[2])
    assert same_bits(info["final_alpha"], fa)


def assert_order_sensitive(name, values, **kw):
    """The restatement with its contraction reversed: same P_T, other final weights."""
    right, wrong = T.traced(name, values, **kw), T.traced(name, values, reverse=True, **kw)
    assert C.same_hier(right[0], wrong[0])
    assert np.array_equal(right[1][1], wrong[1][1])
    differing = int((right[1][2].view(np.uint64) != wrong[1][2].view(np.uint64)).sum())
    assert differing > 0, "this case cannot see the summation order"


@pytest.mark.parametrize("name,values,stall", CASES)
def test_trace_matches_oracle(oracle, name, values, stall):
    A = T.weights_from(T.graph(name), values)
    want = oracle.partition(A, T.CF, stall=stall)
    assert C.same_hier(T.traced(name, values, cf=T.CF, stall=stall)[0], want)


@pytest.mark.parametrize("name,values,stall", CASES)
def test_host_path_final_graph_bits(name, values, stall):
    assert_order_sensitive(name, values, cf=T.CF, stall=stall)
    A = T.weights_from(T.graph(name), values)
    got, info = ge.partition(A, T.CF, stall=stall, info=True)
    assert info["path"] == ge.PATH_HOST and info["rebuilt"] == [0, 0, 0]
    assert info["rounds"] > 1
    check_against_trace(got, info, T.traced(name, values, cf=T.CF, stall=stall))


def ineligible_inputs():
    """Inputs the device paths leave to the host: -0.0, NaN, infinite, asymmetric."""
    ip, ix, dx = T.weights_from(T.graph("rmat600"), T.W3)
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    e = int(np.flatnonzero(rows < ix)[5])
    m = int(np.flatnonzero((rows == ix[e]) & (ix == rows[e]))[0])
    out = {}
    for label, v in (("negative_zero", -0.0), ("nan", float("nan")), ("inf", float("inf"))):
        w = dx.copy()
        w[e] = w[m] = v
        out[label] = (ip, ix, w)
    w = dx.copy()
    w[e] = 0.25  # its mirror keeps the hashed weight
    out["asymmetric"] = (ip, ix, w)
    return out


@pytest.mark.parametrize("label", ["negative_zero", "nan", "inf", "asymmetric"])
def test_host_path_accepts_ineligible_inputs(oracle, label):
    A = ineligible_inputs()[label]
    got, info = ge.partition(A, T.CF, info=True)
    assert info["path"] == ge.PATH_HOST
    assert C.same_hier(got, oracle.partition(A, T.CF))


# -- the one-level overloads ----------------------------------------------------

def one_level_graphs():
    return {"rmat600": T.graph("rmat600"), "er600w": T.weights_from(T.graph("er600"), T.W3)}


def one_level_cases():
    out = []
    for name, n in (("rmat600", None), ("er600w", None)):
        for p in (1, 40, 200, "n", None):
            out.append((name, p))
    return out


def one_level_want(fix, name, A, p):
    for part, arr in zip(("ip", "ix", "dx"), A):
        assert np.array_equal(fix[f"{name}_A_{part}"], arr), "the fixture's input changed"
    key = f"{name}_single" if p is None else f"{name}_parts{p}"
    return fix[key + "_ip"], fix[key + "_ix"]


def resolve_parts(A, p):
    return len(A[0]) - 1 if p == "n" else p


@pytest.mark.parametrize("name,p", one_level_cases())
def test_partition_single_reproduces_reference_fixture(golden, name, p):
    A = one_level_graphs()[name]
    p = resolve_parts(A, p)
    want = one_level_want(golden("ref_partition_one_level"), name, A, p)
    got = ge.partition_single(A, p, **ONE_LEVEL_KW)
    assert got[2] == len(want[0]) - 1 and got[3] == len(A[0]) - 1
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name,p", one_level_cases())
def test_partition_single_live(name, p):
    if not ref_lib.available():
        pytest.skip("no reference binary")
    A = one_level_graphs()[name]
    p = resolve_parts(A, p)
    (want,) = ref_lib.partition(A, num_parts=p, positive_merging=False, matching=1, stall=0.9)
    assert C.same_hier([ge.partition_single(A, p, **ONE_LEVEL_KW)], [want])
    # and with the defaults of the signature
    (want,) = ref_lib.partition(A, num_parts=p)
    assert C.same_hier([ge.partition_single(A, p)], [want])


@pytest.mark.parametrize("name", ["rmat600", "er600w"])
def test_partition_single_is_the_last_level_without_snapshots(name):
    """coarseningFactor 0.0 never fires a snapshot: the hierarchy loop is then the
    one-level loop, and so are their final graphs."""
    A = one_level_graphs()[name]
    one, info1 = ge.partition_single(A, info=True)
    hier, info = ge.partition(A, 0.0, info=True)
    assert len(hier) == 1 and C.same_hier([one], hier)
    assert info1["rounds"] == info["rounds"]
    assert same_bits(info1["final_graph"][2], info["final_graph"][2])
    assert same_bits(info1["final_alpha"], info["final_alpha"])


@pytest.mark.parametrize("name,p", [("er600w", 40), ("er600w", None), ("rmat600", 200)])
def test_partition_single_against_trace(name, p):
    """The stop rule's final graph, not only its P_T."""
    A = one_level_graphs()[name]
    kw = dict(positive_merging=False, stall=0.9, matching=1)
    want = T.trace(A, num_parts=p, **kw)
    got, info = ge.partition_single(A, p, info=True, **ONE_LEVEL_KW)
    check_against_trace([got], info, want)


def test_partition_single_rejects_merge_leaves():
    with pytest.raises(ge.GeError):
        ge.partition_single(T.graph("rmat600"), merge_leaves=True)


def build_overload_driver(tmp_path):
    exe = str(tmp_path / "partition_overloads")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "partition_overloads.cpp"), f"-L{PKG}/lib",
                           "-lge", f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    return exe


def test_overload_driver_compiles(tmp_path):
    """The drop-in header's one-level overloads resolve as the reference's do (no
    argument / bools -> the single P_T, an int -> numParts) under -Wall -Werror;
    the driver runs in tests/test_gpu_partition_real_weights.py (the drop-in
    creates a device context)."""
    assert os.path.exists(build_overload_driver(tmp_path))
