"""Dimensions above 4 through the C++ drop-in headers (graph-embed_amd/include):
partition::forceAtlas(A, 6) and partition::embed(As, Ps, 8) as a caller of the
reference writes them (tests/cpp/dims_driver.cpp), against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import dims_cases as D
import graphs as G
from test_dropin import PKG, REPO, HERE, write_csr

SEED = 77


def build_driver(tmp_path):
    exe = str(tmp_path / "dims_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "dims_driver.cpp"), f"-L{PKG}/lib", "-lge",
                           f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    return exe


def test_dims_driver_compiles(tmp_path):
    assert os.path.exists(build_driver(tmp_path))


@pytest.mark.gpu
def test_dropin_force_atlas_6_and_embed_8(tmp_path, oracle):
    exe = build_driver(tmp_path)
    A = G.erdos_renyi(40, 0.15, seed=40)  # the two-argument overload runs 100 000 iterations
    B = D.e_graph()
    paths = [str(tmp_path / f) for f in ("a.bin", "xa.bin", "b.bin", "xb.bin")]
    write_csr(paths[0], A)
    write_csr(paths[2], B)
    r = subprocess.run([exe] + paths + [str(SEED)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(paths[1], dtype=np.float64).reshape(-1, 6)
    assert np.array_equal(got, oracle.force_atlas(A, 6, iterations=100000, seed=SEED))
    hier = oracle.partition(B, 0.2)
    As = oracle.hierarchy_As(B, hier)
    got = np.fromfile(paths[3], dtype=np.float64).reshape(-1, 8)
    assert np.array_equal(got, oracle.embed(As, hier, 8, seed=SEED))
