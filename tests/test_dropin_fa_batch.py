"""forceAtlasToMultilevel and forceAtlasBatch of the drop-in headers
(graph-embed_amd/include/embed.hpp, forceatlas.hpp) through a C++ driver."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "graph-embed_amd")


def write_csr(path, A):
    ip, ix, dx = A
    with open(path, "wb") as f:
        np.array([len(ip) - 1, len(ix)], np.int32).tofile(f)
        np.asarray(ip, np.int32).tofile(f)
        np.asarray(ix, np.int32).tofile(f)
        np.asarray(dx, np.float64).tofile(f)


def build_driver(tmp_path):
    exe = str(tmp_path / "fa_batch_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror",
                           f"-I{PKG}/include", f"-I{PKG}/compat", f"-I{REPO}/include",
                           os.path.join(HERE, "cpp", "fa_batch_driver.cpp"), f"-L{PKG}/lib",
                           "-lge", f"-Wl,-rpath,{PKG}/lib", "-o", exe])
    return exe


def test_dropin_headers_compile(tmp_path):
    assert os.path.exists(build_driver(tmp_path))


@pytest.mark.gpu
def test_force_atlas_to_multilevel_equals_the_composition(tmp_path, golden):
    """embedVia(As, P_Ts, 2, forceAtlasToMultilevel(200)) against embedVia(As, P_Ts, 2,
    anyToMultilevel(<forceAtlas, 200 iterations>)) on config 1, bit for bit."""
    g = golden("embed_c1_er1000_d2")
    exe = build_driver(tmp_path)
    inp, batched, composed = (str(tmp_path / f) for f in ("a.bin", "b.bin", "c.bin"))
    write_csr(inp, (g["A_ip"], g["A_ix"], g["A_dx"]))
    r = subprocess.run([exe, inp, batched, composed, "2", str(int(g["seed"])), "0.1", "200"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    X = np.fromfile(batched, dtype=np.float64).reshape(-1, 2)
    Y = np.fromfile(composed, dtype=np.float64).reshape(-1, 2)
    assert X.shape == (len(g["A_ip"]) - 1, 2)
    assert np.isfinite(Y).all()
    assert np.array_equal(X, Y)
