"""Dimensions 5..16 on the CPU: the oracle reproduces, bit for bit, the fixtures
recorded from the reference binary (tests/golden/ref_dims_*.npz,
tests/golden/make_ref_dims.py), and so does the live binary where it exists.

These pin the yardstick of tests/test_gpu_dims.py, not the device code: the oracle
carries kMaxDim = 16 and the reference takes the dimension at run time.
"""
import numpy as np
import pytest

import dims_cases as D
import ref_cases as C
import ref_lib as R


@pytest.fixture(scope="module")
def man():
    return D.manifest()


@pytest.fixture(scope="module")
def ref():
    if not R.available():  # raises where the tree is present and the build fails
        pytest.skip("neither the reference tree nor a built oracle/_ref/ge_ref is here")
    return R


FA = [(d, name) for d in D.DIMS for name in D.fa_names()]
ML = [(d, name) for d in D.DIMS for name in D.ml_names(d)]


def test_manifest_has_the_fields_of_the_first_one(man):
    assert set(man) == set(C.manifest()) == {"build", "cases"}
    assert set(man["build"]) == set(C.manifest()["build"])
    assert "-ffp-contract=off" in man["build"]["flags"]


@pytest.mark.parametrize("d,name", FA)
def test_fixture_force_atlas(oracle, man, d, name):
    case = D.fa_case(name, d)
    assert C.input_hashes(case) == man["cases"][f"fa_d{d}"][name]["inputs"]  # generator drift
    want = D.load("fa", d)[name]
    assert want.shape == (D.FA_N, d) and np.isfinite(want).all()
    assert np.array_equal(C.run_fa(oracle.force_atlas, case), want)


@pytest.mark.parametrize("d,name", ML)
def test_fixture_force_atlas_ml(oracle, man, d, name):
    case = D.ml_case(name, d)
    assert C.input_hashes(case) == man["cases"][f"ml_d{d}"][name]["inputs"]
    assert np.array_equal(C.run_ml(oracle.force_atlas_ml, case), D.load("ml", d)[name])


@pytest.mark.parametrize("d", D.E_DIMS)
def test_fixture_embed(oracle, man, d):
    g = D.load_embed()
    hier = C.hier_from(g, "h")
    As = oracle.hierarchy_As(D.e_graph(), hier)
    entry = man["cases"]["embed"]
    assert C.input_hashes({"As": As}) == entry["inputs"]
    assert len(hier) >= 2
    assert np.array_equal(oracle.embed(As, hier, d, seed=entry["seed"]), g[f"x_d{d}"])


# --------------------------------------------------------------------------
# the live binary: every fixture again

@pytest.mark.parametrize("d,name", FA)
def test_live_force_atlas(ref, d, name):
    case = D.fa_case(name, d)
    assert np.array_equal(C.run_fa(ref.force_atlas, case), D.load("fa", d)[name])


@pytest.mark.parametrize("d,name", ML)
def test_live_force_atlas_ml(ref, d, name):
    case = D.ml_case(name, d)
    assert np.array_equal(C.run_ml(ref.force_atlas_ml, case), D.load("ml", d)[name])


def test_live_partition_of_the_embed_case(ref):
    g = D.load_embed()
    assert C.same_hier(ref.partition(D.e_graph(), cf=D.E_CF), C.hier_from(g, "h"))


@pytest.mark.parametrize("d", D.E_DIMS)
def test_live_embed(ref, oracle, man, d):
    g = D.load_embed()
    hier = C.hier_from(g, "h")
    As = oracle.hierarchy_As(D.e_graph(), hier)
    assert np.array_equal(ref.embed(As, hier, d, seed=man["cases"]["embed"]["seed"]), g[f"x_d{d}"])
