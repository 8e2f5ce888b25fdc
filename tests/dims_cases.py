"""The cases above dimension 4 recorded from the reference binary
(tests/golden/make_ref_dims.py writes tests/golden/ref_dims_*.npz and
ref_dims_manifest.json from them), replayed by tests/test_dims.py (oracle, live
binary) and tests/test_gpu_dims.py (device paths).  Same conventions as
tests/ref_cases.py: inputs are rebuilt from tests/graphs.py and hashed in the
manifest; a fixture holds outputs of the reference only.

One .npz per function and dimension, one array per case.
"""
import functools
import json
import os

import numpy as np

import graphs as G
import ref_cases as C

MANIFEST = os.path.join(C.GOLDEN, "ref_dims_manifest.json")
DIMS = (5, 8, 16)       # fixtures: the first wide dimension, a record-width change, the bound
ALL_DIMS = tuple(range(5, 17))
E_DIMS = (5, 16)

FA_N = 130              # past the one-workgroup default (64): the fused step; > 2 blocks at G = 64
ML_ITERS = 12


def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def load(kind, dim):
    return dict(np.load(os.path.join(C.GOLDEN, f"ref_dims_{kind}_d{dim}.npz"), allow_pickle=False))


def load_embed():
    """The hierarchy (C.hier_from(g, "h")) and x_d<dim> of the embed case."""
    return dict(np.load(os.path.join(C.GOLDEN, "ref_dims_embed.npz"), allow_pickle=False))


# --------------------------------------------------------------------------
# single-level forceAtlas on ER(130, 0.06)

@functools.lru_cache(maxsize=None)
def fa_graph():
    return C._canon(G.erdos_renyi(FA_N, 0.06, seed=130))


def _start(dim):
    return G.random_coords(FA_N, dim, seed=100 + dim)


def _opt_nohubs(dim):
    return C._fa(fa_graph(), dim, _start(dim), 2, nohubs=1)


def _opt_unweighted(dim):
    # fractional weights that use_weights = 0 must ignore
    return C._fa(C.symmetric_weights(fa_graph()), dim, _start(dim), 2, use_weights=0)


def _opt_repel(dim):
    # repel outside weight_ok (2^60): the `/` bodies for every pair
    return C._fa(fa_graph(), dim, _start(dim), 2, repel=2.0 ** 70)


def _opt_tiny(dim):
    x0 = _start(dim)
    x0[77, dim - 1] = C.TINY  # the last component of one vertex outside coord_ok
    return C._fa(fa_graph(), dim, x0, 2)


def _opt_coincident(dim):
    x0 = _start(dim)
    x0[41] = x0[40]  # distance 0: the eps clamp
    return C._fa(fa_graph(), dim, x0, 2)


def _opt_selfloop(dim):
    ip, ix, _ = fa_graph()
    rows = np.repeat(np.arange(FA_N), np.diff(ip)).astype(np.int64)
    A = G.csr_from_edges(FA_N, np.concatenate([rows, [9]]), np.concatenate([ix.astype(np.int64), [9]]))
    assert 9 in A[1][A[0][9]:A[0][10]]
    return C._fa(A, dim, _start(dim), 2)


def _opt_isolated(dim):
    ip, ix, _ = fa_graph()
    rows = np.repeat(np.arange(FA_N), np.diff(ip)).astype(np.int64)
    keep = (rows != 23) & (ix != 23)
    A = G.csr_from_edges(FA_N, rows[keep], ix[keep].astype(np.int64))
    assert A[0][24] == A[0][23]
    return C._fa(A, dim, _start(dim), 2)


FA_OPTIONS = {
    "nohubs": _opt_nohubs, "unweighted": _opt_unweighted, "repel_2p70": _opt_repel,
    "tiny": _opt_tiny, "coincident": _opt_coincident, "selfloop": _opt_selfloop,
    "isolated": _opt_isolated,
}
FA_ITERS = (1, 2, 25)


def fa_names():
    return ([f"start_it{k}" for k in FA_ITERS] + [f"seeded_it{k}" for k in FA_ITERS]
            + list(FA_OPTIONS))


@functools.lru_cache(maxsize=None)
def fa_case(name, dim):
    if name in FA_OPTIONS:
        return FA_OPTIONS[name](dim)
    kind, it = name.split("_it")
    if kind == "start":
        return C._fa(fa_graph(), dim, _start(dim), int(it))
    return C._fa(fa_graph(), dim, None, int(it), seed=4200 + dim)


# --------------------------------------------------------------------------
# forceAtlasMultilevel

@functools.lru_cache(maxsize=None)
def er90():
    return C._canon(G.erdos_renyi(90, 0.08, seed=90))


def _ml_er90(dim):
    import oracle_lib as O
    A = er90()
    PT = O.partition(A, 0.2)[0]
    m = PT[2]
    return dict(A=A, PT=(PT[0], PT[1]), vA=C.vertex_of(PT), cA=G.random_coords(m, dim, seed=m),
                rA=np.random.RandomState(m).uniform(0.0, 0.6, m), dim=dim, iterations=ML_ITERS,
                seed=17, kw={})


def _ml_m1(dim):
    # M1's graph and aggregates (1..256 members: the packed classes) at this dimension
    sizes = C.M1_SIZES
    return C._ml(C.layout_graph("packed"), sizes, sum(sizes), dim, ML_ITERS, 31)


def _ml_m2(dim):
    # M2's streamed aggregates and hub rows; fits the fixture size at dim 5 only
    return C._m2(dim, 1.5)


ML_CASES = {"er90": _ml_er90, "M1": _ml_m1, "M2": _ml_m2}


def ml_names(dim):
    return ["er90", "M1"] + (["M2"] if dim == 5 else [])


@functools.lru_cache(maxsize=None)
def ml_case(name, dim):
    return ML_CASES[name](dim)


# --------------------------------------------------------------------------
# embed on ER(300, 0.03) with partition(A, 0.2)

E_SEED = 11


E_CF = 0.2


@functools.lru_cache(maxsize=None)
def e_graph():
    # (its largest component: embed wants a connected graph; ER(300, 0.03) is one)
    return C._canon(G.largest_component(G.erdos_renyi(300, 0.03, seed=300)))
