"""Dimension 8 across two ranks (csrc/ge_dist.hip): row-sharded forceAtlas and
aggregate-sharded forceAtlasMultilevel over the library's transport communicator, as
tests/test_gpu_dist.py starts them, equal the single-GPU bits (and the oracle) on
every rank.  The shards run the same plans as one GPU -- above dimension 4 the fused
step on a row range and the ordered-pair kernel on a split aggregate's row tiles --
and the padding to nranks * ceil(n / nranks) rows is per row, whatever the dimension.
"""
import os
import socket

import numpy as np
import pytest

import ge_amd as ge
import graphs as G
import ref_cases as C

pytestmark = pytest.mark.gpu

DIM = 8
SPLIT_SIZES = [700, 257, 100, 90, 1]  # 100 members: 2 row tiles, one per rank


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _inputs():
    n = sum(SPLIT_SIZES)
    A = G.with_hubs(G.rmat(n, 8 * n, seed=17), [(3, 600)], seed=3)  # 1148 vertices: odd shards
    PT = C.block_partition(n, SPLIT_SIZES, seed=5)
    PT = (PT[0], PT[1], len(SPLIT_SIZES), n)
    m = len(SPLIT_SIZES)
    return (A, PT, G.random_coords(m, DIM, seed=m),
            np.random.RandomState(m).uniform(0.0, 0.6, m), G.random_coords(n, DIM, seed=4))


def _run_all(api, inputs):
    A, PT, cA, rA, X0 = inputs
    return {"fa": api.force_atlas(A, DIM, coords=X0, iterations=5),
            "fa_seeded": api.force_atlas(A, DIM, iterations=3, seed=21, repel=1.5, normalize=1),
            "faml": api.force_atlas_ml(A, PT, ge.vertex_of(PT), cA, rA, DIM, iterations=6, seed=9)}


def _worker(rank, world, port, out_path, split_min):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GE_DIST_REPLICA_MAX="0")
    if split_min:
        os.environ["GE_DIST_SPLIT_MIN"] = split_min
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = ge.Context(0)
    comm = ge.Comm(ctx, world, rank, backend="transport")
    res = _run_all(comm, _inputs())
    np.savez(out_path % rank, **res)
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def single(ctx):
    return _run_all(ctx, _inputs())


def test_single_gpu_matches_oracle(oracle, single):
    A, PT, cA, rA, X0 = _inputs()
    assert np.array_equal(single["fa"], oracle.force_atlas(A, DIM, coords=X0, iterations=5))
    assert np.array_equal(single["faml"],
                          oracle.force_atlas_ml(A, PT, ge.vertex_of(PT), cA, rA, DIM,
                                                iterations=6, seed=9))


@pytest.mark.parametrize("split_min", [None, "100"], ids=["whole-aggregates", "split-row-tiles"])
def test_two_transport_ranks_match_single_gpu(tmp_path, single, split_min):
    import torch.multiprocessing as mp
    if split_min:  # the three aggregates of >= 100 members are dealt out by row tiles
        A, PT = _inputs()[:2]
        owner = ge.assign_aggregates_split(PT, A[0], 2, int(split_min))
        assert list(owner[:3]) == [-1, -1, -1] and (owner[3:] >= 0).all()
    out = str(tmp_path / "r%d.npz")
    mp.start_processes(_worker, args=(2, _free_port(), out, split_min), nprocs=2, join=True,
                       start_method="spawn")
    for r in range(2):
        got = dict(np.load(out % r))
        for k, v in single.items():
            assert np.array_equal(got[k], v), (r, k)
