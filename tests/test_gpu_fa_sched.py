"""A live single-level plan holds the schedule the host function gives
(graph-embed_amd/csrc/ge_fa_sched.hpp): FaPlan.schedule() equals ge_amd.fa_schedule for the
plan's arguments, the knobs in the environment and the device's CU count, on one plan per
route; and the route is a property of the plan: a second plan created identically takes the
same step, bit for bit.  tests/test_fa_sched.py pins the rules themselves without a device.
"""
import numpy as np
import pytest

import ge_amd as ge
import graphs as G

pytestmark = pytest.mark.gpu

KNOBS = ("GE_STREAM_MAX", "GE_GRP_G", "GE_GRP_SPLIT", "GE_REP_BLOCKS", "GE_REP_R", "GE_FA_SYM",
         "GE_FAR_MIN", "GE_FAR_R", "GE_WIDE_MIN_DIM")

# name: n, dim, rows (None: the whole level), env, params, negative-mass row, and the route
# the case is here for (step, rep)
CASES = {
    "fused_step": (300, 3, None, {}, {}, None, ("fused", "grouped")),
    "fused_stream": (3100, 3, None, {}, {}, None, ("stream", "ordered")),
    "sweeps": (3100, 3, None, {"GE_STREAM_MAX": "0"}, {}, None, ("split", "sweeps")),
    "row_shard": (3100, 3, (1000, 2100), {"GE_STREAM_MAX": "0"}, {}, None, ("split", "ordered")),
    "fast": (300, 3, None, {}, {"mode": ge.MODE_FAST}, None, ("split", "fast")),
    "farfield_active": (300, 3, None, {"GE_FAR_MIN": "256"}, {"mode": ge.MODE_FARFIELD}, None,
                        ("split", "farfield")),
    "farfield_mass": (300, 3, None, {"GE_FAR_MIN": "256"}, {"mode": ge.MODE_FARFIELD}, 77,
                      ("split", "fast")),
    "wide": (700, 16, None, {}, {}, None, ("stream", "ordered_wide")),
}


def _graph(n, bad_row):
    ip, ix, dx = G.rmat(n, 5 * n, seed=n)
    if bad_row is not None:  # deg + 1 <= 0 on one row: the far field's mass check rejects it
        dx = dx.copy()
        assert ip[bad_row + 1] - ip[bad_row] >= 1
        dx[ip[bad_row]:ip[bad_row + 1]] = -1.0
    return ip, ix, dx


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_holds_the_host_schedule(ctx, monkeypatch, name):
    torch = pytest.importorskip("torch")
    n, dim, rows, env, params, bad_row, route = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rb, re = rows or (0, n)
    A = _graph(n, bad_row)
    dev = torch.device("cuda:0")
    ip = torch.from_numpy(A[0].astype(np.int32)).to(dev)
    ix = torch.from_numpy(A[1].astype(np.int32)).to(dev)
    dx = torch.from_numpy(A[2]).to(dev)
    x = torch.from_numpy(G.random_coords(n, dim, seed=3)).to(dev)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = ge.fa_schedule(n, dim, cus, rb=rb, re=re, masses_ok=bad_row is None, **params)
    outs = []
    for _ in range(2):
        plan = ctx.fa_plan(n, len(A[1]), ip.data_ptr(), ix.data_ptr(), dx.data_ptr(), dim, rb, re,
                           **params)
        got = plan.schedule()
        y = torch.zeros_like(x)
        plan.step(x.data_ptr(), y.data_ptr())
        ctx.sync()
        far = plan.far_info()
        plan.close()
        assert got == {k: want[k] for k in ge.FA_SCHED_PLAN_SCALARS}
        assert (got["step"], got["rep"]) == route
        assert far["reason"] == got["far_reason"] and far["active"] == (got["rep"] == "farfield")
        outs.append(y[rb:re].cpu().numpy())
    assert np.isfinite(outs[0]).all() and outs[0].any()
    assert outs[0].tobytes() == outs[1].tobytes()
    if name == "farfield_mass":
        assert want["far_reason"] == "mass" and want["mode"] == ge.MODE_FAST
    if name == "wide":
        assert want["wide"] and want["lanes"] == 64 and not want["repel_one"]
