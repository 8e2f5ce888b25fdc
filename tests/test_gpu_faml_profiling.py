"""The multilevel plan's profiling readers count what was timed since the last
ge_faml_plan_set_profiling call: that call rewinds the event pools, so runs made
before it are not averaged in."""
import numpy as np
import pytest

import ge_amd as ge
import graphs as G
import ref_cases as C

pytestmark = pytest.mark.gpu

K_LOOK = 16
# EDGE_SIZES of test_gpu_sym_prio.py with one aggregate at each edge of the small and
# mid classes (case a of tests/golden/faml_sched.json)
SIZES = [2600, 321, 64 * K_LOOK, 64 * K_LOOK + 1, 64 * (K_LOOK + 1) + 1, 320, 257, 1, 64, 65, 256]


def test_counts_after_reset(ctx, monkeypatch):
    import torch
    monkeypatch.setenv("GE_FAML_RES_CAP", "256")
    n, dim, iters = sum(SIZES), 2, 3
    case = C._ml(C.symmetric_weights(G.rmat(n, 8 * n, seed=3)), SIZES, 13, dim, iters, 29)
    A, PT = case["A"], case["PT"]
    dev = torch.device("cuda:0")

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    i32, f64 = np.int32, np.float64
    d = [up(A[0], i32), up(A[1], i32), up(A[2], f64), up(PT[0], i32), up(PT[1], i32),
         up(case["vA"], i32), up(case["cA"], f64), up(case["rA"], f64),
         up(ge.uniform_stream(case["seed"], n * dim), f64)]
    ptr = [t.data_ptr() for t in d]
    X = torch.zeros((n, dim), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    plan = ge.FamlPlan(ctx, n, ptr[0], ptr[1], ptr[2], PT[0], ptr[3], ptr[4], ptr[5], dim,
                       iterations=iters)
    try:
        def run():
            plan.run(ptr[6], ptr[7], ptr[8], X.data_ptr())
            ctx.sync()

        def counts():
            return plan.kernel_ms()[2], plan.repulse_ms()[1], plan.rows_ms()[1]

        run()  # not profiled
        assert counts() == (0, 0, 0)
        plan.set_profiling(True)
        run()
        run()
        assert counts() == (2, 2 * iters, 2 * iters)
        plan.set_profiling(True)  # rewinds
        run()
        assert counts() == (1, iters, iters)
        assert all(t >= 0.0 for t in plan.kernel_ms()[:2])
    finally:
        plan.close()
