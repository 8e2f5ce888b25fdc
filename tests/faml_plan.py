"""Runs a multilevel case through ge_faml_plan_* on device-resident arrays and says
which kernels ran it (test infrastructure for the GPU tests).

run_plan returns the coordinates with the plan's census (FamlPlan.classes()) and
schedule (FamlPlan.schedule()); expected_classes restates the scheduler's
bucketing (classes_and_packs, graph-embed_amd/csrc/ge_faml_sched.hpp) from the
sizes, the dimension and the device's CU count, so a test asserts the path it means to cover instead of
claiming it in a comment.
"""
import math

import numpy as np

import ge_amd as ge


def large_cap(dim):
    """Members the one-aggregate-per-block resident kernel holds in LDS (ge_faml.hip)."""
    return 4096 if dim + 1 <= 4 else 2048


def run_plan(ctx, case, init=None):
    """case: a ref_cases multilevel case.  init: the n * dim starting values in P_T
    storage order (default: the seeded stream).  Returns (X, classes, schedule)."""
    import torch
    A, PT, dim = case["A"], case["PT"], case["dim"]
    n = len(A[0]) - 1
    if init is None:
        init = ge.uniform_stream(case["seed"], n * dim)
    dev = torch.device("cuda:0")

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    i32, f64 = np.int32, np.float64
    d = [up(A[0], i32), up(A[1], i32), up(A[2], f64), up(PT[0], i32), up(PT[1], i32),
         up(case["vA"], i32), up(case["cA"], f64), up(case["rA"], f64),
         up(np.asarray(init).reshape(-1), f64)]
    assert d[8].numel() == n * dim
    ptr = [t.data_ptr() for t in d]
    X = torch.zeros((n, dim), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    plan = ge.FamlPlan(ctx, n, ptr[0], ptr[1], ptr[2], PT[0], ptr[3], ptr[4], ptr[5], dim,
                       iterations=case["iterations"], **case["kw"])
    try:
        plan.run(ptr[6], ptr[7], ptr[8], X.data_ptr())
        ctx.sync()
        classes, schedule = plan.classes(), plan.schedule()
    finally:
        plan.close()
    return X.cpu().numpy(), classes, schedule


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_classes(sizes, dim, knob=None):
    """(res_cap, {class: sizes}) as faml_plan_build buckets them.  knob: the value of
    GE_FAML_RES_CAP the test set (None: the plan's rule from the CU count)."""
    sizes = [int(s) for s in sizes]
    if knob is None:
        cap = int(math.sqrt(float(sum(s * s for s in sizes)) / max(cu_count(), 1) / 4.0))
    else:
        cap = int(knob)
    cap = max(256, min(cap, large_cap(dim)))
    return cap, {"small": [s for s in sizes if 0 < s <= 64],
                 "mid": [s for s in sizes if 64 < s <= 256],
                 "large": [s for s in sizes if 256 < s <= cap],
                 "streamed": [s for s in sizes if s > cap]}


def _packs(sizes, cap):
    """Blocks of build_packs(ids by descending size, cap, max_aggs = cap)."""
    blocks = tot = cnt = 0
    for s in sorted(sizes, reverse=True):
        if cnt > 0 and (tot + s > cap or cnt >= cap):
            blocks += 1
            tot = cnt = 0
        tot += s
        cnt += 1
    return blocks + (cnt > 0)


def assert_census(classes, sizes, dim, knob=None):
    """The plan put every aggregate in the class the rule implies and launches the
    resident kernels with the blocks that follow.  Returns the expected sizes by class."""
    cap, want = expected_classes(sizes, dim, knob)
    assert classes["res_cap"] == cap, (classes, cap)
    for k, v in want.items():
        assert classes[k] == len(v), (k, classes, want)
    assert classes["blocks_small"] == _packs(want["small"], 64), classes
    assert classes["blocks_mid"] == _packs(want["mid"], 256), classes
    assert classes["blocks_large"] == len(want["large"]), classes
    return want


def assert_schedule(schedule, classes, streamed_sizes, mode):
    """mode: 'sweeps' (GE_FAML_SYM_CHAIN=0), 'row-blocks' (1e9), 'ordered' (GE_FAML_SYM=0),
    None (the plan's own mix)."""
    tiles = sum((s + 63) // 64 for s in streamed_sizes)
    k = len(streamed_sizes)
    assert classes["streamed"] == k
    if mode == "ordered":
        assert (schedule["sweeps"], schedule["row_blocks"], schedule["units"]) == (0, 0, 0), schedule
        return
    assert schedule["units"] == tiles, (schedule, tiles)
    assert schedule["sweeps"] + schedule["row_blocks"] == k, schedule
    if mode == "sweeps":
        assert schedule["sweeps"] == k, schedule
    elif mode == "row-blocks":
        assert schedule["row_blocks"] == k, schedule
