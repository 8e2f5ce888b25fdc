"""Which single-level kernel a test reaches, from the schedule (ge_amd.fa_schedule, no
device): the knob tests assert the path their docstring names, so that a threshold that
moves fails them instead of sending them down another kernel unnoticed.

The names: "fa_small_strict" (every iteration in one workgroup), "fa_grouped_persistent",
and for the per-iteration path the step's kernels -- "fa_grouped_step",
"fa_grouped_stream", or the split step's repulsion ("fa_repulse_grouped",
"fa_repulse_strict", "fa_repulse_strict_wide", "fa_repulse_fast", "sweeps", "farfield")
followed by "+rows".  The CU count enters the grids only, not the route.
"""
import ge_amd as ge

_REP = {"grouped": "fa_repulse_grouped", "ordered": "fa_repulse_strict",
        "ordered_wide": "fa_repulse_strict_wide", "fast": "fa_repulse_fast", "sweeps": "sweeps",
        "farfield": "farfield"}
_STEP = {"fused": "fa_grouped_step", "stream": "fa_grouped_stream"}


def schedule(n, dim, **kw):
    return ge.fa_schedule(n, dim, 256, **kw)


def step_kernel(n, dim, **kw):
    """What a plan's step launches (rb, re and ge_amd.params keywords in kw)."""
    s = schedule(n, dim, **kw)
    return _STEP.get(s["step"]) or _REP[s["rep"]] + "+rows"


def repulse_kernel(n, dim, **kw):
    """What the split step's repulsion pass and FaPlan.repulse launch."""
    return _REP[schedule(n, dim, **kw)["rep"]]


def run_kernel(A, dim, iterations, **kw):
    """What ge_force_atlas runs on the graph A for `iterations`: the one-workgroup run, the
    persistent kernel where it is tried, else the step's kernels."""
    n, nnz = len(A[0]) - 1, len(A[1])
    s = schedule(n, dim, iterations=iterations, nnz=nnz, **kw)
    if s["small"]:
        return "fa_small_strict"
    if s["persist"]:
        return "fa_grouped_persistent"
    return step_kernel(n, dim, **kw)
