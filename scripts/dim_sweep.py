"""One iteration per embedding dimension, single level and multilevel, on the graph
of `bench.py --workload c3` (R-MAT 1M ids / 8M draws, largest component; level 0 of
partition(A, 0.125)).  One JSON line per case: HIP events on the library's stream, one
warm-up, then the median of --reps runs with [min, max].

    python scripts/dim_sweep.py [--dims 3,4,5,8,12,16] [--reps 5] [--out FILE]

At d <= 4 each leg is measured three times: the shipped default, the ordered-pair
schedule chosen with the existing knobs (GE_FA_SYM=0 / GE_FAML_SYM=0: the like-for-like
baseline of the kernels above d = 4), and the wide schedule itself (GE_WIDE_MIN_DIM=1).
`ns_per_pair` is the step's time over the ordered pairs it evaluates (n (n - 1), or the
sum of s (s - 1) over the aggregates); the single-level figure is the repulsion kernel
alone where the plan's own events separate it (`rep_ms`).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "graph-embed_amd", "py"))
import ge_amd as ge  # noqa: E402

KNOBS = ("GE_FA_SYM", "GE_FAML_SYM", "GE_WIDE_MIN_DIM")
SCHEDULES = {"default": {}, "ordered": {"GE_FA_SYM": "0", "GE_FAML_SYM": "0"},
             "wide": {"GE_WIDE_MIN_DIM": "1"}}


def set_schedule(name):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(SCHEDULES[name])


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "runs_ms": [round(v, 4) for v in ms]}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=8_000_000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--dims", default="3,4,5,8,12,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="single,multilevel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dims = [int(x) for x in args.dims.split(",")]
    dev = torch.device("cuda:0")
    ctx = ge.Context(0)
    work = torch.cuda.Stream(dev)
    torch.cuda.set_stream(work)
    ctx.set_stream(work.cuda_stream)
    L = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=True)
    n, nnz = len(L[0]) - 1, len(L[1])
    PT = ctx.partition(L, 0.125)[0]
    m = PT[2]
    vA = ge.vertex_of(PT)
    sizes = np.diff(PT[0]).astype(np.float64)
    ml_pairs = float((sizes * (sizes - 1)).sum())
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g = dict(ip=T(L[0]), ix=T(L[1]), dx=T(L[2]), pip=T(PT[0]), pix=T(PT[1]), vA=T(vA))
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(fn, warm=True):
        if warm:
            fn()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(work)
            fn()
            b.record(work)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    for d in dims:
        for sched in (["default", "ordered", "wide"] if d <= 4 else ["default"]):
            set_schedule(sched)
            base = {"dim": d, "schedule": sched, "n": n, "nnz": nnz}
            if "single" in args.legs:
                x = T(ge.uniform_stream(args.seed, n * d).reshape(n, d))
                y = torch.empty_like(x)
                plan = ctx.fa_plan(n, nnz, g["ip"].data_ptr(), g["ix"].data_ptr(),
                                   g["dx"].data_ptr(), d, 0, n)
                plan.step(x.data_ptr(), y.data_ptr())  # warm-up, outside the plan's own events
                plan.set_profiling(True)
                ms = timed(lambda: plan.step(x.data_ptr(), y.data_ptr()), warm=False)
                rep_ms, attr_ms, _ = plan.kernel_ms()
                plan.close()
                pairs = float(n) * (n - 1)
                rec = dict(base, leg="single", pairs=pairs, rep_ms=rep_ms, attr_ms=attr_ms,
                           ns_per_pair=1e6 * rep_ms / pairs, **stats(ms))
                emit(rec)
                del x, y
            if "multilevel" in args.legs:
                cA = T(ge.uniform_stream(args.seed + 1, m * d).reshape(m, d))
                rA = T(0.01 + 0.19 * (ge.uniform_stream(args.seed + 2, m) + 1.0) / 2.0)
                init = T(ge.uniform_stream(args.seed, n * d))
                X = torch.zeros((n, d), dtype=torch.float64, device=dev)
                plan = ge.FamlPlan(ctx, n, g["ip"].data_ptr(), g["ix"].data_ptr(),
                                   g["dx"].data_ptr(), PT[0], g["pip"].data_ptr(),
                                   g["pix"].data_ptr(), g["vA"].data_ptr(), d, iterations=1)
                ms = timed(lambda: plan.run(cA.data_ptr(), rA.data_ptr(), init.data_ptr(),
                                            X.data_ptr()))
                cls, sch = plan.classes(), plan.schedule()
                plan.close()
                rec = dict(base, leg="multilevel", aggregates=m, pairs=ml_pairs,
                           ns_per_pair=1e6 * statistics.median(ms) / ml_pairs, classes=cls,
                           sweeps=sch, **stats(ms))
                emit(rec)
                del cA, rA, init, X
    for k in KNOBS:
        os.environ.pop(k, None)
    ctx.close()


if __name__ == "__main__":
    main()
