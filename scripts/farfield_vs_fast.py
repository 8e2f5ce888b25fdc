"""GE_MODE_FARFIELD against GE_MODE_FAST on the C2 graph (BASELINE.json configs[1], built
as bench.py builds it: the 1M-id device R-MAT, the reference's random start).

For each dimension (--dims 2,3) a FAST plan and one FARFIELD plan per theta (--thetas
0.25,0.5,0.75) are built in one process over the same graph and stepped interleaved
(one warm-up step each, then --rounds >= 3 alternations of --steps steps, wall time
around a synchronised block plus the plans' HIP-event split).  Records, one JSON line
each: "round" (ms per step, repulsion / attraction ms; for FARFIELD also the pass
before the item kernel -- box, keys, sort, records, summaries -- against the item
kernel, the cells accepted per level and the pair terms per row), "summary" per theta
(ranges, ratio, whether the FARFIELD range lies wholly below FAST's), with
--crossover the same comparison at d = 3, theta = 0.5 for n = 2^13 .. 2^20 (GE_FAR_MIN=0;
the plan's default far_min is the smallest n at which FARFIELD wins), with --items the
C2 step for 64- and 256-row items (GE_FAR_R) and the partners of the item with the
largest ball ("worst_item": the launch ends with it), and "drift": max |dX| / max |X| against
STRICT after 1, 2, 10 and 100 iterations on a graph small enough for STRICT (--drift-n).

  python scripts/farfield_vs_fast.py --rounds 3 --steps 2 --crossover --items \
      > profiles/r13/farfield_vs_fast.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "graph-embed_amd", "py"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import far_cases as F  # noqa: E402  (the numpy restatement of the walk)
import ge_amd as ge  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


class Graph:
    def __init__(self, ctx, dev, n, draws, dim, seed):
        self.ctx, self.dev, self.dim = ctx, dev, dim
        A = ctx.rmat_csr(n, draws, seed=seed)
        self.A = A
        self.n, self.nnz = len(A[0]) - 1, len(A[1])
        self.X0 = ge.uniform_stream(seed, self.n * dim).reshape(self.n, dim)
        self.t = [torch.from_numpy(a).to(dev) for a in A]
        self.x = [torch.from_numpy(self.X0).to(dev), torch.zeros((self.n, dim), dtype=torch.float64,
                                                                 device=dev)]

    def plan(self, **kw):
        return self.ctx.fa_plan(self.n, self.nnz, *(t.data_ptr() for t in self.t), self.dim, 0,
                                self.n, **kw)

    def steps(self, plan, k):
        """k steps from the start coordinates; (wall ms per step, repulsion ms, attraction ms)."""
        self.x[0].copy_(torch.from_numpy(self.X0))
        torch.cuda.synchronize(self.dev)
        plan.set_profiling(True)
        t0 = time.perf_counter()
        a, b = self.x
        for _ in range(k):
            plan.step(a.data_ptr(), b.data_ptr())
            a, b = b, a
        self.ctx.sync()
        ms = (time.perf_counter() - t0) / k * 1e3
        rep, att, _ = plan.kernel_ms()
        plan.set_profiling(False)
        return ms, rep, att


def compare(g, plans, steps, rounds, tag):
    """plans: {name: plan}, 'fast' among them.  Interleaved rounds; returns {name: [ms]}."""
    for p in plans.values():
        g.steps(p, 1)  # warm-up
    ms = {k: [] for k in plans}
    for rnd in range(rounds):
        for name, p in plans.items():
            step, rep, att = g.steps(p, steps)
            ms[name].append(step)
            rec = dict(record="round", round=rnd, plan=name, n=g.n, dim=g.dim, steps=steps,
                       ms_per_step=step, repulse_ms=rep, attract_ms=att, **tag)
            info = p.far_info()
            if info["active"]:
                rec.update(theta=info["theta"], item_rows=info["item_rows"],
                           prep_ms=info["prep_ms"], item_ms=info["item_ms"],
                           accepted=info["accepted"], exact_leaves=info["exact_leaves"],
                           terms_per_row=info["pair_terms"] / g.n, fallback=info["fallback"])
            emit(**rec)
    lo, hi = min(ms["fast"]), max(ms["fast"])
    for name, v in ms.items():
        if name != "fast":
            emit(record="summary", plan=name, n=g.n, dim=g.dim, fast_ms_range=[lo, hi],
                 far_ms_range=[min(v), max(v)],
                 ratio_fast_over_far=float(np.median(ms["fast"]) / np.median(v)),
                 far_wholly_below_fast=max(v) < lo, **tag)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=8_000_000)
    ap.add_argument("--dims", default="2,3")
    ap.add_argument("--thetas", default="0.25,0.5,0.75")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--items", action="store_true")
    ap.add_argument("--drift", default="1,2,10,100")
    ap.add_argument("--drift-n", type=int, default=50_000)
    args = ap.parse_args()
    assert args.rounds >= 3, "at least 3 alternations"
    os.environ["GE_FAR_MIN"] = "0"
    ctx = ge.Context(0)
    dev = torch.device("cuda:0")
    thetas = [float(t) for t in args.thetas.split(",") if t]

    for dim in [int(d) for d in args.dims.split(",") if d]:
        g = Graph(ctx, dev, args.n, args.draws, dim, args.seed)
        plans = {"fast": g.plan(mode=ge.MODE_FAST)}
        for th in thetas:
            plans[f"far{th:g}"] = g.plan(mode=ge.MODE_FARFIELD, theta=th)
        compare(g, plans, args.steps, args.rounds, dict(what="c2"))
        for p in plans.values():
            p.close()
        if args.items and dim == 3:
            plans = {"fast": g.plan(mode=ge.MODE_FAST)}
            for r in ("1", "4"):
                os.environ["GE_FAR_R"] = r
                plans[f"far_R{r}"] = g.plan(mode=ge.MODE_FARFIELD, theta=0.5)
            del os.environ["GE_FAR_R"]
            compare(g, plans, args.steps, args.rounds, dict(what="items"))
            # the item kernel ends with its most expensive item: the partners of the item
            # with the largest ball against the average (tests/far_cases.py's walk)
            for name in ("far_R1", "far_R4"):
                lay, info = plans[name].far_layout(), plans[name].far_info()
                q = int(np.argmax(lay["items"][:, dim + 1]))
                k = sum(1 if ok else F.cell_range(0, idx, g.n)[1] - F.cell_range(0, idx, g.n)[0]
                        for _, idx, ok in F.walk(lay, q, g.n))
                emit(record="worst_item", plan=name, n=g.n, dim=dim, item=q,
                     radius=float(lay["items"][q, dim + 1]),
                     median_radius=float(np.median(lay["items"][:, dim + 1])),
                     partners=int(k), mean_partners=info["pair_terms"] / g.n)
            for p in plans.values():
                p.close()
        del g

    if args.crossover:
        for lg in range(13, 21):
            n = 1 << lg
            g = Graph(ctx, dev, n, 8 * n, 3, args.seed)
            plans = {"fast": g.plan(mode=ge.MODE_FAST),
                     "far0.5": g.plan(mode=ge.MODE_FARFIELD, theta=0.5)}
            compare(g, plans, 20 if lg <= 16 else 2, args.rounds, dict(what="crossover"))
            for p in plans.values():
                p.close()

    its = [int(x) for x in args.drift.split(",") if x]
    if its:
        for dim in (2, 3):
            g = Graph(ctx, dev, args.drift_n, 8 * args.drift_n, dim, args.seed)
            for it in its:
                ref = ctx.force_atlas(g.A, dim, coords=g.X0, iterations=it, mode=ge.MODE_STRICT)
                row = {"fast": ctx.force_atlas(g.A, dim, coords=g.X0, iterations=it,
                                               mode=ge.MODE_FAST)}
                for th in thetas:
                    row[f"far{th:g}"] = ctx.force_atlas(g.A, dim, coords=g.X0, iterations=it,
                                                        mode=ge.MODE_FARFIELD, theta=th)
                emit(record="drift", n=g.n, dim=dim, iterations=it,
                     max_dx_over_max_x={k: float(np.abs(v - ref).max() / np.abs(ref).max())
                                        for k, v in row.items()},
                     finite=bool(all(np.isfinite(v).all() for v in row.values())))
    ctx.close()


if __name__ == "__main__":
    main()
