"""GE_MODE_FAST against GE_MODE_STRICT on the C4 multilevel level (BASELINE.json
configs[3], built as bench.py builds it: device R-MAT, LCC, device partition, level 0).

K steps of a STRICT plan and of a FAST plan are timed interleaved on one box
(--rounds alternations, profiling events on), then the drift max |dX| / max |X| of
FAST against STRICT after 1, 2, 10 and 100 iterations, then with --shares N[,N..] the
per-rank shares of scripts/scale_sim.py (ge_assign_aggregates, each share a subset
plan, one after another on this GPU) in both modes.  One JSON line per record; the
"summary" record carries the ratio and whether the ranges of the interleaved runs
overlap (FAST has no reason to exist unless they do not and it is the faster one).

  python scripts/faml_fast_vs_strict.py --steps 5 --rounds 3 --shares 4,8
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
import ge_amd as ge  # noqa: E402

MODES = (("strict", ge.MODE_STRICT), ("fast", ge.MODE_FAST))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--draws", type=int, default=80_000_000)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--drift", default="1,2,10,100")
    ap.add_argument("--shares", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least 3 alternations"

    ctx = ge.Context(0)
    dev = torch.device("cuda:0")
    L = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=True)
    PT = ctx.partition(L, 0.125)[0]
    n0, m, dim = len(L[0]) - 1, PT[2], args.dim
    vA = ge.vertex_of(PT)
    cA = ge.uniform_stream(args.seed + 1, m * dim).reshape(m, dim)
    rA = 0.01 + 0.19 * (ge.uniform_stream(args.seed + 2, m) + 1.0) / 2.0
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = dict(ip=T(L[0]), ix=T(L[1]), dx=T(L[2]), pip=T(PT[0]), pix=T(PT[1]), vA=T(vA),
             cA=T(cA), rA=T(rA), init=T(ge.uniform_stream(args.seed, n0 * dim)))
    X = {k: torch.zeros((n0, dim), dtype=torch.float64, device=dev) for k, _ in MODES}
    torch.cuda.synchronize(dev)

    def plan(iters, mode, aggs=None):
        return ge.FamlPlan(ctx, n0, d["ip"].data_ptr(), d["ix"].data_ptr(), d["dx"].data_ptr(),
                           PT[0], d["pip"].data_ptr(), d["pix"].data_ptr(), d["vA"].data_ptr(), dim,
                           iterations=iters, aggs=aggs, mode=mode)

    def run(p, name):
        p.run(d["cA"].data_ptr(), d["rA"].data_ptr(), d["init"].data_ptr(), X[name].data_ptr())
        ctx.sync()

    def timed(p, name, iters):
        p.set_profiling(True)  # restarts the plan's event counters
        t0 = time.perf_counter()
        run(p, name)
        ms = (time.perf_counter() - t0) / iters * 1e3
        return ms, p.repulse_ms()[0], p.rows_ms()[0]

    K = args.steps
    plans = {name: plan(K, mode) for name, mode in MODES}
    cls = plans["fast"].classes()
    print(json.dumps({"record": "level", "n": n0, "nnz": len(L[1]), "aggregates": m, "dim": dim,
                      "streamed": cls["streamed"], "res_cap": cls["res_cap"],
                      "pairs_per_launch": plans["fast"].repulse_ms()[2],
                      "fast_mode": plans["fast"].mode(), "strict_schedule": plans["strict"].schedule(),
                      "fast_schedule": plans["fast"].schedule()}), flush=True)
    for name, _ in MODES:
        run(plans[name], name)  # warm-up
    ms = {name: [] for name, _ in MODES}
    for rnd in range(args.rounds):
        for name, _ in MODES:
            step, rep, rows = timed(plans[name], name, K)
            ms[name].append(step)
            print(json.dumps({"record": "round", "round": rnd, "mode": name, "steps": K,
                              "ms_per_step": step, "repulse_ms": rep, "rows_ms": rows}), flush=True)
    for p in plans.values():
        p.close()
    lo = {k: min(v) for k, v in ms.items()}
    hi = {k: max(v) for k, v in ms.items()}
    print(json.dumps({"record": "summary", "N": 1, "strict_ms_range": [lo["strict"], hi["strict"]],
                      "fast_ms_range": [lo["fast"], hi["fast"]],
                      "ratio_strict_over_fast": float(np.median(ms["strict"]) / np.median(ms["fast"])),
                      "ranges_overlap": not (hi["fast"] < lo["strict"] or hi["strict"] < lo["fast"]),
                      "fast_is_faster": hi["fast"] < lo["strict"]}), flush=True)

    drift = {}
    for it in [int(x) for x in args.drift.split(",") if x]:
        for name, mode in MODES:
            p = plan(it, mode)
            run(p, name)
            p.close()
        drift[it] = float(((X["fast"] - X["strict"]).abs().max() / X["strict"].abs().max()).item())
        finite = bool(torch.isfinite(X["fast"]).all().item())
        print(json.dumps({"record": "drift", "iterations": it, "max_dx_over_max_x": drift[it],
                          "fast_finite": finite}), flush=True)

    t1 = {k: float(np.median(v)) for k, v in ms.items()}
    for N in [int(x) for x in args.shares.split(",") if x]:
        owner = ge.assign_aggregates(PT, L[0], N)
        by_rank = {name: [] for name, _ in MODES}
        rep_by_rank = {name: [] for name, _ in MODES}
        for r in range(N):
            mine = np.flatnonzero(owner == r).astype(np.int32)
            share = {name: plan(K, mode, aggs=mine) for name, mode in MODES}
            for name, _ in MODES:
                run(share[name], name)  # warm-up
            for name, _ in MODES:
                step, rep, _ = timed(share[name], name, K)
                by_rank[name].append(step)
                rep_by_rank[name].append(rep)
            for p in share.values():
                p.close()
        print(json.dumps({"record": "shares", "N": N, "ms_per_step_by_rank": by_rank,
                          "repulse_ms_by_rank": rep_by_rank,
                          "max_ms": {k: max(v) for k, v in by_rank.items()},
                          "efficiency": {k: t1[k] / (N * max(v)) for k, v in by_rank.items()}}),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
