"""GE_MODE_FARFIELD against GE_MODE_FAST on a multilevel level's streamed aggregates.

Default: the C4 level (BASELINE.json configs[3], built as bench.py builds it: device
R-MAT, LCC, device partition, level 0) at d = 3, theta = 0.5.  K steps of a FAST plan
and of a FARFIELD plan are timed interleaved on one box (one warm-up, --rounds
alternations, profiling events on) with the far pass's split (prep / item kernel) and
its pair terms per row from far_info, then the drift max |dX| / max |X| of both against
STRICT after 1, 2, 10 and 100 iterations (recorded, not gated), then with --shares
N[,N..] the per-rank shares of ge_assign_aggregates, each a subset plan, in both modes.
--far-min sets GE_FAR_MIN_ML for the FARFIELD plans (default 257: every streamed
aggregate), --items the rows of a far item (64 or 256).

--crossover: synthetic levels of equal aggregates of 2^12 .. 2^16 members (a ring each,
about --rows members in all, GE_FAML_RES_CAP=256 so that all are streamed), FAST against
FARFIELD with 64- and 256-row items, interleaved.  The plan's default far_min_ml is the
smallest swept size from which FARFIELD's range lies wholly below FAST's (never below
4096), and the default item the one that wins there.

One JSON line per record.
  python scripts/faml_far_vs_fast.py --steps 5 --rounds 3 --shares 4,8
  python scripts/faml_far_vs_fast.py --crossover --steps 3 --rounds 3
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


class Level:
    """A level on the device and plans over it."""

    def __init__(self, ctx, A, PT, dim, seed):
        self.ctx, self.PT, self.dim = ctx, PT, dim
        self.n, self.m = len(A[0]) - 1, len(PT[0]) - 1
        dev = torch.device("cuda:0")
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        cA = ge.uniform_stream(seed + 1, self.m * dim).reshape(self.m, dim)
        rA = 0.01 + 0.19 * (ge.uniform_stream(seed + 2, self.m) + 1.0) / 2.0
        self.d = dict(ip=T(A[0]), ix=T(A[1]), dx=T(A[2]), pip=T(PT[0]), pix=T(PT[1]),
                      vA=T(ge.vertex_of(PT)), cA=T(cA), rA=T(rA),
                      init=T(ge.uniform_stream(seed, self.n * dim)))
        self.X = {}
        torch.cuda.synchronize(dev)

    def plan(self, iters, mode, aggs=None, env=None, **kw):
        d = self.d
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            return ge.FamlPlan(self.ctx, self.n, d["ip"].data_ptr(), d["ix"].data_ptr(),
                               d["dx"].data_ptr(), self.PT[0], d["pip"].data_ptr(),
                               d["pix"].data_ptr(), d["vA"].data_ptr(), self.dim, iterations=iters,
                               aggs=aggs, mode=mode, **kw)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v

    def run(self, p, name):
        if name not in self.X:
            self.X[name] = torch.zeros((self.n, self.dim), dtype=torch.float64, device="cuda:0")
        d = self.d
        p.run(d["cA"].data_ptr(), d["rA"].data_ptr(), d["init"].data_ptr(), self.X[name].data_ptr())
        self.ctx.sync()

    def timed(self, p, name, iters):
        p.set_profiling(True)  # restarts the plan's event counters
        t0 = time.perf_counter()
        self.run(p, name)
        ms = (time.perf_counter() - t0) / iters * 1e3
        rec = {"ms_per_step": ms, "repulse_ms": p.repulse_ms()[0], "rows_ms": p.rows_ms()[0]}
        if p.mode()[0] == ge.MODE_FARFIELD:
            fi = p.far_info()
            rec.update(prep_ms=fi["prep_ms"], item_ms=fi["item_ms"],
                       terms_per_row=fi["pair_terms"] / max(fi["rows"], 1),
                       accepted=fi["accepted"], exact_leaves=fi["exact_leaves"])
        return rec


def interleave(lv, plans, K, rounds, tag):
    """One warm-up of every plan, then `rounds` alternations; returns {name: [ms per step]}."""
    for name, p in plans.items():
        lv.run(p, name)
    ms = {name: [] for name in plans}
    for rnd in range(rounds):
        for name, p in plans.items():
            rec = lv.timed(p, name, K)
            ms[name].append(rec["ms_per_step"])
            print(json.dumps(dict(record="round", round=rnd, mode=name, steps=K, **tag, **rec)),
                  flush=True)
    return ms


def c4(args):
    ctx = ge.Context(0)
    L = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=True)
    PT = ctx.partition(L, 0.125)[0]
    lv = Level(ctx, L, PT, args.dim, args.seed)
    far_env = {"GE_FAR_MIN_ML": str(args.far_min), "GE_FAR_R": "4" if args.items == 256 else "1"}
    K = args.steps
    mk = {"fast": lambda it, aggs=None: lv.plan(it, ge.MODE_FAST, aggs),
          "far": lambda it, aggs=None: lv.plan(it, ge.MODE_FARFIELD, aggs, env=far_env,
                                               theta=args.theta),
          "strict": lambda it, aggs=None: lv.plan(it, ge.MODE_STRICT, aggs)}
    plans = {k: mk[k](K) for k in ("fast", "far")}
    fi, cls = plans["far"].far_info(), plans["far"].classes()
    sizes = np.diff(PT[0])
    print(json.dumps({"record": "level", "n": lv.n, "nnz": len(L[1]), "aggregates": lv.m,
                      "dim": args.dim, "theta": args.theta, "streamed": cls["streamed"],
                      "res_cap": cls["res_cap"], "far_mode": plans["far"].mode(),
                      "fast_mode": plans["fast"].mode(), "far_aggregates": len(fi["aggregates"]),
                      "far_rows": fi["rows"], "far_min_ml": fi["far_min_ml"],
                      "item_rows": fi["item_rows"], "key_bits": fi["key_bits"],
                      "far_sizes_min_max": [int(sizes[fi["aggregates"]].min()),
                                            int(sizes[fi["aggregates"]].max())]
                      if fi["aggregates"] else None,
                      "pairs_per_launch": plans["fast"].repulse_ms()[2]}), flush=True)
    ms = interleave(lv, plans, K, args.rounds, {})
    for p in plans.values():
        p.close()
    lo = {k: min(v) for k, v in ms.items()}
    hi = {k: max(v) for k, v in ms.items()}
    print(json.dumps({"record": "summary", "N": 1, "fast_ms_range": [lo["fast"], hi["fast"]],
                      "far_ms_range": [lo["far"], hi["far"]],
                      "ratio_fast_over_far": float(np.median(ms["fast"]) / np.median(ms["far"])),
                      "far_is_faster": hi["far"] < lo["fast"]}), flush=True)
    for it in [int(x) for x in args.drift.split(",") if x]:
        for name in ("strict", "fast", "far"):
            p = mk[name](it)
            lv.run(p, name)
            p.close()
        ref = lv.X["strict"]
        print(json.dumps({"record": "drift", "iterations": it,
                          **{name + "_vs_strict": float(((lv.X[name] - ref).abs().max()
                                                         / ref.abs().max()).item())
                             for name in ("fast", "far")},
                          "far_finite": bool(torch.isfinite(lv.X["far"]).all().item())}), flush=True)
    t1 = {k: float(np.median(v)) for k, v in ms.items()}
    for N in [int(x) for x in args.shares.split(",") if x]:
        owner = ge.assign_aggregates(PT, L[0], N)
        by_rank = {"fast": [], "far": []}
        for r in range(N):
            mine = np.flatnonzero(owner == r).astype(np.int32)
            share = {k: mk[k](K, mine) for k in ("fast", "far")}
            for name, p in share.items():
                lv.run(p, name)  # warm-up
            for name, p in share.items():
                by_rank[name].append(lv.timed(p, name, K)["ms_per_step"])
            for p in share.values():
                p.close()
        print(json.dumps({"record": "shares", "N": N, "ms_per_step_by_rank": by_rank,
                          "max_ms": {k: max(v) for k, v in by_rank.items()},
                          "efficiency": {k: t1[k] / (N * max(v)) for k, v in by_rank.items()}}),
              flush=True)
    ctx.close()


def crossover(args):
    os.environ["GE_FAML_RES_CAP"] = "256"
    ctx = ge.Context(0)
    K = args.steps
    for e in range(12, 17):
        s = 1 << e
        m = max(1, args.rows // s)
        n = m * s
        i = np.arange(n, dtype=np.int64)
        nxt = (i // s) * s + (i % s + 1) % s  # a ring inside every aggregate
        prv = (i // s) * s + (i % s - 1) % s
        ix = np.sort(np.stack([prv, nxt], axis=1), axis=1).reshape(-1).astype(np.int32)
        A = (np.arange(0, 2 * n + 1, 2, dtype=np.int32), ix, np.ones(2 * n))
        PT = (np.arange(0, n + 1, s, dtype=np.int32), np.arange(n, dtype=np.int32), m)
        lv = Level(ctx, A, PT, args.dim, args.seed)
        plans = {"fast": lv.plan(K, ge.MODE_FAST)}
        for rows in (64, 256):
            plans[f"far{rows}"] = lv.plan(K, ge.MODE_FARFIELD, theta=args.theta,
                                          env={"GE_FAR_MIN_ML": "257",
                                               "GE_FAR_R": "4" if rows == 256 else "1"})
            assert plans[f"far{rows}"].far_info()["item_rows"] == rows
        ms = interleave(lv, plans, K, args.rounds, {"members": s, "aggregates": m})
        for p in plans.values():
            p.close()
        print(json.dumps({"record": "crossover", "members": s, "aggregates": m, "rows": n,
                          "dim": args.dim, "theta": args.theta,
                          **{k + "_ms_range": [min(v), max(v)] for k, v in ms.items()},
                          **{k + "_is_faster": max(ms[k]) < min(ms["fast"])
                             for k in ("far64", "far256")}}), flush=True)
        del lv
        torch.cuda.empty_cache()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--draws", type=int, default=80_000_000)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--drift", default="1,2,10,100")
    ap.add_argument("--shares", default="")
    ap.add_argument("--far-min", type=int, default=257)
    ap.add_argument("--items", type=int, default=64, choices=(64, 256))
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--rows", type=int, default=1 << 22)
    args = ap.parse_args()
    assert args.rounds >= 3, "at least 3 alternations"
    (crossover if args.crossover else c4)(args)


if __name__ == "__main__":
    main()
