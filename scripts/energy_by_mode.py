"""What STRICT, FAST and FARFIELD reach, measured with the layout energy (include/ge.h,
"layout energy"; FaPlan.energy, Context.layout_energy).

  single   the level-0 graph of bench.py --workload c3 (the LCC of the 1M-id R-MAT; --graph c2
           takes the whole R-MAT of --workload c2), d = 3: a plan per mode stepped from the same
           seeded start, E, its three parts and the relative edge length lambda after 0, 1,
           2, 10 and 100 iterations.  FARFIELD runs with theta = 0.5; when the level is below
           the plan's far_min the script lowers GE_FAR_MIN to 0 and says so in the record.
  embed    one full embed per mode over the C3 hierarchy (device partition(A, 0.125), P^T A P
           per level), and the single-level energy of its output on the level-0 graph.
  time     the energy pass against FaPlan.repulse of a FAST plan of the same build on the
           c2 graph, interleaved (one warm-up each, then --rounds >= 3 alternations of
           --reps passes, wall time around a synchronised block).

One JSON line per record, appended to --out:
  python scripts/energy_by_mode.py single embed time --out profiles/r20/energy_by_mode.jsonl
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

MODES = (("strict", ge.MODE_STRICT), ("fast", ge.MODE_FAST), ("farfield", ge.MODE_FARFIELD))
OUT = None


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def summary(tot, n, nnz):
    return dict(E=float(tot[ge.ENERGY_REP] + tot[ge.ENERGY_ATT] + tot[ge.ENERGY_GRAV]),
                rep=float(tot[ge.ENERGY_REP]), att=float(tot[ge.ENERGY_ATT]),
                grav=float(tot[ge.ENERGY_GRAV]),
                rel_edge_length=float(ge.relative_edge_length(tot, n, nnz)))


def graph(ctx, args, which):
    A = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=which == "c3")
    return A, len(A[0]) - 1, len(A[1])


def single(ctx, dev, args):
    A, n, nnz = graph(ctx, args, args.graph)
    dim = 3
    X0 = ge.uniform_stream(args.seed, n * dim).reshape(n, dim)
    t = [torch.from_numpy(a).to(dev) for a in A]
    marks = sorted(int(k) for k in args.iterations.split(","))
    for name, mode in MODES:
        lowered = False
        if mode == ge.MODE_FARFIELD:
            probe = ctx.fa_plan(n, nnz, *(v.data_ptr() for v in t), dim, 0, n, mode=mode, theta=0.5)
            lowered = probe.far_info()["reason"] == "small"
            probe.close()
            if lowered:
                os.environ["GE_FAR_MIN"] = "0"
        plan = ctx.fa_plan(n, nnz, *(v.data_ptr() for v in t), dim, 0, n, mode=mode, theta=0.5)
        info = plan.far_info()
        a = torch.from_numpy(X0).to(dev)
        b = torch.zeros_like(a)
        it = 0
        t0 = time.perf_counter()
        for mark in marks:
            while it < mark:
                plan.step(a.data_ptr(), b.data_ptr())
                a, b = b, a
                it += 1
            ctx.sync()
            tot = plan.energy(a.data_ptr())
            emit(record="single", graph=args.graph, n=n, nnz=nnz, dim=dim, mode=name,
                 iterations=it, far_active=info["active"], far_min_lowered=lowered,
                 seconds=time.perf_counter() - t0, finite=bool(np.isfinite(tot).all()),
                 **summary(tot, n, nnz))
        plan.close()
        os.environ.pop("GE_FAR_MIN", None)


def embed(ctx, dev, args):
    A, n, nnz = graph(ctx, args, "c3")
    hier = ctx.partition(A, 0.125)[:args.levels]
    As = [A]
    for PT in hier:
        As.append(ctx.ptap(As[-1], PT))
    for name, mode in MODES:
        t0 = time.perf_counter()
        X = ctx.embed(As, hier, 3, seed=args.seed, mode=mode, theta=0.5)
        secs = time.perf_counter() - t0
        _, tot = ctx.layout_energy(A, X, rows=False)
        emit(record="embed", n=n, nnz=nnz, dim=3, levels=[h[2] for h in hier], mode=name,
             embed_seconds=secs, finite=bool(np.isfinite(X).all()), **summary(tot, n, nnz))


def timing(ctx, dev, args):
    assert args.rounds >= 3, "at least 3 alternations"
    A, n, nnz = graph(ctx, args, "c2")
    dim = 3
    x = torch.from_numpy(ge.uniform_stream(args.seed, n * dim).reshape(n, dim)).to(dev)
    out = torch.zeros((n, dim), dtype=torch.float64, device=dev)
    t = [torch.from_numpy(a).to(dev) for a in A]
    plan = ctx.fa_plan(n, nnz, *(v.data_ptr() for v in t), dim, 0, n, mode=ge.MODE_FAST)
    passes = {"energy": lambda: plan.energy(x.data_ptr()),
              "fast_repulse": lambda: plan.repulse(x.data_ptr(), out.data_ptr())}
    for f in passes.values():
        f()
    ms = {k: [] for k in passes}
    for rnd in range(args.rounds):
        for name, f in passes.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                f()  # both synchronise
            ms[name].append((time.perf_counter() - t0) / args.reps * 1e3)
            emit(record="time_round", round=rnd, what=name, n=n, dim=dim, reps=args.reps,
                 ms_per_pass=ms[name][-1])
    emit(record="time_summary", n=n, dim=dim,
         energy_ms_range=[min(ms["energy"]), max(ms["energy"])],
         fast_repulse_ms_range=[min(ms["fast_repulse"]), max(ms["fast_repulse"])],
         energy_over_repulse=float(np.median(ms["energy"]) / np.median(ms["fast_repulse"])),
         energy_wholly_below_repulse=max(ms["energy"]) < min(ms["fast_repulse"]))
    plan.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="+", choices=["single", "embed", "time"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=8_000_000)
    ap.add_argument("--graph", choices=["c2", "c3"], default="c3")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--iterations", default="0,1,2,10,100")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    OUT = args.out
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    ctx = ge.Context(0)
    dev = torch.device("cuda:0")
    for part in args.parts:
        {"single": single, "embed": embed, "time": timing}[part](ctx, dev, args)
    ctx.close()


if __name__ == "__main__":
    main()
