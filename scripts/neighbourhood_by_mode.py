"""What STRICT, FAST and FARFIELD keep of each vertex's own neighbourhood, measured with the
neighbourhood precision (include/ge.h, "layout neighbours"; Context.layout_neighbourhood).

  single   the level-0 graph of bench.py --workload c3 (the LCC of the 1M-id R-MAT), d = 3: a
           plan per mode stepped from the same seeded start for --iterations steps, then the
           precision of a seeded sample of --rows query rows at kmax = --kmax.  FARFIELD runs
           with theta = 0.5; when the level is below the plan's far_min the script lowers
           GE_FAR_MIN to 0 and says so in the record.  A record for the start itself (a
           random layout: about k / (n - 1)) comes first.
  embed    one full embed per mode over the C3 hierarchy (device partition(A, 0.125), P^T A P
           per level), and the precision of its output on the level-0 graph, same sample.

One JSON line per record, appended to --out:
  python scripts/neighbourhood_by_mode.py single embed --out profiles/r23/neighbourhood_by_mode.jsonl
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


def precision(ctx, A, X, rows, kmax):
    t0 = time.perf_counter()
    per, tot = ctx.layout_neighbourhood(A, X, kmax=kmax, rows=rows)
    secs = time.perf_counter() - t0
    mean, pooled = ge.neighbourhood_precision(per)
    info = ctx.knn_info()
    return dict(precision_mean=mean, precision_pooled=pooled, rows_with_neighbours=int(tot[ge.NBHD_ROWS]),
                sum_k=int(tot[ge.NBHD_K]), hits=int(tot[ge.NBHD_HITS]), kmax=kmax,
                sample_rows=len(rows), knn_seconds=secs, knn_jsplit=info["jsplit"],
                knn_rows_per_wg=info["rows_per_wg"], knn_insertions=info["insertions"])


def graph(ctx, args):
    A = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=True)
    n = len(A[0]) - 1
    rows = np.sort(np.random.RandomState(args.seed).choice(n, size=min(args.rows, n), replace=False))
    return A, n, len(A[1]), rows.astype(np.int32)


def single(ctx, dev, args):
    A, n, nnz, rows = graph(ctx, args)
    dim = 3
    X0 = ge.uniform_stream(args.seed, n * dim).reshape(n, dim)
    emit(record="start", n=n, nnz=nnz, dim=dim, random_layout_expectation=args.kmax / (n - 1.0),
         **precision(ctx, A, X0, rows, args.kmax))
    t = [torch.from_numpy(a).to(dev) for a in A]
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
        t0 = time.perf_counter()
        for _ in range(args.iterations):
            plan.step(a.data_ptr(), b.data_ptr())
            a, b = b, a
        ctx.sync()
        secs = time.perf_counter() - t0
        X = a.cpu().numpy()
        plan.close()
        os.environ.pop("GE_FAR_MIN", None)
        emit(record="single", n=n, nnz=nnz, dim=dim, mode=name, iterations=args.iterations,
             far_active=info["active"], far_min_lowered=lowered, seconds=secs,
             finite=bool(np.isfinite(X).all()), **precision(ctx, A, X, rows, args.kmax))


def embed(ctx, dev, args):
    A, n, nnz, rows = graph(ctx, args)
    hier = ctx.partition(A, 0.125)[:args.levels]
    As = [A]
    for PT in hier:
        As.append(ctx.ptap(As[-1], PT))
    for name, mode in MODES:
        t0 = time.perf_counter()
        X = ctx.embed(As, hier, 3, seed=args.seed, mode=mode, theta=0.5)
        secs = time.perf_counter() - t0
        emit(record="embed", n=n, nnz=nnz, dim=3, levels=[h[2] for h in hier], mode=name,
             embed_seconds=secs, finite=bool(np.isfinite(X).all()),
             **precision(ctx, A, X, rows, args.kmax))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="+", choices=["single", "embed"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=8_000_000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--kmax", type=int, default=16)
    args = ap.parse_args()
    OUT = args.out
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    ctx = ge.Context(0)
    dev = torch.device("cuda:0")
    for part in args.parts:
        {"single": single, "embed": embed}[part](ctx, dev, args)
    ctx.close()


if __name__ == "__main__":
    main()
