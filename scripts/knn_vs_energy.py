"""One exact k-nearest-neighbour pass (all rows, k = 16, d = 3; ge_layout_knn_device) against
FaPlan.energy of the same build on the graph of bench.py --workload c2, interleaved: one
warm-up each, then --rounds >= 3 alternations of --reps passes, wall time around a
synchronised block.  Per pair the kNN pass does the d subtractions, the d multiply / fma and
one compare; the energy pass does those plus the rsq, two Newton steps, an fma and an add.
What the kNN pass takes beyond the energy's time is its select path; the record carries
ge_knn_info's insertion count to size it.  Neither time is a gate.

One JSON line per record, appended to --out:
  python scripts/knn_vs_energy.py --out profiles/r23/knn_vs_energy.jsonl
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=8_000_000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    assert args.rounds >= 3, "at least 3 alternations"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    ctx = ge.Context(0)
    dev = torch.device("cuda:0")
    A = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=False)
    n, nnz, dim, k = len(A[0]) - 1, len(A[1]), 3, args.k
    x = torch.from_numpy(ge.uniform_stream(args.seed, n * dim).reshape(n, dim)).to(dev)
    idx = torch.zeros((n, k), dtype=torch.int32, device=dev)
    t = [torch.from_numpy(a).to(dev) for a in A]
    plan = ctx.fa_plan(n, nnz, *(v.data_ptr() for v in t), dim, 0, n, mode=ge.MODE_FAST)
    torch.cuda.synchronize(dev)

    def knn():
        ctx.layout_knn_device(n, dim, x.data_ptr(), k, n, None, idx.data_ptr())
        ctx.sync()

    passes = {"knn": knn, "energy": lambda: plan.energy(x.data_ptr())}
    for f in passes.values():
        f()
    info = ctx.knn_info()
    ms = {name: [] for name in passes}
    for rnd in range(args.rounds):
        for name, f in passes.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                f()  # both synchronise
            ms[name].append((time.perf_counter() - t0) / args.reps * 1e3)
            emit(record="time_round", round=rnd, what=name, n=n, dim=dim, k=k, reps=args.reps,
                 ms_per_pass=ms[name][-1])
    emit(record="time_summary", n=n, dim=dim, k=k, knn_ms_range=[min(ms["knn"]), max(ms["knn"])],
         energy_ms_range=[min(ms["energy"]), max(ms["energy"])],
         knn_over_energy=float(np.median(ms["knn"]) / np.median(ms["energy"])),
         knn_rows_per_wg=info["rows_per_wg"], knn_jsplit=info["jsplit"],
         knn_insertions=info["insertions"], insertions_per_row=info["insertions"] / n,
         expected_insertions_per_row=k * (1 + float(np.log(n / k))))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
