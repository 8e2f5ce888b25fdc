"""ge_force_atlas_batch against the loop of ge_force_atlas calls it replaces.

The graphs are sub-matrices of level-0 aggregates of the C3 hierarchy (BASELINE.json
configs[2], built as bench.py builds it: device R-MAT, LCC, device partition(A, 0.125)),
as anyToMultilevel extracts them.  K of them are drawn without replacement (seeded)
from the aggregates of at most --max-size members (default 512: the wave and block
classes; a larger graph takes ge_force_atlas's own path in both runs), so K graphs follow
the level's size histogram.  (That histogram is lopsided: of C3's 66 374 level-0 aggregates
about 98 % have one member, and a few hold thousands; --min-size 2 draws from the
aggregates that have an edge to lay out.)  For each K the batch (one ge_force_atlas_batch on the
concatenated CSR, concatenated outside the timed window) and the loop (one
Context.force_atlas per graph: the parent's code path, unchanged) run the same starts for
--iterations iterations at d = --dim, interleaved on one box in one process: one warm-up
of each, then --rounds alternations (for K above --loop-cap, where one pass of the loop
takes minutes, the loop runs once).  Host wall clock around calls that end in a
device synchronise.  The results of both are compared bit for bit once per K.

One JSON line per K: seconds of every round, the class totals, the size histogram.
  python scripts/fa_batch_vs_loop.py --out profiles/r22/fa_batch_vs_loop.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "graph-embed_amd", "py"))
import ge_amd as ge  # noqa: E402


def level_blocks(A, PT):
    """Every aggregate's internal entries as one block-diagonal CSR over P_T positions
    (1.0 per stored entry; A has no duplicate entries): (off, indptr, indices)."""
    ip, ix = np.asarray(A[0], np.int64), np.asarray(A[1], np.int64)
    pip, pix = np.asarray(PT[0], np.int64), np.asarray(PT[1], np.int64)
    n = len(ip) - 1
    vA = ge.vertex_of(PT).astype(np.int64)
    pos = np.empty(n, dtype=np.int64)
    pos[pix] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(ip))
    keep = vA[rows] == vA[ix]
    r, c = pos[rows[keep]], pos[ix[keep]]
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    bip = np.zeros(n + 1, dtype=np.int64)
    np.add.at(bip, r + 1, 1)
    return pip, np.cumsum(bip), c


def take(blocks, aggs):
    off, bip, bix = blocks
    out = []
    for a in aggs:
        r0, r1 = off[a], off[a + 1]
        e0, e1 = bip[r0], bip[r1]
        out.append(((bip[r0:r1 + 1] - e0).astype(np.int32), (bix[e0:e1] - r0).astype(np.int32),
                    np.ones(e1 - e0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=8_000_000)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--ks", default="1,16,256,4096,65536")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=4096)
    ap.add_argument("--max-size", type=int, default=512)
    ap.add_argument("--min-size", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ctx = ge.Context(0)
    L = ctx.rmat_csr(args.n, args.draws, seed=args.seed, lcc=True)
    PT = ctx.partition(L, 0.125)[0]
    blocks = level_blocks(L, PT)
    sizes = np.diff(blocks[0])
    pool = np.flatnonzero((sizes >= max(args.min_size, 1)) & (sizes <= args.max_size))
    rs = np.random.RandomState(args.seed)
    out = open(args.out, "w") if args.out else None
    for K in (int(k) for k in args.ks.split(",")):
        aggs = rs.choice(pool, size=min(K, len(pool)), replace=False)
        graphs = take(blocks, aggs)
        X0 = [rs.uniform(-1.0, 1.0, size=(len(g[0]) - 1, args.dim)) for g in graphs]
        off, ip, ix, dx = ge.concat_graphs(graphs)
        Xcat = np.ascontiguousarray(np.concatenate(X0))

        def batch():
            X = Xcat.copy()
            t0 = time.perf_counter()
            ge._force_atlas_batch_raw(ctx, off, ip, ix, dx, args.dim, X, False, None,
                                      args.iterations, {})
            return time.perf_counter() - t0, X

        def loop():
            t0 = time.perf_counter()
            res = [ctx.force_atlas(g, args.dim, coords=x, iterations=args.iterations)
                   for g, x in zip(graphs, X0)]
            return time.perf_counter() - t0, res

        _, Xb = batch()  # warm-up of both, and the comparison
        t_first, Xl = loop()
        equal = bool(np.array_equal(Xb, np.concatenate(Xl), equal_nan=True))
        tb, tl = [], []
        # above --loop-cap one pass of the loop takes minutes: its comparison pass is its one
        # reading (the smaller K before it have warmed the same kernels)
        loop_rounds = args.rounds if K <= args.loop_cap else 0
        if K > args.loop_cap:
            tl.append(t_first)
        for r in range(args.rounds):
            tb.append(batch()[0])
            if r < loop_rounds:
                tl.append(loop()[0])
        totals = (ge.ctypes.c_int * 4)()
        ge._check(ge.lib().ge_fa_batch_info(ctx.h, totals))
        hist = np.bincount(np.diff(off))
        rec = dict(K=len(graphs), min_size=args.min_size, max_size=args.max_size, dim=args.dim, iterations=args.iterations,
                   vertices=int(off[-1]), entries=int(len(ix)), batch_s=tb, loop_s=tl,
                   equal=equal, totals=dict(zip(ge.FA_BATCH_TOTALS, totals)),
                   sizes={int(s): int(c) for s, c in enumerate(hist) if c},
                   level=dict(aggregates=int(len(sizes)), pool=int(len(pool)),
                              mean_size=float(sizes.mean()), max_size=int(sizes.max())))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    ctx.close()


if __name__ == "__main__":
    main()
