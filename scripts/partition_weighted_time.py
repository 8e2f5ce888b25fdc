"""Time `ctx.partition(A, 0.125)` of this build against another libge.so (another
commit's build, loaded through GE_LIB_PATH), alternating the two in one command:

    python scripts/partition_weighted_time.py OTHER_LIBGE_SO [--cfg c3|c4]
        [--weights w3|unit] [--pairs 3] [--reps 2] [--warmup 1]
        [--other-reps R] [--other-warmup W]

One child process per measurement (a library is chosen when it is loaded), A B A
B ...; every child builds the same graph (the LCC of the seeded R-MAT, as
tests/test_gpu_configs.py does), warms up with --warmup untimed calls, times
--reps calls with a host clock (the call ends synchronised: it returns host
arrays), reports each call on stderr as it ends, with a line every minute while
one runs (a host-path call of another build takes minutes at C3: --other-reps /
--other-warmup give that build fewer calls), and prints a sha256 of the
hierarchy, which must agree across all children.
--weights w3: symmetric weights from {0.1, 0.2, 0.3} (real weights: the ordered
device path here, the host path in a build without it); unit: the R-MAT's own
integer weights (the exact device path in both).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "graph-embed_amd", "py"))

SIZES = {"c3": (1_000_000, 8_000_000), "c4": (10_000_000, 80_000_000)}
W3 = np.array([0.1, 0.2, 0.3])


def child(args):
    import ge_amd as ge
    n_ids, draws = SIZES[args.cfg]
    ctx = ge.Context(0)
    ip, ix, dx = ctx.rmat_csr(n_ids, draws, seed=12345, lcc=True)
    if args.weights == "w3":
        rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        lo, hi = np.minimum(rows, ix).astype(np.int64), np.maximum(rows, ix).astype(np.int64)
        dx = W3[(lo * 7 + hi * 13) % 3]
    A = (ip, ix, dx)
    times, dig = [], None
    done = threading.Event()

    def beat():
        t0 = time.perf_counter()
        while not done.wait(60.0):
            print(f"  ... {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)

    threading.Thread(target=beat, daemon=True).start()
    for r in range(args.reps + args.warmup):
        t0 = time.perf_counter()
        hier = ctx.partition(A, 0.125)
        dt = time.perf_counter() - t0
        print(f"  call {r}{' (warm-up)' if r < args.warmup else ''}: {dt:.3f} s", file=sys.stderr,
              flush=True)
        if r >= args.warmup:
            times.append(dt)
        h = hashlib.sha256()
        for lv in hier:
            h.update(np.ascontiguousarray(lv[0], np.int32).tobytes())
            h.update(np.ascontiguousarray(lv[1], np.int32).tobytes())
        assert dig in (None, h.hexdigest())
        dig = h.hexdigest()
    done.set()
    ctx.close()
    print(json.dumps({"n": len(ip) - 1, "nnz": len(ix), "times": times,
                      "rows": [lv[2] for lv in hier], "sha256": dig}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", nargs="?")
    ap.add_argument("--cfg", default="c3", choices=sorted(SIZES))
    ap.add_argument("--weights", default="w3", choices=["w3", "unit"])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--other-reps", type=int, default=None)
    ap.add_argument("--other-warmup", type=int, default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    assert args.other and os.path.exists(args.other), "the other build's libge.so"
    def cmd(which):
        reps, warm = args.reps, args.warmup
        if which == "other":
            reps = reps if args.other_reps is None else args.other_reps
            warm = warm if args.other_warmup is None else args.other_warmup
        return [sys.executable, os.path.abspath(__file__), "--child", "--cfg", args.cfg,
                "--weights", args.weights, "--reps", str(reps), "--warmup", str(warm)]

    res = {"this": [], "other": []}
    shas = set()
    for p in range(args.pairs):
        for which in ("other", "this"):
            env = dict(os.environ)
            env.pop("GE_LIB_PATH", None)
            if which == "other":
                env["GE_LIB_PATH"] = os.path.abspath(args.other)
            r = subprocess.run(cmd(which), env=env, stdout=subprocess.PIPE, text=True, check=True)
            out = json.loads(r.stdout.strip().splitlines()[-1])
            shas.add(out["sha256"])
            res[which] += out["times"]
            print(f"pair {p} {which}: n={out['n']} nnz={out['nnz']} rows={out['rows']} "
                  f"times {[round(t, 3) for t in out['times']]} s", flush=True)
    assert len(shas) == 1, "the two builds give different hierarchies"
    for which in ("other", "this"):
        t = np.array(res[which])
        print(f"{which}: median {np.median(t):.3f} s, min {t.min():.3f} s, max {t.max():.3f} s "
              f"over {len(t)} calls")
    print(f"other / this (medians): {np.median(res['other']) / np.median(res['this']):.2f}x; "
          f"cfg {args.cfg}, weights {args.weights}; same hierarchy sha256 {shas.pop()[:16]}")


if __name__ == "__main__":
    main()
