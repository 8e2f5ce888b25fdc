"""Generates tests/golden/faml_sched.json: the multilevel plan's schedule
(graph-embed_amd/csrc/ge_faml_sched.hpp) as the commit before the scheduler was
split out built it, case by case, as scalars plus length and sha256 of every table.

The schedule changes no result bit, so the oracle cannot see it; this file pins it
instead.  tests/test_faml_sched.py feeds each case's inputs to the host-only entry
(ge_amd.faml_schedule) and requires every scalar, length and digest to be equal.

How the tables were recorded (once, on an MI355X; neither the patch nor a library
built from it is committed): faml_plan_build of the parent commit was given a dump
that, under the scratch-only environment variable GE_SCRATCH_SCHED_DUMP=<file>,
writes every table ("T name count v0 v1 ...") and scalar ("S name value",
"D name hexfloat") it had built, with the CU count and the occupancy of
faml_sym_repulse the device reported.  Then

  GE_LIB_PATH=<that library> python tests/golden/make_faml_sched.py record DIR
  python tests/golden/make_faml_sched.py write DIR

`record` runs every case through ge_faml_plan_create* (and one iteration on an
edgeless graph; the graph does not enter the schedule) and leaves DIR/<case>.txt;
`write` turns the dumps into the json.  Changing a constant of the schedule means
recording again, deliberately.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "graph-embed_amd", "py"))

import numpy as np  # noqa: E402

K_LOOK = 16  # ge_sym.hpp kLook
# EDGE_SIZES of tests/test_gpu_sym_prio.py, then one aggregate at each edge of the
# small and mid classes
EDGE = [2600, 321, 64 * K_LOOK, 64 * K_LOOK + 1, 64 * (K_LOOK + 1) + 1, 320, 257]
A_SIZES = [[s, 1] for s in EDGE + [1, 64, 65, 256]]
CAP = {"GE_FAML_RES_CAP": "256"}
STRICT, FAST = 0, 1


def _case(name, sizes, dim=3, mode=STRICT, env=CAP, aggs=None, split=None, rank=0, nranks=1):
    return {"name": name, "sizes": sizes, "dim": dim, "mode": mode, "env": dict(env),
            "aggs": aggs, "split": split or [], "rank": rank, "nranks": nranks}


# sizes: [[members, how many aggregates], ...] in aggregate-id order
N_SIZES = [[2600, 1], [321, 1], [1, 1], [64, 1], [65, 1], [256, 1]]
O_SIZES = [[257, 1], [1025, 1]]
R4 = dict(CAP, GE_FAML_SYM="0", GE_FAML_R="4", GE_FAML_U="1")
CASES = [
    _case("a", A_SIZES),
    _case("b", [[64 * 200, 1], [64 * 10, 30]]),
    _case("c", [[2560, 400]], env={}),
    _case("d", [[64 * 300, 1], [64 * 40, 600]]),
    _case("e", [[320, 2]]),
    _case("f", A_SIZES, env=dict(CAP, GE_FAML_SYM_CHAIN="0")),
    _case("g", A_SIZES, env=dict(CAP, GE_FAML_SYM_CHAIN="1e9")),
    _case("h", A_SIZES, env=dict(CAP, GE_FAML_SYM="0")),
    _case("i", A_SIZES, env=R4),
    _case("j", A_SIZES, env=dict(CAP, GE_FAML_SYM="0", GE_FAML_R="3")),
    _case("k", A_SIZES, dim=5),
    _case("l", A_SIZES, mode=FAST),
    _case("m", A_SIZES, dim=5, mode=FAST),
    _case("n_strict", N_SIZES, aggs=[2, 3, 4, 5], split=[0, 1], rank=1, nranks=4),
    _case("n_fast", N_SIZES, mode=FAST, aggs=[2, 3, 4, 5], split=[0, 1], rank=1, nranks=4),
    _case("o", O_SIZES, aggs=[1], split=[0], rank=3, nranks=4),
    _case("p", O_SIZES, aggs=[1], split=[0], rank=0, nranks=4),
    _case("q", [[100, 1]], aggs=[]),
    _case("r", [[300, 1], [0, 1], [70, 1]]),
    # beyond the issue's table: the large-resident class (empty at a cap of 256), and a
    # split aggregate of 3 tiles over 4 ranks, of which rank 0 owns none, under R = 4
    _case("s", A_SIZES, env={"GE_FAML_RES_CAP": "1100"}),
    _case("o_r4", [[129, 1], [1025, 1]], env=R4, aggs=[1], split=[0], rank=3, nranks=4),
    _case("p_r4", [[129, 1], [1025, 1]], env=R4, aggs=[1], split=[0], rank=0, nranks=4),
]
KNOBS = ("GE_FAML_RES_CAP", "GE_FAML_R", "GE_FAML_U", "GE_FAML_SYM", "GE_FAML_SYM_CHAIN")
SCALAR_NAMES = {"census0": "small", "census1": "mid", "census2": "large", "census3": "streamed",
                "off_m": "off_mid", "off_l": "off_large", "ns": "blocks_small",
                "nm": "blocks_mid", "nl": "blocks_large", "swept": "sweeps",
                "rows_mode": "row_blocks", "xr": "xrows"}


def indptr(sizes):
    flat = [s for s, k in sizes for _ in range(k)]
    return np.concatenate([[0], np.cumsum(flat)]).astype(np.int32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def record(outdir):
    import torch

    import ge_amd as ge
    os.makedirs(outdir, exist_ok=True)
    ctx = ge.Context(0)
    dev = torch.device("cuda:0")
    for c in CASES:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(c["env"])
        os.environ["GE_SCRATCH_SCHED_DUMP"] = os.path.join(outdir, c["name"] + ".txt")
        pip = indptr(c["sizes"])
        m, n, dim = len(pip) - 1, int(pip[-1]), c["dim"]
        i32 = torch.int32
        d_ip = torch.zeros(n + 1, dtype=i32, device=dev)  # no edges
        d_ix = torch.zeros(1, dtype=i32, device=dev)
        d_dx = torch.zeros(1, dtype=torch.float64, device=dev)
        d_pip = torch.from_numpy(pip).to(dev)
        d_pix = torch.arange(n, dtype=i32, device=dev)
        d_vA = torch.from_numpy(np.repeat(np.arange(m, dtype=np.int32), np.diff(pip))).to(dev)
        d_cA = torch.zeros(m * dim, dtype=torch.float64, device=dev)
        d_rA = torch.ones(m, dtype=torch.float64, device=dev)
        d_init = torch.from_numpy(ge.uniform_stream(7, n * dim)).to(dev)
        d_x = torch.zeros(n * dim, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        comm = ge.Comm(ctx, c["nranks"], c["rank"], backend="transport") if c["nranks"] > 1 else None
        plan = ge.FamlPlan(ctx, n, d_ip.data_ptr(), d_ix.data_ptr(), d_dx.data_ptr(), pip,
                           d_pip.data_ptr(), d_pix.data_ptr(), d_vA.data_ptr(), dim, iterations=1,
                           aggs=c["aggs"], split=c["split"] or None, comm=comm, mode=c["mode"])
        try:
            if comm is None:  # a shard's run exchanges rows with ranks that do not exist here
                plan.run(d_cA.data_ptr(), d_rA.data_ptr(), d_init.data_ptr(), d_x.data_ptr())
                ctx.sync()
            print(c["name"], plan.schedule(), plan.classes(), flush=True)
        finally:
            plan.close()
            if comm is not None:
                comm.close()
    ctx.close()


def write(outdir):
    out = []
    for c in CASES:
        rec = dict(c, scalars={}, tables={})
        for line in open(os.path.join(outdir, c["name"] + ".txt")):
            kind, name, *rest = line.split()
            name = SCALAR_NAMES.get(name, name)
            if kind == "T":
                vals = np.array(rest[1:], dtype=np.int64)
                assert len(vals) == int(rest[0])
                rec["tables"][name] = {"len": len(vals), "sha256": digest(vals)}
            elif kind == "S" and name in ("cus", "sym_occ"):
                rec[name] = int(rest[0])
            elif kind == "S":
                rec["scalars"][name] = int(rest[0])
            else:
                rec[name] = float.fromhex(rest[0])
        out.append(rec)
    with open(os.path.join(HERE, "faml_sched.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_faml_sched.py", "cases": out}, f, indent=1)
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    {"record": record, "write": write}[sys.argv[1]](sys.argv[2])
