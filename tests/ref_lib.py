"""Runner of oracle/_ref/ge_ref: the reference's own translation units behind
oracle/ref_driver.cpp (test infrastructure only; recipe in oracle/Makefile).

The binary exists where the reference tree was present when oracle/Makefile ran,
or where it travelled with the tree.  available() builds it when it can:
  - reference tree present, build fails  -> the error propagates (tests fail)
  - no tree, a binary is there           -> True
  - neither                              -> False (the live tests skip)
Each call runs one subcommand in a subprocess with a time limit and returns
numpy arrays.  Everything that draws random numbers runs on 1 thread (the
reference shares one generator across its `omp parallel for`).
"""
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np

import oracle_lib

REF_DIR = os.path.join(oracle_lib.ORACLE_DIR, "_ref")
REF_BIN = os.path.join(REF_DIR, "ge_ref")
REF_FLAGS_FILE = os.path.join(REF_DIR, "flags.txt")
REF_FILES = ("src/partitioner.cpp", "src/embed.cpp", "src/matrixutils.cpp",
             "include/forceatlas.hpp", "include/embed.hpp", "include/partitioner.hpp",
             "include/matrixutils.hpp")

# The reference's defaults (include/forceatlas.hpp:89-103, :314-331); the driver
# restates none, every call passes all of them.
FA_DEFAULTS = dict(ks=0.1, ksmax=1.0, repel=1.0, attract=1.0, gravity=1.0, use_weights=1,
                   linlog=0, nohubs=0, delta=1.0, tolerate=1.0, normalize=0)
ML_KEYS = ("ks", "ksmax", "use_weights", "linlog", "nohubs", "repel", "attract", "gravity",
           "delta", "tolerate")


def ref_root():
    """The reference tree oracle/Makefile compiles from (its REF variable)."""
    env = os.environ.get("REF")
    if env:
        return env
    with open(os.path.join(oracle_lib.ORACLE_DIR, "Makefile")) as f:
        return re.search(r"^REF \?= (\S+)", f.read(), re.M).group(1)


def tree_present():
    return os.path.exists(os.path.join(ref_root(), "src", "embed.cpp"))


_available = None


def available():
    global _available
    if _available is None:
        if tree_present():
            oracle_lib.build()  # raises when the reference does not compile
            if not os.path.exists(REF_BIN):
                raise RuntimeError("the reference tree is present but make built no ge_ref")
        _available = os.path.exists(REF_BIN)
    return _available


def build_info():
    """Compile flags and the sha256 of every reference file the binary was built from."""
    with open(REF_FLAGS_FILE) as f:
        flags = f.read().strip()
    files = {}
    for rel in REF_FILES:
        with open(os.path.join(ref_root(), rel), "rb") as f:
            files[rel] = hashlib.sha256(f.read()).hexdigest()
    return {"flags": flags, "reference_sha256": files}


def write_csr(path, A):
    """A = (indptr, indices, data), or (indptr, indices) for a pattern (data = 1)."""
    with open(path, "wb") as f:
        write_csr_to(f, (A[0], A[1], A[2] if len(A) > 2 else np.ones(len(A[1]))))


def write_csr_to(f, A):
    ip, ix, dx = A
    np.array([len(ip) - 1, len(ix)], np.int32).tofile(f)
    np.asarray(ip, np.int32).tofile(f)
    np.asarray(ix, np.int32).tofile(f)
    np.asarray(dx, np.float64).tofile(f)


def read_csrs(buf, count, off=0):
    out = []
    for _ in range(count):
        n, nnz = (int(v) for v in np.frombuffer(buf, np.int32, 2, off))
        off += 8
        ip = np.frombuffer(buf, np.int32, n + 1, off).copy()
        off += 4 * (n + 1)
        ix = np.frombuffer(buf, np.int32, nnz, off).copy()
        off += 4 * nnz
        dx = np.frombuffer(buf, np.float64, nnz, off).copy()
        off += 8 * nnz
        out.append((ip, ix, dx))
    assert off == len(buf), (off, len(buf))
    return out


def _run(cmd, files, scalars, seed=0, threads=1, timeout=120):
    """files: name -> writer(path), None (passed as '-') or a literal word."""
    assert available(), "oracle/_ref/ge_ref is not available"
    with tempfile.TemporaryDirectory(prefix="ge_ref_") as tmp:
        out = os.path.join(tmp, "out.bin")
        args = [REF_BIN, cmd, f"threads={threads}", f"seed={seed}", f"out={out}"]
        for name, writer in files.items():
            if writer is None or isinstance(writer, str):
                args.append(f"{name}={writer or '-'}")
            else:
                path = os.path.join(tmp, name + ".bin")
                writer(path)
                args.append(f"{name}={path}")
        # repr() round-trips a Python float through strtod
        args += [f"{k}={v!r}" if isinstance(v, float) else f"{k}={v}" for k, v in scalars.items()]
        env = dict(os.environ, OMP_NUM_THREADS=str(threads))
        r = subprocess.run(args, capture_output=True, text=True, timeout=timeout, env=env)
        assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
        with open(out, "rb") as f:
            return f.read()


def _arr(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return lambda path: a.tofile(path)


def _fa_scalars(kw, keys):
    p = dict(FA_DEFAULTS)
    bad = set(kw) - set(p)
    assert not bad, bad
    p.update(kw)
    out = {}
    for k in keys:
        out[k] = int(p[k]) if isinstance(FA_DEFAULTS[k], int) else float(p[k])
    return out


def force_atlas(A, dim, coords=None, iterations=100000, seed=0, threads=1, timeout=120, **kw):
    sc = dict(dim=dim, iterations=iterations)
    sc.update(_fa_scalars(kw, FA_DEFAULTS.keys()))
    buf = _run("fa", {"A": lambda p: write_csr(p, A),
                      "start": None if coords is None else _arr(coords, np.float64)},
               sc, seed=seed, threads=threads, timeout=timeout)
    return np.frombuffer(buf, np.float64).reshape(-1, dim).copy()


def force_atlas_ml(A, PT, vertex_A, coords_A, r_A, dim, iterations=10, seed=0, threads=1,
                   timeout=120, **kw):
    sc = dict(dim=dim, iterations=iterations)
    sc.update(_fa_scalars(kw, ML_KEYS))
    buf = _run("ml", {"A": lambda p: write_csr(p, A), "PT": lambda p: write_csr(p, PT[:2]),
                      "vA": _arr(vertex_A, np.int32), "cA": _arr(coords_A, np.float64),
                      "rA": _arr(r_A, np.float64)}, sc, seed=seed, threads=threads,
               timeout=timeout)
    return np.frombuffer(buf, np.float64).reshape(-1, dim).copy()


def _hier_from(buf):
    count = int(np.frombuffer(buf, np.int32, 1)[0])
    return [(ip, ix, len(ip) - 1, len(ix)) for ip, ix, _ in read_csrs(buf, count, 4)]


def partition(A, cf=None, num_parts=None, positive_merging=True, stall=1.0, matching=2,
              merge_leaves=False, threads=1, timeout=120):
    """cf: the hierarchy overload; num_parts: the numParts overload (one P_T);
    neither: the single-P_T overload.  Returns a list of (indptr, indices, rows, cols)."""
    if cf is not None:
        mode, value = "cf", float(cf)
    elif num_parts is not None:
        mode, value = "parts", int(num_parts)
    else:
        mode, value = "single", 0
    buf = _run("partition", {"A": lambda p: write_csr(p, A)},
               dict(mode=mode, value=value, positive_merging=int(positive_merging),
                    stall=float(stall), matching=int(matching), merge_leaves=int(merge_leaves)),
               threads=threads, timeout=timeout)
    return _hier_from(buf)


def modularity(A, PT):
    buf = _run("modularity", {"A": lambda p: write_csr(p, A), "PT": lambda p: write_csr(p, PT[:2])},
               {})
    return float(np.frombuffer(buf, np.float64)[0])


def interpolation_matrix(num_cols, sets):
    ip = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
    ix = np.concatenate([np.asarray(s, np.int32) for s in sets]) if sets else np.zeros(0, np.int32)
    buf = _run("interp", {"sets": lambda p: write_csr(p, (ip, ix))}, dict(cols=num_cols))
    return read_csrs(buf, 1)[0]


def _write_hier(As, hier):
    def w(path):
        with open(path, "wb") as f:
            np.array([len(hier)], np.int32).tofile(f)
            for A in As:
                write_csr_to(f, A)
            for PT in hier:
                write_csr_to(f, (PT[0], PT[1], np.ones(len(PT[1]))))
    return w


def embed(As, hier, dim, seed=0, threads=1, timeout=300):
    """partition::embed(As, P_Ts, d): the reference's own 100000 / 100 iterations."""
    buf = _run("embed", {"hier": _write_hier(As, hier)}, dict(dim=dim), seed=seed,
               threads=threads, timeout=timeout)
    return np.frombuffer(buf, np.float64).reshape(-1, dim).copy()


def embed_via_minimization(A, dim, coords=None, iterations=10, seed=0, timeout=300):
    """embedViaMinimization(A, d, coords, iterations); coords=None: the seeded random
    start (its empty-coords branch); coords="default": the two-argument overload
    embedViaMinimization(A, d) (zero start, its own sweep count)."""
    start = coords if coords is None or isinstance(coords, str) else _arr(coords, np.float64)
    buf = _run("minimize", {"A": lambda p: write_csr(p, A), "start": start},
               dict(dim=dim, iterations=iterations), seed=seed, timeout=timeout)
    return np.frombuffer(buf, np.float64).reshape(-1, dim).copy()


def embed_via_minimization_ml(As, hier, dim, seed=0, timeout=600):
    """embedVia(As, P_Ts, d, anyToMultilevel(embedViaMinimization))."""
    buf = _run("minimize_ml", {"hier": _write_hier(As, hier)}, dict(dim=dim), seed=seed,
               timeout=timeout)
    return np.frombuffer(buf, np.float64).reshape(-1, dim).copy()


def laplacian(A):
    """(identity(n), toLaplacian(A), fromLaplacian(toLaplacian(A))) as CSR triples."""
    return read_csrs(_run("laplacian", {"A": lambda p: write_csr(p, A)}, {}), 3)
