"""ctypes binding of libge.so (include/ge.h) -- the host-side mirror of
graph-embed's partition:: API for Python callers, tests and the benchmark.

The library is the product: every call below runs the gfx950 HIP kernels (or,
for the host-resident steps, the library's own C++).  There is no CPU fallback:
if libge.so is missing or no device is visible, the device entry points raise.

Reference interfaces mirrored (LLNL/graph-embed):
  force_atlas        partition::forceAtlas          include/forceatlas.hpp:89-312
  force_atlas_ml     partition::forceAtlasMultilevel include/forceatlas.hpp:314-574
  partition          partition::partition (hierarchy) src/partitioner.cpp:1550-1893
  interpolation_matrix                               src/partitioner.cpp:29-65
  ptap               P_T.Mult(A).Mult(P_T.Transpose()) examples/embed.cpp:96-98
  embed              partition::embed                src/embed.cpp:561-796
  modularity         partition::modularity           src/partitioner.cpp:69-114
  embed_via_minimization_ml  anyToMultilevel(embedViaMinimization), one level
                                                     src/embed.cpp:23-83, :341-559
"""
import ctypes
import os
import subprocess

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPO_ROOT = os.path.dirname(PKG_ROOT)
# GE_LIB_PATH: a variant build of the same library (kernel tuning scripts only)
LIB_PATH = os.environ.get("GE_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libge.so")
HEADER = os.path.join(REPO_ROOT, "include", "ge.h")

MODE_STRICT = 0
MODE_FAST = 1
MODE_FARFIELD = 2
FAR_MAX_LEVELS = 8  # GE_FAR_MAX_LEVELS
# the columns of the layout energy (GE_ENERGY_*, include/ge.h)
ENERGY_COLS = 5
ENERGY_REP, ENERGY_ATT, ENERGY_GRAV, ENERGY_PAIRDIST, ENERGY_EDGELEN = range(ENERGY_COLS)
# layout neighbours (include/ge.h): GE_KNN_MAX_K, the totals of the neighbourhood
# precision (GE_NBHD_*) and ge_knn_info's codes (GE_KNN_PATH_*, GE_KNN_FORM_*)
KNN_MAX_K = 64
NBHD_TOTALS = 3
NBHD_ROWS, NBHD_K, NBHD_HITS = range(NBHD_TOTALS)
KNN_PATHS = ("none", "host", "device")
KNN_FORMS = ("narrow", "wide")
# ge_fa_plan_far_info reason codes (GE_FAR_*)
FAR_REASONS = ("active", "not_requested", "dim", "row_shard", "mass", "small")
# GE_ROW_*: how the last row pass finished a heavy row (FaPlan.rows_info)
ROW_NONE, ROW_BINADE, ROW_SERIAL_FLAG, ROW_SERIAL_BASE, ROW_SERIAL_RANGE, ROW_SERIAL_WHOLE = (
    0, 1, 2, 4, 8, 16)
MATH_OPS = {"sqrt": 0, "div": 1, "pair": 2, "rep": 3}  # GE_MATH_*

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_vp = ctypes.c_void_p
_ip = ctypes.POINTER(ctypes.c_int)


class GeError(RuntimeError):
    pass


class FaParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in
                ("ks", "ksmax", "repel", "attract", "gravity", "delta", "tolerate")] + \
               [(k, ctypes.c_int) for k in ("use_weights", "linlog", "nohubs", "normalize")] + \
               [("seed", ctypes.c_uint), ("mode", ctypes.c_int), ("theta", ctypes.c_double)]


_SIGS = {
    "ge_fa_params_default": (None, [ctypes.POINTER(FaParams)]),
    "ge_last_error": (ctypes.c_char_p, []),
    "ge_version": (ctypes.c_char_p, []),
    "ge_device_count": (ctypes.c_int, [_ip]),
    "ge_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_ctx_destroy": (ctypes.c_int, [_vp]),
    "ge_ctx_set_stream": (ctypes.c_int, [_vp, _vp]),
    "ge_ctx_sync": (ctypes.c_int, [_vp]),
    "ge_force_atlas": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int,
                                      _f64p, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(FaParams)]),
    "ge_fa_plan_create": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                         ctypes.c_int, ctypes.POINTER(FaParams), ctypes.c_int,
                                         ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_fa_plan_step": (ctypes.c_int, [_vp, _vp, _vp]),
    "ge_fa_plan_attract": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "ge_fa_plan_repulse": (ctypes.c_int, [_vp, _vp, _vp]),
    "ge_fa_plan_forces": (ctypes.c_int, [_vp, _vp]),
    "ge_fa_plan_energy": (ctypes.c_int, [_vp, _vp, _vp, _f64p]),
    "ge_layout_energy": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int,
                                        _f64p, ctypes.POINTER(FaParams), _vp, _f64p]),
    "ge_layout_knn": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _f64p, ctypes.c_int,
                                     ctypes.c_int, _vp, _vp, _vp]),
    "ge_layout_knn_device": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                            ctypes.c_int, _vp, _vp, _vp]),
    "ge_layout_neighbourhood": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, ctypes.c_int,
                                               _f64p, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                               ctypes.POINTER(ctypes.c_longlong)]),
    "ge_knn_info": (ctypes.c_int, [_vp, _ip, _ip, _ip, _ip, ctypes.POINTER(ctypes.c_longlong)]),
    "ge_fa_plan_rows_info": (ctypes.c_int, [_vp, _ip, _vp, _vp]),
    "ge_fa_plan_far_info": (ctypes.c_int, [_vp, _ip, _ip, ctypes.POINTER(ctypes.c_double), _ip, _ip,
                                           _ip, ctypes.POINTER(ctypes.c_longlong), _ip,
                                           ctypes.POINTER(ctypes.c_longlong),
                                           ctypes.POINTER(ctypes.c_longlong),
                                           ctypes.POINTER(ctypes.c_longlong),
                                           ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double)]),
    "ge_fa_plan_far_layout": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ge_fa_plan_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "ge_fa_plan_kernel_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), _ip]),
    "ge_fa_sched_query": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(FaParams), ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, _ip]),
    "ge_fa_plan_schedule": (ctypes.c_int, [_vp, _ip]),
    "ge_force_atlas_batch": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _i32p, _f64p,
                                            ctypes.c_int, _f64p, ctypes.c_int, _vp, ctypes.c_int,
                                            ctypes.POINTER(FaParams)]),
    "ge_fa_batch_sched_query": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, ctypes.c_int,
                                               ctypes.POINTER(FaParams), _i32p, _i32p, _ip]),
    "ge_fa_batch_info": (ctypes.c_int, [_vp, _ip]),
    "ge_embed_via_force_atlas_ml": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, ctypes.c_int,
                                                   _i32p, _i32p, _i32p, _f64p, _f64p,
                                                   ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(FaParams), _f64p, _ip]),
    "ge_fa_plan_destroy": (ctypes.c_int, [_vp]),
    "ge_force_atlas_ml": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int,
                                         _i32p, _i32p, _i32p, _f64p, _f64p, _f64p, ctypes.c_int,
                                         ctypes.c_int, ctypes.POINTER(FaParams)]),
    "ge_partition": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_double,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                    ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_partition_single": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                           ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_hier_info": (ctypes.c_int, [_vp, _ip, _ip, ctypes.POINTER(ctypes.c_longlong)]),
    "ge_hier_census": (ctypes.c_int, [_vp, _vp]),
    "ge_hier_final_graph": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "ge_hier_final_alpha": (ctypes.c_int, [_vp, _f64p]),
    "ge_hier_levels": (ctypes.c_int, [_vp, _ip]),
    "ge_hier_shape": (ctypes.c_int, [_vp, ctypes.c_int, _ip, _ip]),
    "ge_hier_copy": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p]),
    "ge_hier_free": (ctypes.c_int, [_vp]),
    "ge_interpolation_matrix": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i32p, _i32p,
                                               ctypes.POINTER(_vp)]),
    "ge_ptap": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int, _i32p,
                               _i32p, ctypes.POINTER(_vp)]),
    "ge_ptap_rows": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int, _i32p,
                                    _i32p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_ptap_info": (ctypes.c_int, [_vp, _ip, _ip, _ip, _ip, ctypes.POINTER(ctypes.c_longlong),
                                    ctypes.POINTER(ctypes.c_longlong)]),
    "ge_graph_info": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_longlong), _ip, _ip, _ip]),
    "ge_radius_info": (ctypes.c_int, [_vp, _ip, _ip]),
    "ge_csr_shape": (ctypes.c_int, [_vp, _ip, _ip, ctypes.POINTER(ctypes.c_longlong)]),
    "ge_csr_copy": (ctypes.c_int, [_vp, _i32p, _vp, _vp]),
    "ge_csr_free": (ctypes.c_int, [_vp]),
    "ge_modularity_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _vp,
                                            ctypes.POINTER(ctypes.c_double)]),
    "ge_modularity": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int, _i32p,
                                     ctypes.POINTER(ctypes.c_double)]),
    "ge_embed": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _f64p,
                                _i32p, _i32p, _i32p, _i32p, _i32p, ctypes.c_int, ctypes.c_int,
                                ctypes.c_int, ctypes.c_int, ctypes.POINTER(FaParams), _f64p]),
    "ge_radius_step": (ctypes.c_int, [ctypes.c_int, _f64p, _f64p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ge_uniform_stream": (ctypes.c_int, [ctypes.c_uint, ctypes.c_longlong, _f64p]),
    "ge_faml_plan_create": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _i32p,
                                           _vp, _vp, _vp, ctypes.c_int, ctypes.POINTER(FaParams),
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(_vp)]),
    "ge_faml_plan_create_subset": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int,
                                                  _i32p, _vp, _vp, _vp, ctypes.c_int,
                                                  ctypes.POINTER(FaParams), ctypes.c_int, _i32p,
                                                  ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_faml_plan_create_shard": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp,
                                                 ctypes.c_int, _i32p, _vp, _vp, _vp, ctypes.c_int,
                                                 ctypes.POINTER(FaParams), ctypes.c_int, _i32p,
                                                 ctypes.c_int, _i32p, ctypes.c_int,
                                                 ctypes.POINTER(_vp)]),
    "ge_faml_plan_run": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "ge_faml_plan_mode": (ctypes.c_int, [_vp, _ip, _ip]),
    "ge_faml_plan_repulse": (ctypes.c_int, [_vp, _vp, _vp]),
    "ge_faml_plan_far_info": (ctypes.c_int, [_vp, _ip, _ip, ctypes.POINTER(ctypes.c_double), _ip,
                                             _ip, _ip, _ip, ctypes.POINTER(ctypes.c_longlong), _ip,
                                             ctypes.POINTER(ctypes.c_longlong),
                                             ctypes.POINTER(ctypes.c_longlong),
                                             ctypes.POINTER(ctypes.c_longlong),
                                             ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double)]),
    "ge_faml_plan_far_aggregates": (ctypes.c_int, [_vp, _vp]),
    "ge_faml_plan_far_shape": (ctypes.c_int, [_vp, ctypes.c_int, _ip, _ip, _ip, _ip]),
    "ge_faml_plan_far_layout": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "ge_faml_plan_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "ge_faml_plan_kernel_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double), _ip]),
    "ge_faml_plan_repulse_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), _ip,
                                               ctypes.POINTER(ctypes.c_double)]),
    "ge_faml_plan_schedule": (ctypes.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "ge_faml_plan_classes": (ctypes.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "ge_faml_plan_rows_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), _ip,
                                            ctypes.POINTER(ctypes.c_longlong),
                                            ctypes.POINTER(ctypes.c_longlong)]),
    "ge_faml_plan_destroy": (ctypes.c_int, [_vp]),
    "ge_faml_sched_create": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, ctypes.c_int, _i32p,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_faml_sched_table": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_ip),
                                           ctypes.POINTER(ctypes.c_longlong)]),
    "ge_faml_sched_pairs": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "ge_faml_sched_destroy": (ctypes.c_int, [_vp]),
    "ge_selftest_math": (ctypes.c_int, [_vp, ctypes.c_longlong, ctypes.c_ulonglong,
                                        ctypes.POINTER(ctypes.c_longlong)]),
    "ge_math_cases": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, _f64p,
                                     np.ctypeslib.ndpointer(dtype=np.uint64,
                                                            flags="C_CONTIGUOUS")]),
    "ge_rmat_csr": (ctypes.c_int, [ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong,
                                   ctypes.POINTER(_vp)]),
    "ge_largest_component": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, _f64p,
                                            ctypes.POINTER(_vp)]),
    "ge_radius_step_device": (ctypes.c_int, [_vp, ctypes.c_int, _f64p, _f64p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp,
                                             _vp, _ip]),
    "ge_embed_via_minimization": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, ctypes.c_int, _f64p,
                                                 ctypes.c_int, ctypes.c_uint, ctypes.c_int]),
    "ge_embed_via_minimization_ml": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, ctypes.c_int,
                                                    _i32p, _i32p, _i32p, _f64p, _f64p,
                                                    ctypes.c_int, ctypes.c_int, _f64p, _ip]),
    "ge_rmat_csr_device": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong,
                                          ctypes.c_int, ctypes.POINTER(_vp)]),
    "ge_largest_component_device": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p,
                                                   ctypes.POINTER(_vp)]),
    # multi-GPU (ge_dist.hip)
    "ge_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "ge_comm_create": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                      ctypes.POINTER(_vp)]),
    "ge_comm_create_transport": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp,
                                                ctypes.POINTER(_vp)]),
    "ge_comm_info": (ctypes.c_int, [_vp, _ip, _ip, _ip]),
    "ge_comm_destroy": (ctypes.c_int, [_vp]),
    "ge_row_shard": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _ip, _ip, _ip]),
    "ge_allgather_coords": (ctypes.c_int, [_vp, _vp, ctypes.c_longlong, ctypes.c_int]),
    "ge_assign_aggregates": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, _vp, ctypes.c_int,
                                            _i32p]),
    "ge_assign_aggregates_split": (ctypes.c_int, [ctypes.c_int, _i32p, _i32p, _vp, ctypes.c_int,
                                                  ctypes.c_int, _i32p]),
    "ge_allgather_members": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _i32p, _i32p,
                                            _i32p]),
    "ge_force_atlas_dist": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int,
                                           _f64p, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(FaParams)]),
    "ge_layout_energy_dist": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int,
                                             _f64p, ctypes.POINTER(FaParams), _vp, _f64p]),
    "ge_force_atlas_ml_dist": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p,
                                              ctypes.c_int, _i32p, _i32p, _i32p, _f64p, _f64p,
                                              _f64p, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(FaParams)]),
    "ge_ptap_dist": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _f64p, ctypes.c_int, _i32p,
                                    _i32p, ctypes.POINTER(_vp)]),
    "ge_embed_dist": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, _i32p, _i32p, _i32p, _i32p,
                                     _f64p, _i32p, _i32p, _i32p, _i32p, _i32p, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(FaParams), _f64p]),
}

_lib = None


def build():
    """Compile libge.so in-tree (hipcc --offload-arch=gfx950)."""
    subprocess.check_call(["make", "-s", "-C", PKG_ROOT, "-j8"])


def lib():
    global _lib
    if _lib is None:
        # torch ships its own libamdhip64.so.7; two HIP runtimes in one process
        # cannot share the device.  Load torch first (when present) so libge.so
        # binds to the runtime already in the process.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise GeError(f"{LIB_PATH} is missing: build it with `make -C {PKG_ROOT}` "
                          "(no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            # an older variant build (GE_LIB_PATH, tuning A/B only) may lack newer entry
            # points; the product library must export every one (tests/test_host.py)
            if os.environ.get("GE_LIB_PATH") and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        msg = lib().ge_last_error().decode(errors="replace")
        raise GeError(f"libge error {rc}: {msg}")


def params(**kw):
    p = FaParams()
    lib().ge_fa_params_default(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown ForceAtlas parameter {k}")
        setattr(p, k, v)
    return p


def device_count():
    c = ctypes.c_int(0)
    _check(lib().ge_device_count(ctypes.byref(c)))
    return c.value


def _csr(A):
    ip, ix, dx = A
    return (np.ascontiguousarray(ip, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.int32),
            np.ascontiguousarray(dx, dtype=np.float64))


def _layout_energy(fn, handle, A, X, rows, kw):
    ip, ix, dx = _csr(A)
    n = len(ip) - 1
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"coordinates must be n x dim with n = {n}, got {X.shape}")
    out = np.empty((n, ENERGY_COLS)) if rows else None
    totals = np.empty(ENERGY_COLS)
    p = params(**kw)
    _check(fn(handle, n, ip, ix, dx, X.shape[1], X.reshape(-1), ctypes.byref(p),
              out.ctypes.data if rows else None, totals))
    return out, totals


def relative_edge_length(totals, n, nnz):
    """lambda of include/ge.h: the mean length of a stored entry over the mean distance
    of a pair; scale-free, 1 for a random layout."""
    return (totals[ENERGY_EDGELEN] / nnz) / (totals[ENERGY_PAIRDIST] / (n * (n - 1.0)))


def _knn_args(X, rows):
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError(f"coordinates must be n x dim, got {X.shape}")
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    return X, rows, (X.shape[0] if rows is None else len(rows))


def layout_knn(X, k, rows=None, dist=False, ctx=None):
    """The exact k nearest neighbours of the query rows in the layout X (ge_layout_knn,
    "layout neighbours" in include/ge.h): idx (n_rows x k int32; -1 past the last
    candidate), in ascending order of (squared distance, index); with dist=True also the
    squared distances (+inf past the last candidate).  rows=None asks for every row;
    otherwise ids in any order, repeats allowed.  With a Context the pass runs on the
    device; without one (or GE_KNN_HOST=1) on the library's host path, with the same
    bits."""
    X, rows, n_rows = _knn_args(X, rows)
    k = int(k)
    idx = np.empty((n_rows, max(k, 0)), dtype=np.int32)
    d2 = np.empty((n_rows, max(k, 0))) if dist else None
    _check(lib().ge_layout_knn(ctx.h if ctx is not None else None, X.shape[0], X.shape[1],
                               X.reshape(-1), k, n_rows,
                               rows.ctypes.data if rows is not None else None, idx.ctypes.data,
                               d2.ctypes.data if dist else None))
    return (idx, d2) if dist else idx


def layout_neighbourhood(A, X, kmax=16, rows=None, ctx=None):
    """The neighbourhood precision's integers (ge_layout_neighbourhood): per query row
    {k_i, hits_i} (n_rows x 2 int32) and the totals (3 int64, NBHD_ROWS / NBHD_K /
    NBHD_HITS); neighbourhood_precision turns either into the score.  The rows of A must
    be ascending; its weights are not read."""
    ip = np.ascontiguousarray(A[0], dtype=np.int32)
    ix = np.ascontiguousarray(A[1], dtype=np.int32)
    X, rows, n_rows = _knn_args(X, rows)
    if X.shape[0] != len(ip) - 1:
        raise ValueError(f"coordinates must be n x dim with n = {len(ip) - 1}, got {X.shape}")
    per_row = np.empty((n_rows, 2), dtype=np.int32)
    totals = (ctypes.c_longlong * NBHD_TOTALS)()
    _check(lib().ge_layout_neighbourhood(ctx.h if ctx is not None else None, X.shape[0], ip, ix,
                                         X.shape[1], X.reshape(-1), int(kmax), n_rows,
                                         rows.ctypes.data if rows is not None else None,
                                         per_row.ctypes.data, totals))
    return per_row, np.array(list(totals), dtype=np.int64)


def neighbourhood_precision(per_row):
    """(mean, pooled) of layout_neighbourhood's per-row integers: the mean of hits_i / k_i
    over the rows with k_i > 0, and sum hits_i / sum k_i.  1 when every vertex has its
    graph neighbours nearest, about k / (n - 1) for a random layout; (nan, nan) when no
    row has a neighbour."""
    per_row = np.asarray(per_row).reshape(-1, 2)
    k, hits = per_row[:, 0].astype(np.int64), per_row[:, 1].astype(np.int64)
    live = k > 0
    if not live.any():
        return float("nan"), float("nan")
    return float((hits[live] / k[live]).mean()), float(hits.sum() / k.sum())


class Context:
    """One device + one HIP stream (ge_ctx)."""

    def __init__(self, device=0):
        h = _vp()
        _check(lib().ge_ctx_create(device, ctypes.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib().ge_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(lib().ge_ctx_set_stream(self.h, _vp(stream_ptr) if stream_ptr else None))

    def sync(self):
        _check(lib().ge_ctx_sync(self.h))

    # -- partition (device path) ---------------------------------------------
    def partition(self, A, coarsening_factor, **kw):
        return partition(A, coarsening_factor, ctx=self, **kw)

    def partition_single(self, A, num_parts=None, **kw):
        return partition_single(A, num_parts, ctx=self, **kw)

    # -- ForceAtlas ----------------------------------------------------------
    def force_atlas(self, A, dim, coords=None, iterations=100000, **kw):
        ip, ix, dx = _csr(A)
        n = len(ip) - 1
        X = np.zeros((n, dim)) if coords is None else np.array(coords, dtype=np.float64)
        X = np.ascontiguousarray(X)
        p = params(**kw)
        _check(lib().ge_force_atlas(self.h, n, ip, ix, dx, dim, X.reshape(-1),
                                    int(coords is None), iterations, ctypes.byref(p)))
        return X

    def force_atlas_ml(self, A, PT, vertex_A, coords_A, r_A, dim, iterations=10, **kw):
        ip, ix, dx = _csr(A)
        pip = np.ascontiguousarray(PT[0], dtype=np.int32)
        pix = np.ascontiguousarray(PT[1], dtype=np.int32)
        n = len(ip) - 1
        X = np.zeros((n, dim))
        p = params(**kw)
        _check(lib().ge_force_atlas_ml(
            self.h, n, ip, ix, dx, len(pip) - 1, pip, pix,
            np.ascontiguousarray(vertex_A, dtype=np.int32),
            np.ascontiguousarray(coords_A, dtype=np.float64).reshape(-1),
            np.ascontiguousarray(r_A, dtype=np.float64), X.reshape(-1), dim, iterations,
            ctypes.byref(p)))
        return X

    def embed_via_minimization_ml(self, A, PT, vertex_A, coords_A, r_A, dim, **kw):
        return embed_via_minimization_ml(A, PT, vertex_A, coords_A, r_A, dim, ctx=self, **kw)

    def force_atlas_batch(self, graphs, dim, coords=None, iterations=100000, seeds=None,
                          info=False, **kw):
        return force_atlas_batch(graphs, dim, coords=coords, iterations=iterations, seeds=seeds,
                                 info=info, ctx=self, **kw)

    def embed_via_force_atlas_ml(self, A, PT, vertex_A, coords_A, r_A, dim, **kw):
        return embed_via_force_atlas_ml(A, PT, vertex_A, coords_A, r_A, dim, ctx=self, **kw)

    def modularity(self, A, vertex_A, m):
        """partition::modularity with the O(nnz) pass on the device
        (ge_modularity_device); same bits as the host ge_amd.modularity."""
        import torch
        ip, ix, dx = _csr(A)
        dev = torch.device("cuda", self.device)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (ip, ix, dx, np.asarray(vertex_A, dtype=np.int32))]
        q = ctypes.c_double()
        _check(lib().ge_modularity_device(self.h, len(ip) - 1, _vp(t[0].data_ptr()),
                                          _vp(t[1].data_ptr()), _vp(t[2].data_ptr()), m,
                                          _vp(t[3].data_ptr()), ctypes.byref(q)))
        return q.value

    def ptap(self, A, PT, rows=None):
        """P_T A P_T^T; rows=(a0, a1): coarse rows [a0, a1) only (ge_ptap_rows)."""
        ip, ix, dx = _csr(A)
        pip = np.ascontiguousarray(PT[0], dtype=np.int32)
        pix = np.ascontiguousarray(PT[1], dtype=np.int32)
        h = _vp()
        if rows is None:
            _check(lib().ge_ptap(self.h, len(ip) - 1, ip, ix, dx, len(pip) - 1, pip, pix,
                                 ctypes.byref(h)))
        else:
            _check(lib().ge_ptap_rows(self.h, len(ip) - 1, ip, ix, dx, len(pip) - 1, pip, pix,
                                      rows[0], rows[1], ctypes.byref(h)))
        return _take_csr(h)

    def ptap_info(self):
        """ge_ptap_info of the last P^T A P call on this context: key widths bn, bb, ba,
        sort (one of PTAP_SORT_*), emitted entries and (row, column) runs."""
        v = [ctypes.c_int() for _ in range(4)] + [ctypes.c_longlong(), ctypes.c_longlong()]
        _check(lib().ge_ptap_info(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("bn", "bb", "ba", "sort", "entries", "runs"), (x.value for x in v)))

    def graph_info(self):
        """ge_graph_info of the last rmat_csr / largest_component on this context."""
        c = ctypes.c_longlong()
        v = [ctypes.c_int() for _ in range(3)]
        _check(lib().ge_graph_info(self.h, ctypes.byref(c), *[ctypes.byref(x) for x in v]))
        return dict(chunk=c.value, sort_segments=v[0].value, scans=v[1].value,
                    scan_calls=v[2].value)

    def radius_info(self):
        """ge_radius_info of the last radius_step on this context: (rounds, max pops in one)."""
        r, p = ctypes.c_int(), ctypes.c_int()
        _check(lib().ge_radius_info(self.h, ctypes.byref(r), ctypes.byref(p)))
        return r.value, p.value

    def embed(self, As, hier, dim, base_iterations=100000, ml_iterations=100,
              print_progress=False, **kw):
        parts = concat_levels(As, hier)
        out = np.empty((len(As[0][0]) - 1, dim))
        p = params(**kw)
        _check(lib().ge_embed(self.h, len(hier), *parts, dim, base_iterations, ml_iterations,
                              int(print_progress), ctypes.byref(p), out.reshape(-1)))
        return out

    def radius_step(self, coords_A, dim, coarse_is_base, PTc=None, coords_Ac=None, r_Ac=None,
                    Ac=None):
        """ge_radius_step_device: returns (r_A, coords_A after the rescale, ran_on_device)."""
        cA = np.array(coords_A, dtype=np.float64, copy=True).reshape(-1)
        m = cA.size // dim
        rA = np.zeros(m)
        keep = []

        def ptr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data_as(_vp)

        used = ctypes.c_int(-1)
        mc = 0 if PTc is None else len(PTc[0]) - 1
        _check(lib().ge_radius_step_device(
            self.h, m, cA, rA, dim, int(coarse_is_base), mc,
            ptr(None if PTc is None else PTc[0], np.int32),
            ptr(None if PTc is None else PTc[1], np.int32),
            ptr(coords_Ac, np.float64), ptr(r_Ac, np.float64),
            ptr(None if Ac is None else Ac[0], np.int32),
            ptr(None if Ac is None else Ac[1], np.int32), ctypes.byref(used)))
        return rA, cA.reshape(m, dim), bool(used.value)

    def rmat_csr(self, n, draws, seed=12345, lcc=False):
        """ge_rmat_csr_device: the R-MAT (or its largest component) built on the device."""
        h = _vp()
        _check(lib().ge_rmat_csr_device(self.h, n, draws, seed, int(lcc), ctypes.byref(h)))
        return _take_csr(h)

    def largest_component(self, A):
        ip, ix, dx = _csr(A)
        h = _vp()
        _check(lib().ge_largest_component_device(self.h, len(ip) - 1, ip, ix, dx,
                                                 ctypes.byref(h)))
        return _take_csr(h)

    def selftest_math(self, samples=1 << 24, seed=1):
        bad = ctypes.c_longlong()
        _check(lib().ge_selftest_math(self.h, samples, seed, ctypes.byref(bad)))
        return bad.value

    def math_cases(self, op, rows, dim=0):
        """ge_math_cases: the production helpers on the caller's operands.  op: "sqrt",
        "div", "pair" or "rep"; rows: one case per row (include/ge.h has the columns).
        Returns the raw result bits, one uint64 row per case."""
        code = MATH_OPS[op]
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        rows = rows.reshape(len(rows), -1)
        win = {"sqrt": 1, "div": 2, "pair": 3, "rep": 2 * dim + 3}[op]
        wout = {"sqrt": 2, "div": 2, "pair": 5, "rep": 2 * dim}[op]
        if rows.shape[1] != win:
            raise ValueError(f"{op}: {win} operands per case, got {rows.shape[1]}")
        out = np.zeros((len(rows), wout), dtype=np.uint64)
        _check(lib().ge_math_cases(self.h, code, dim, len(rows), rows.reshape(-1),
                                   out.reshape(-1)))
        return out

    def layout_energy(self, A, X, rows=True, **kw):
        """(rows, totals) of the layout X (n x dim) of graph A: the five ENERGY_* columns per
        vertex (n x 5; None with rows=False) and their sums (ge_layout_energy).  E is
        totals[ENERGY_REP] + totals[ENERGY_ATT] + totals[ENERGY_GRAV]."""
        return _layout_energy(lib().ge_layout_energy, self.h, A, X, rows, kw)

    def layout_knn(self, X, k, rows=None, dist=False):
        """layout_knn on the device (ge_layout_knn)."""
        return layout_knn(X, k, rows=rows, dist=dist, ctx=self)

    def layout_knn_device(self, n, dim, d_x, k, n_rows, d_rows, d_idx, d_dist2=None):
        """ge_layout_knn_device on device pointers (d_rows and d_dist2 may be None):
        enqueues on the context's stream and does not synchronise."""
        _check(lib().ge_layout_knn_device(self.h, n, dim, _vp(d_x), k, n_rows,
                                          _vp(d_rows) if d_rows else None,
                                          _vp(d_idx) if d_idx else None,
                                          _vp(d_dist2) if d_dist2 else None))

    def layout_neighbourhood(self, A, X, kmax=16, rows=None):
        """layout_neighbourhood with the neighbours from the device."""
        return layout_neighbourhood(A, X, kmax=kmax, rows=rows, ctx=self)

    def knn_info(self):
        """The last nearest-neighbour call on this context (ge_knn_info), to be read once
        its work is complete: the path and kernel form by name, the query rows per
        workgroup, the j splits and the list insertions summed over the call."""
        v = [ctypes.c_int(0) for _ in range(4)]
        ins = ctypes.c_longlong(0)
        _check(lib().ge_knn_info(self.h, *(ctypes.byref(x) for x in v), ctypes.byref(ins)))
        return {"path": KNN_PATHS[v[0].value], "form": KNN_FORMS[v[1].value],
                "rows_per_wg": v[2].value, "jsplit": v[3].value, "insertions": ins.value}

    def fa_plan(self, n, nnz, d_ip, d_ix, d_dx, dim, row_begin, row_end, **kw):
        return FaPlan(self, n, nnz, d_ip, d_ix, d_dx, dim, row_begin, row_end, **kw)


_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, _vp, _vp, _vp, ctypes.c_ulonglong)


class _Transport(ctypes.Structure):
    _fields_ = [("user", _vp), ("allgather", _ALLGATHER_FN)]


def _torch_allgather(send, recv, nbytes):
    """ge_transport.allgather over the default torch.distributed group (gloo):
    host byte blocks, rank-major."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size()
    if nbytes == 0:
        dist.barrier()
        return
    src = np.ctypeslib.as_array((ctypes.c_ubyte * nbytes).from_address(send))
    dst = np.ctypeslib.as_array((ctypes.c_ubyte * (nbytes * world)).from_address(recv))
    outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
    dist.all_gather(outs, torch.from_numpy(src.copy()))
    for r, t in enumerate(outs):
        dst[r * nbytes:(r + 1) * nbytes] = t.numpy()


class Comm:
    """ge_comm: the library's communicator for one rank (one process per GPU).

    backend "rccl": ncclCommInitRank inside libge; the 128-byte unique id made by
    rank 0 (unique_id()) must be handed to every rank (e.g. broadcast_object_list).
    backend "transport": the library's collectives call back into Python, which
    all-gathers host blocks over torch.distributed's default group (gloo) -- the
    multi-process rehearsal on one GPU and the CPU-side tests."""

    def __init__(self, ctx, nranks, rank, backend="rccl", uid=None):
        self.ctx, self.nranks, self.rank = ctx, nranks, rank
        h = _vp()
        if backend == "rccl":
            assert uid is not None and len(uid) == 128
            _check(lib().ge_comm_create(ctx.h, nranks, rank, bytes(uid), ctypes.byref(h)))
        else:
            def cb(user, send, recv, nbytes):
                try:
                    _torch_allgather(send, recv, int(nbytes))
                    return 0
                except Exception:  # reported to the library as a failed collective
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = _ALLGATHER_FN(cb)  # kept alive with the communicator
            self._tp = _Transport(None, self._cb)
            _check(lib().ge_comm_create_transport(ctx.h, nranks, rank,
                                                  ctypes.cast(ctypes.byref(self._tp), _vp),
                                                  ctypes.byref(h)))
        self.h = h

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _check(lib().ge_comm_unique_id(buf))
        return buf.raw

    def info(self):
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().ge_comm_info(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, bool(c.value)

    def close(self):
        if getattr(self, "h", None):
            lib().ge_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def allgather_coords(self, d_x, rows_per_rank, dim):
        _check(lib().ge_allgather_coords(self.h, _vp(d_x), rows_per_rank, dim))

    def allgather_members(self, d_x, dim, PT, owner):
        pip = np.ascontiguousarray(PT[0], dtype=np.int32)
        pix = np.ascontiguousarray(PT[1], dtype=np.int32)
        _check(lib().ge_allgather_members(self.h, _vp(d_x), dim, len(pip) - 1, pip, pix,
                                          np.ascontiguousarray(owner, dtype=np.int32)))

    def force_atlas(self, A, dim, coords=None, iterations=100000, **kw):
        ip, ix, dx = _csr(A)
        n = len(ip) - 1
        X = np.zeros((n, dim)) if coords is None else np.array(coords, dtype=np.float64)
        X = np.ascontiguousarray(X)
        p = params(**kw)
        _check(lib().ge_force_atlas_dist(self.h, n, ip, ix, dx, dim, X.reshape(-1),
                                         int(coords is None), iterations, ctypes.byref(p)))
        return X

    def layout_energy(self, A, X, rows=True, **kw):
        """Context.layout_energy over row shards (ge_layout_energy_dist): the same bits on
        every rank."""
        return _layout_energy(lib().ge_layout_energy_dist, self.h, A, X, rows, kw)

    def force_atlas_ml(self, A, PT, vertex_A, coords_A, r_A, dim, iterations=10, **kw):
        ip, ix, dx = _csr(A)
        pip = np.ascontiguousarray(PT[0], dtype=np.int32)
        pix = np.ascontiguousarray(PT[1], dtype=np.int32)
        n = len(ip) - 1
        X = np.zeros((n, dim))
        p = params(**kw)
        _check(lib().ge_force_atlas_ml_dist(
            self.h, n, ip, ix, dx, len(pip) - 1, pip, pix,
            np.ascontiguousarray(vertex_A, dtype=np.int32),
            np.ascontiguousarray(coords_A, dtype=np.float64).reshape(-1),
            np.ascontiguousarray(r_A, dtype=np.float64), X.reshape(-1), dim, iterations,
            ctypes.byref(p)))
        return X

    def ptap(self, A, PT):
        ip, ix, dx = _csr(A)
        pip = np.ascontiguousarray(PT[0], dtype=np.int32)
        pix = np.ascontiguousarray(PT[1], dtype=np.int32)
        h = _vp()
        _check(lib().ge_ptap_dist(self.h, len(ip) - 1, ip, ix, dx, len(pip) - 1, pip, pix,
                                  ctypes.byref(h)))
        return _take_csr(h)

    def embed(self, As, hier, dim, base_iterations=100000, ml_iterations=100,
              print_progress=False, **kw):
        parts = concat_levels(As, hier)
        out = np.empty((len(As[0][0]) - 1, dim))
        p = params(**kw)
        _check(lib().ge_embed_dist(self.h, len(hier), *parts, dim, base_iterations,
                                   ml_iterations, int(print_progress), ctypes.byref(p),
                                   out.reshape(-1)))
        return out


def assign_aggregates_split(PT, indptr, nranks, min_members=-1):
    """ge_assign_aggregates_split: owner per aggregate, -1 for the aggregates split
    by row tiles over all ranks (min_members > 0: every aggregate at least that
    large; 0: none; < 0: the automatic rule)."""
    pip = np.ascontiguousarray(PT[0], dtype=np.int32)
    pix = np.ascontiguousarray(PT[1], dtype=np.int32)
    owner = np.empty(len(pip) - 1, dtype=np.int32)
    ipa = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.int32)
    _check(lib().ge_assign_aggregates_split(len(pip) - 1, pip, pix,
                                            None if ipa is None else ipa.ctypes.data_as(_vp),
                                            nranks, min_members, owner))
    return owner


def assign_aggregates(PT, indptr, nranks):
    """ge_assign_aggregates: the rank of every aggregate (LPT by s(s-1) + the
    members' CSR entries when indptr is given)."""
    pip = np.ascontiguousarray(PT[0], dtype=np.int32)
    pix = np.ascontiguousarray(PT[1], dtype=np.int32)
    owner = np.empty(len(pip) - 1, dtype=np.int32)
    ipa = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.int32)
    _check(lib().ge_assign_aggregates(len(pip) - 1, pip, pix,
                                      None if ipa is None else ipa.ctypes.data_as(_vp), nranks,
                                      owner))
    return owner


def row_shard(n, nranks, rank):
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(lib().ge_row_shard(n, nranks, rank, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


FAML_SCHED_TABLES = ("order", "beg", "rows", "irows", "huge", "xrows", "xcounts", "items",
                     "fitems", "units")  # GE_FAML_SCHED_*; the scalars follow
FAML_SCHED_FARAGGS = 11  # GE_FAML_SCHED_FARAGGS: faml_schedule()["faraggs"]
FAML_SCHED_SCALARS = ("res_cap", "small", "mid", "large", "streamed", "off_mid", "off_large",
                      "blocks_small", "blocks_mid", "blocks_large", "R", "U", "code", "fast",
                      "sym", "wide", "ntiles", "sweeps", "row_blocks", "sym_blocks")


def faml_schedule(pt_indptr, dim, cus, sym_occ, aggs=None, split=None, rank=0, nranks=1,
                  mode=MODE_STRICT):
    """The schedule a FamlPlan over these aggregates would settle on, without a device
    (ge_faml_sched_*): {table name: int32 array} for FAML_SCHED_TABLES, the scalars of
    FAML_SCHED_SCALARS, streamed_pairs and faraggs (mode=MODE_FARFIELD: the aggregates
    that take the far field, larger first).  aggs: default all; the GE_FAML_* knobs and
    GE_FAR_MIN_ML are read from the environment as the plan reads them."""
    pip = np.ascontiguousarray(pt_indptr, dtype=np.int32)
    m = len(pip) - 1
    ids = np.ascontiguousarray(np.arange(m) if aggs is None else aggs, dtype=np.int32)
    sp = np.ascontiguousarray(np.zeros(0) if split is None else split, dtype=np.int32)
    h = _vp()
    _check(lib().ge_faml_sched_create(m, pip, ids, len(ids), sp, len(sp), rank, nranks, dim,
                                      mode, cus, sym_occ, ctypes.byref(h)))
    try:
        out = {}
        for k, name in enumerate(FAML_SCHED_TABLES + ("scalars",)):
            p, n = _ip(), ctypes.c_longlong()
            _check(lib().ge_faml_sched_table(h, k, ctypes.byref(p), ctypes.byref(n)))
            out[name] = (np.ctypeslib.as_array(p, (n.value,)).astype(np.int32) if n.value
                         else np.zeros(0, dtype=np.int32))
        out.update(zip(FAML_SCHED_SCALARS, (int(v) for v in out.pop("scalars"))))
        p, n = _ip(), ctypes.c_longlong()
        _check(lib().ge_faml_sched_table(h, FAML_SCHED_FARAGGS, ctypes.byref(p), ctypes.byref(n)))
        out["faraggs"] = (np.ctypeslib.as_array(p, (n.value,)).astype(np.int32) if n.value
                          else np.zeros(0, dtype=np.int32))
        d = ctypes.c_double()
        _check(lib().ge_faml_sched_pairs(h, ctypes.byref(d)))
        out["streamed_pairs"] = d.value
    finally:
        lib().ge_faml_sched_destroy(h)
    return out


class FamlPlan:
    """Device-resident multilevel level (ge_faml_plan_*): P_T's indptr on the host
    (pt_indptr_host, numpy) plus device pointers for everything else."""

    def __init__(self, ctx, n, d_ip, d_ix, d_dx, pt_indptr_host, d_pt_ip, d_pt_ix, d_vA, dim,
                 iterations=100, agg_range=None, aggs=None, split=None, comm=None, **kw):
        """agg_range=(a0, a1) or aggs=(strictly increasing aggregate ids) restricts
        the plan to those aggregates (one rank's share); default: all.  split (with
        comm): aggregates split by row tiles over comm's ranks
        (ge_faml_plan_create_shard)."""
        self.ctx = ctx
        pip = np.ascontiguousarray(pt_indptr_host, dtype=np.int32)
        m = len(pip) - 1
        p = params(**kw)
        h = _vp()
        if comm is not None:
            ids = np.ascontiguousarray(np.zeros(0) if aggs is None else aggs, dtype=np.int32)
            sp = np.ascontiguousarray(np.zeros(0) if split is None else split, dtype=np.int32)
            _check(lib().ge_faml_plan_create_shard(
                ctx.h, comm.h, n, _vp(d_ip), _vp(d_ix), _vp(d_dx), m, pip, _vp(d_pt_ip),
                _vp(d_pt_ix), _vp(d_vA), dim, ctypes.byref(p), iterations, ids, len(ids), sp,
                len(sp), ctypes.byref(h)))
        elif aggs is not None:
            ids = np.ascontiguousarray(aggs, dtype=np.int32)
            _check(lib().ge_faml_plan_create_subset(
                ctx.h, n, _vp(d_ip), _vp(d_ix), _vp(d_dx), m, pip, _vp(d_pt_ip), _vp(d_pt_ix),
                _vp(d_vA), dim, ctypes.byref(p), iterations, ids, len(ids), ctypes.byref(h)))
        else:
            a0, a1 = agg_range if agg_range else (0, m)
            _check(lib().ge_faml_plan_create(ctx.h, n, _vp(d_ip), _vp(d_ix), _vp(d_dx), m, pip,
                                             _vp(d_pt_ip), _vp(d_pt_ix), _vp(d_vA), dim,
                                             ctypes.byref(p), iterations, a0, a1,
                                             ctypes.byref(h)))
        self.h = h
        self.dim = dim

    def run(self, d_cA, d_rA, d_init, d_x):
        _check(lib().ge_faml_plan_run(self.h, _vp(d_cA), _vp(d_rA), _vp(d_init), _vp(d_x)))

    def mode(self):
        """(mode, fast_items): MODE_FARFIELD when an aggregate runs the far field, else
        MODE_FAST only when the closed-form repulsion kernel is scheduled for the streamed
        aggregates; fast_items: its row items per launch (ge_faml_plan_mode); otherwise
        (MODE_STRICT, 0)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        _check(lib().ge_faml_plan_mode(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def repulse(self, d_x, d_frep):
        """One repulsion pass of the streamed aggregates on the coordinates d_x (n * dim,
        P_T storage order) into d_frep, same layout; other members' positions are left
        untouched (ge_faml_plan_repulse)."""
        _check(lib().ge_faml_plan_repulse(self.h, _vp(d_x), _vp(d_frep)))

    def far_info(self):
        """ge_faml_plan_far_info: active, reason (FAR_REASONS), theta, far_min_ml, item_rows,
        key_bits (per axis), aggregates (the far aggregates' ids, larger first), rows and, of
        the last pass, bad_boxes, accepted (cells per level, GE_FAR_MAX_LEVELS entries),
        exact_leaves, pair_terms, prep_ms, item_ms."""
        act, why, fmin, rows_i, bits, nagg, bad = (ctypes.c_int() for _ in range(7))
        th, prep, item = (ctypes.c_double() for _ in range(3))
        acc = (ctypes.c_longlong * FAR_MAX_LEVELS)()
        rows, leaves, terms = (ctypes.c_longlong() for _ in range(3))
        _check(lib().ge_faml_plan_far_info(
            self.h, ctypes.byref(act), ctypes.byref(why), ctypes.byref(th), ctypes.byref(fmin),
            ctypes.byref(rows_i), ctypes.byref(bits), ctypes.byref(nagg), ctypes.byref(rows),
            ctypes.byref(bad), acc, ctypes.byref(leaves), ctypes.byref(terms), ctypes.byref(prep),
            ctypes.byref(item)))
        aggs = np.zeros(nagg.value, dtype=np.int32)
        if nagg.value:
            _check(lib().ge_faml_plan_far_aggregates(self.h, aggs.ctypes.data_as(_vp)))
        return {"active": bool(act.value), "reason": FAR_REASONS[why.value], "theta": th.value,
                "far_min_ml": fmin.value, "item_rows": rows_i.value, "key_bits": bits.value,
                "aggregates": [int(a) for a in aggs], "rows": rows.value,
                "bad_boxes": bad.value, "accepted": list(acc), "exact_leaves": leaves.value,
                "pair_terms": terms.value, "prep_ms": prep.value, "item_ms": item.value}

    def far_layout(self, agg):
        """ge_faml_plan_far_layout: what the last pass used for far aggregate `agg`, in the
        form of FaPlan.far_layout(): perm (the position within the aggregate at each sorted
        position), keys, box, cells (one array per level, leaves first), items, item_rows,
        theta and key_bits."""
        info = self.far_info()
        mem, lv, nit = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        cnt = (ctypes.c_int * FAR_MAX_LEVELS)()
        _check(lib().ge_faml_plan_far_shape(self.h, agg, ctypes.byref(mem), ctypes.byref(lv), cnt,
                                            ctypes.byref(nit)))
        s, d, L = mem.value, self.dim, lv.value
        level_cells = list(cnt)[:L]
        perm = np.empty(s, dtype=np.int32)
        keys = np.empty(s, dtype=np.uint64)
        box = np.empty(d + 1)
        cells = np.empty((sum(level_cells), d + 2))
        items = np.empty((nit.value, d + 2))
        _check(lib().ge_faml_plan_far_layout(self.h, agg, *(a.ctypes.data_as(_vp)
                                                            for a in (perm, keys, box, cells, items))))
        offs = np.cumsum([0] + level_cells)
        return {"perm": perm, "keys": keys, "box": box, "items": items,
                "item_rows": info["item_rows"], "theta": info["theta"],
                "key_bits": info["key_bits"],
                "cells": [cells[offs[l]:offs[l + 1]] for l in range(L)]}

    def set_profiling(self, on):
        _check(lib().ge_faml_plan_set_profiling(self.h, int(on)))

    def kernel_ms(self):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _check(lib().ge_faml_plan_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b),
                                            ctypes.byref(c)))
        return a.value, b.value, c.value

    def repulse_ms(self):
        """(average ms of one streamed repulsion launch, launches profiled,
        ordered pairs per launch)"""
        a, c, p = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        _check(lib().ge_faml_plan_repulse_ms(self.h, ctypes.byref(a), ctypes.byref(c),
                                             ctypes.byref(p)))
        return a.value, c.value, p.value

    def rows_ms(self):
        """(average ms of one streamed member-row pass, passes profiled, rows, CSR
        entries per pass)"""
        a, c = ctypes.c_double(), ctypes.c_int()
        r, e = ctypes.c_longlong(), ctypes.c_longlong()
        _check(lib().ge_faml_plan_rows_ms(self.h, ctypes.byref(a), ctypes.byref(c),
                                          ctypes.byref(r), ctypes.byref(e)))
        return a.value, c.value, r.value, e.value

    def schedule(self):
        """{sweeps, banded, row_blocks, units}: how the streamed aggregates' repulsion
        is scheduled (ge_faml_plan_schedule)."""
        v = [ctypes.c_int() for _ in range(4)]
        _check(lib().ge_faml_plan_schedule(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("sweeps", "banded", "row_blocks", "units"), (x.value for x in v)))

    def classes(self):
        """The size class every aggregate took and the classes of the streamed members'
        rows (ge_faml_plan_classes): res_cap; aggregates small / mid / large / streamed;
        blocks_small / blocks_mid / blocks_large of the resident launches; ntiles, nheavy,
        nseg, seg_mode, nearly, nseg_early of the rows (late heavy rows: nheavy - nearly)."""
        cap = ctypes.c_int()
        aggs, blocks, rows = (ctypes.c_int * 4)(), (ctypes.c_int * 3)(), (ctypes.c_int * 6)()
        _check(lib().ge_faml_plan_classes(self.h, ctypes.byref(cap), aggs, blocks, rows))
        out = {"res_cap": cap.value}
        out.update(zip(("small", "mid", "large", "streamed"), aggs))
        out.update(zip(("blocks_small", "blocks_mid", "blocks_large"), blocks))
        out.update(zip(("ntiles", "nheavy", "nseg", "seg_mode", "nearly", "nseg_early"), rows))
        return out

    def close(self):
        """Destroys the plan; raises GeError when the library reports a failure
        that surfaced only at teardown (e.g. a sweep hand-over wait that timed out
        after the last step).  __del__ swallows it."""
        if self.h:
            h, self.h = self.h, None
            _check(lib().ge_faml_plan_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# GE_FA_STEP_*, GE_FA_REP_* and the scalars GE_FA_SCHED_* of include/ge.h, in index order
FA_STEPS = ("fused", "stream", "split")
FA_REPS = ("grouped", "ordered", "ordered_wide", "fast", "sweeps", "farfield")
FA_SCHED_PLAN_SCALARS = ("mode", "step", "rep", "wide", "lanes", "repel_one", "linear", "per",
                         "nb", "R", "fast_blocks", "fast_jb", "sym", "far_reason",
                         "far_item_rows", "fpart")
FA_SCHED_RUN_SCALARS = ("small", "small_g_domain", "small_g_general", "small_staged",
                        "small_handover", "persist", "persist_g", "packed", "pack_rows", "graph")
FA_SCHED_SCALARS = FA_SCHED_PLAN_SCALARS + FA_SCHED_RUN_SCALARS
FA_SCHED_COUNT = 26  # GE_FA_SCHED_COUNT
_FA_SCHED_FLAGS = ("wide", "repel_one", "linear", "sym", "fpart", "small", "small_staged",
                   "persist", "packed", "graph")


def _fa_sched_dict(names, values):
    out = dict(zip(names, (int(v) for v in values)))
    out["step"] = FA_STEPS[out["step"]]
    out["rep"] = FA_REPS[out["rep"]]
    out["far_reason"] = FAR_REASONS[out["far_reason"]]
    for k in _FA_SCHED_FLAGS:
        if k in out:
            out[k] = bool(out[k])
    return out


def fa_schedule(n, dim, cus, rb=0, re=None, iterations=0, nnz=0, masses_ok=True, **params_kw):
    """The single-level schedule (ge_fa_sched_query; graph-embed_amd/csrc/ge_fa_sched.hpp)
    with no device touched: which kernels a plan over rows [rb, re) of n vertices runs on
    a device of `cus` compute units under the knobs now in the environment
    (FA_SCHED_PLAN_SCALARS), and how ge_force_atlas runs `iterations` of the whole level
    with nnz CSR entries (FA_SCHED_RUN_SCALARS).  step, rep and far_reason come as the
    names of FA_STEPS, FA_REPS and FAR_REASONS, mode as MODE_*; masses_ok: the answer of
    the far field's device check."""
    out = (ctypes.c_int * FA_SCHED_COUNT)()
    p = params(**params_kw)
    _check(lib().ge_fa_sched_query(n, rb, n if re is None else re, dim, ctypes.byref(p), cus, nnz,
                                   iterations, int(masses_ok), out))
    return _fa_sched_dict(FA_SCHED_SCALARS, out)


FA_BATCH_CLASSES = ("wave", "block", "serial")  # GE_FA_BATCH_*
FA_BATCH_TOTALS = ("waves", "blocks", "serials", "wave_workgroups")


def fa_batch_schedule(sizes, entries, dim, **params_kw):
    """The batch schedule (ge_fa_batch_sched_query; fa_batch_schedule in
    graph-embed_amd/csrc/ge_fa_sched.hpp) with no device touched, under the knobs now in
    the environment: per graph of sizes[g] rows and entries[g] stored entries its class
    (0 wave, 1 block, 2 serial: FA_BATCH_CLASSES) and lanes per row (0: serial), and the
    totals of FA_BATCH_TOTALS."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    entries = np.ascontiguousarray(entries, dtype=np.int32)
    if sizes.shape != entries.shape or sizes.ndim != 1:
        raise ValueError("sizes and entries must be 1-D and of one length")
    cls, lanes = np.zeros(len(sizes), dtype=np.int32), np.zeros(len(sizes), dtype=np.int32)
    totals = (ctypes.c_int * len(FA_BATCH_TOTALS))()
    p = params(**params_kw)
    _check(lib().ge_fa_batch_sched_query(len(sizes), sizes, entries, dim, ctypes.byref(p), cls,
                                         lanes, totals))
    return {"cls": cls, "lanes": lanes, **dict(zip(FA_BATCH_TOTALS, totals))}


def concat_graphs(graphs):
    """A list of CSR matrices as the block-diagonal CSR of ge_force_atlas_batch:
    (off, indptr, indices, data) with graph g on rows and columns [off[g], off[g+1])."""
    gs = [_csr(A) for A in graphs]
    off = np.zeros(len(gs) + 1, dtype=np.int64)
    eoff = np.zeros(len(gs) + 1, dtype=np.int64)
    for g, (ip, ix, _) in enumerate(gs):
        off[g + 1] = off[g] + len(ip) - 1
        eoff[g + 1] = eoff[g] + len(ix)
    ip = np.concatenate([np.zeros(1, dtype=np.int64)] +
                        [a[0][1:].astype(np.int64) + eoff[g] for g, a in enumerate(gs)])
    ix = np.concatenate([np.zeros(0, dtype=np.int64)] +
                        [a[1].astype(np.int64) + off[g] for g, a in enumerate(gs)])
    dx = np.concatenate([np.zeros(0)] + [a[2] for a in gs])
    return (off.astype(np.int32), ip.astype(np.int32), ix.astype(np.int32),
            np.ascontiguousarray(dx, dtype=np.float64))


def force_atlas_batch(graphs, dim, coords=None, iterations=100000, seeds=None, info=False,
                      ctx=None, **kw):
    """ge_force_atlas_batch: forceAtlas on every CSR matrix of `graphs` in one device call,
    each with the bits of Context.force_atlas on it alone.  coords: a list of n_g x dim
    arrays (None: every graph draws its start from mt19937(seeds[g]), or from
    mt19937(seed) when seeds is None).  Returns the list of coordinates; info=True also
    the class totals (FA_BATCH_TOTALS) of the call.  ctx=None only checks the arguments
    (the library then reports the missing context)."""
    off, ip, ix, dx = concat_graphs(graphs)
    N = int(off[-1])
    if coords is None:
        X = np.zeros((N, dim))
    else:
        if len(coords) != len(graphs):
            raise ValueError("one coordinate array per graph")
        X = np.concatenate([np.zeros((0, dim))] + [
            np.asarray(c, dtype=np.float64).reshape(-1, dim) for c in coords])
        if len(X) != N:
            raise ValueError("coordinates must be n_g x dim per graph")
    X = np.ascontiguousarray(X)
    sd = None
    if seeds is not None:
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        if len(sd) != len(graphs):
            raise ValueError("one seed per graph")
    out = _force_atlas_batch_raw(ctx, off, ip, ix, dx, dim, X, coords is None, sd, iterations, kw)
    res = [out[off[g]:off[g + 1]] for g in range(len(graphs))]
    if not info:
        return res
    totals = (ctypes.c_int * len(FA_BATCH_TOTALS))()
    _check(lib().ge_fa_batch_info(ctx.h, totals))
    return res, dict(zip(FA_BATCH_TOTALS, totals))


def _force_atlas_batch_raw(ctx, off, ip, ix, dx, dim, X, init_random, seeds, iterations, kw):
    """ge_force_atlas_batch on the block-diagonal arrays as given (the tests' error cases)."""
    p = params(**kw)
    _check(lib().ge_force_atlas_batch(
        ctx.h if ctx is not None else None, len(off) - 1, off, ip, ix, dx, dim, X.reshape(-1),
        int(init_random), seeds.ctypes.data if seeds is not None else None, iterations,
        ctypes.byref(p)))
    return X


def embed_via_force_atlas_ml(A, PT, vertex_A, coords_A, r_A, dim, iterations=100000, ctx=None,
                             info=False, **kw):
    """anyToMultilevel(forceAtlas) on one level (src/embed.cpp:23-83 over
    include/forceatlas.hpp:307-312) as one ge_embed_via_force_atlas_ml call: per
    aggregate of PT, forceAtlas from the random start of mt19937(seed) on the members'
    internal entries, normalised by its largest norm and placed in the aggregate's ball.
    info=True also returns the batch's class totals (FA_BATCH_TOTALS)."""
    ip = np.ascontiguousarray(A[0], dtype=np.int32)
    ix = np.ascontiguousarray(A[1], dtype=np.int32)
    pip = np.ascontiguousarray(PT[0], dtype=np.int32)
    pix = np.ascontiguousarray(PT[1], dtype=np.int32)
    n, m = len(ip) - 1, len(pip) - 1
    vA = np.ascontiguousarray(vertex_A, dtype=np.int32)
    cA = np.ascontiguousarray(coords_A, dtype=np.float64).reshape(-1)
    rA = np.ascontiguousarray(r_A, dtype=np.float64).reshape(-1)
    if len(vA) != n or len(cA) != m * dim or len(rA) != m or len(pix) != n:
        raise GeError("embed_via_force_atlas_ml: array sizes do not match n, m and dim")
    X = np.zeros((n, dim))
    totals = (ctypes.c_int * len(FA_BATCH_TOTALS))()
    p = params(**kw)
    _check(lib().ge_embed_via_force_atlas_ml(ctx.h if ctx is not None else None, n, ip, ix, m, pip,
                                             pix, vA, cA, rA, dim, iterations, ctypes.byref(p),
                                             X.reshape(-1), totals))
    if not info:
        return X
    return X, dict(zip(FA_BATCH_TOTALS, totals))


class FaPlan:
    """Device-resident ForceAtlas iteration over rows [row_begin, row_end)
    (ge_fa_plan_*).  Device pointers are raw integers (e.g. tensor.data_ptr())."""

    def __init__(self, ctx, n, nnz, d_ip, d_ix, d_dx, dim, row_begin, row_end, **kw):
        self.ctx = ctx
        self.n, self.dim = n, dim
        p = params(**kw)
        h = _vp()
        _check(lib().ge_fa_plan_create(ctx.h, n, nnz, _vp(d_ip), _vp(d_ix), _vp(d_dx), dim,
                                       ctypes.byref(p), row_begin, row_end, ctypes.byref(h)))
        self.h = h

    def step(self, d_x_cur, d_x_next):
        _check(lib().ge_fa_plan_step(self.h, _vp(d_x_cur), _vp(d_x_next)))

    def attract(self, d_x_cur, d_frep, d_x_next):
        """Attraction + gravity + update alone on supplied repulsion sums
        (ge_fa_plan_attract)."""
        _check(lib().ge_fa_plan_attract(self.h, _vp(d_x_cur), _vp(d_frep), _vp(d_x_next)))

    def repulse(self, d_x, d_frep):
        """One repulsion pass alone on the coordinates d_x (n * dim) into d_frep (the
        plan's rows * dim), in the plan's mode (ge_fa_plan_repulse)."""
        _check(lib().ge_fa_plan_repulse(self.h, _vp(d_x), _vp(d_frep)))

    def schedule(self):
        """The kernels this plan runs (ge_fa_plan_schedule): fa_schedule's
        FA_SCHED_PLAN_SCALARS as the live plan holds them."""
        out = (ctypes.c_int * FA_SCHED_COUNT)()
        _check(lib().ge_fa_plan_schedule(self.h, out))
        return _fa_sched_dict(FA_SCHED_PLAN_SCALARS, out)

    def forces(self, d_out):
        """Copies the forces of the last step or attract ((row_end - row_begin) * dim
        doubles) to the device buffer d_out on the plan's stream (ge_fa_plan_forces)."""
        _check(lib().ge_fa_plan_forces(self.h, _vp(d_out)))

    def energy(self, d_x, d_rows=None):
        """The totals (5 doubles, ENERGY_*) of the layout energy of the coordinates d_x
        (n * dim, device) over the plan's rows; d_rows (device, rows * 5) receives the
        per-row columns (ge_fa_plan_energy).  Synchronises; the plan is not disturbed."""
        totals = np.empty(ENERGY_COLS)
        _check(lib().ge_fa_plan_energy(self.h, _vp(d_x), _vp(d_rows) if d_rows else None, totals))
        return totals

    def rows_info(self):
        """ge_fa_plan_rows_info: ntiles, nheavy, nmed, nlight, nseg, seg_mode of the plan's
        rows; heavy_rows (their ids, longest first) and heavy_status (how the last row
        pass finished each: ROW_BINADE, or'ed ROW_SERIAL_FLAG / _BASE / _RANGE,
        ROW_SERIAL_WHOLE, or ROW_NONE before any pass)."""
        cls = (ctypes.c_int * 6)()
        _check(lib().ge_fa_plan_rows_info(self.h, cls, None, None))
        out = dict(zip(("ntiles", "nheavy", "nmed", "nlight", "nseg", "seg_mode"), cls))
        rows = np.empty(out["nheavy"], dtype=np.int32)
        stat = np.empty(out["nheavy"], dtype=np.int32)
        if out["nheavy"]:
            _check(lib().ge_fa_plan_rows_info(self.h, cls, rows.ctypes.data_as(_vp),
                                              stat.ctypes.data_as(_vp)))
        out["heavy_rows"], out["heavy_status"] = rows, stat
        return out

    def far_info(self):
        """ge_fa_plan_far_info: active, reason (FAR_REASONS), theta, item_rows, levels,
        level_cells / level_points per level (leaves first) and, of the last pass,
        fallback, accepted (cells per level), exact_leaves, pair_terms, prep_ms, item_ms."""
        act, why, rows, lv, fb = (ctypes.c_int() for _ in range(5))
        th, prep, item = (ctypes.c_double() for _ in range(3))
        cells = (ctypes.c_int * FAR_MAX_LEVELS)()
        pts, acc = (ctypes.c_longlong * FAR_MAX_LEVELS)(), (ctypes.c_longlong * FAR_MAX_LEVELS)()
        leaves, terms = ctypes.c_longlong(), ctypes.c_longlong()
        _check(lib().ge_fa_plan_far_info(
            self.h, ctypes.byref(act), ctypes.byref(why), ctypes.byref(th), ctypes.byref(rows),
            ctypes.byref(lv), cells, pts, ctypes.byref(fb), acc, ctypes.byref(leaves),
            ctypes.byref(terms), ctypes.byref(prep), ctypes.byref(item)))
        L = lv.value
        return {"active": bool(act.value), "reason": FAR_REASONS[why.value], "theta": th.value,
                "item_rows": rows.value, "levels": L, "level_cells": list(cells)[:L],
                "level_points": list(pts)[:L], "fallback": bool(fb.value),
                "accepted": list(acc)[:L], "exact_leaves": leaves.value,
                "pair_terms": terms.value, "prep_ms": prep.value, "item_ms": item.value}

    def far_layout(self):
        """ge_fa_plan_far_layout: what the last far-field pass used.  perm (the vertex at
        each sorted position), keys (sorted Morton keys), box (lower corner, key scale),
        cells (one array per level, leaves first, rows {c_0 .. c_{d-1}, M, a}) and items
        (same rows; item q holds sorted rows [q item_rows, (q + 1) item_rows))."""
        info = self.far_info()
        if not info["active"]:
            raise GeError("the far field does not run on this plan: " + info["reason"])
        n, d = self.n, self.dim
        nitems = -(-n // info["item_rows"])
        perm = np.empty(n, dtype=np.int32)
        keys = np.empty(n, dtype=np.uint64)
        box = np.empty(d + 1)
        cells = np.empty((sum(info["level_cells"]), d + 2))
        items = np.empty((nitems, d + 2))
        _check(lib().ge_fa_plan_far_layout(self.h, *(a.ctypes.data_as(_vp)
                                                     for a in (perm, keys, box, cells, items))))
        offs = np.cumsum([0] + info["level_cells"])
        return {"perm": perm, "keys": keys, "box": box, "items": items,
                "item_rows": info["item_rows"], "theta": info["theta"],
                "cells": [cells[offs[l]:offs[l + 1]] for l in range(info["levels"])]}

    def set_profiling(self, on):
        _check(lib().ge_fa_plan_set_profiling(self.h, int(on)))

    def kernel_ms(self):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _check(lib().ge_fa_plan_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b),
                                          ctypes.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        """Destroys the plan; raises GeError when the library reports a failure
        that surfaced only at teardown (e.g. a sweep hand-over wait that timed out
        after the last step).  __del__ swallows it."""
        if self.h:
            h, self.h = self.h, None
            _check(lib().ge_fa_plan_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _take_csr(h):
    r, c, z = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    _check(lib().ge_csr_shape(h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(z)))
    ip = np.empty(r.value + 1, dtype=np.int32)
    ix = np.empty(z.value, dtype=np.int32)
    dx = np.empty(z.value, dtype=np.float64)
    _check(lib().ge_csr_copy(h, ip, ix.ctypes.data_as(_vp), dx.ctypes.data_as(_vp)))
    lib().ge_csr_free(h)
    return ip, ix, dx


# -- host-resident entry points (no device needed) ----------------------------

PATH_HOST, PATH_DEVICE_EXACT, PATH_DEVICE_ORDERED = 0, 1, 2  # GE_PARTITION_PATH_*
# GE_PTAP_SORT_*
PTAP_SORT_NONE, PTAP_SORT_SINGLE, PTAP_SORT_SPLIT_WIDTH, PTAP_SORT_SPLIT_OVERRIDE = 0, 1, 2, 3


# ge_partition_census (include/ge.h), in declaration order
CENSUS_FIELDS = (
    "scan_small", "scan_mid", "scan_big", "scan_huge",
    "kept_bound", "kept_runner_up", "kept_nonpositive",
    "rescan_changed", "rescan_bound", "rescan_touched",
    "match_global_rounds", "match_lds_rounds", "match_max_candidates",
    "rebuilt_wave", "rebuilt_block", "rebuilt_global", "rebuilt_in_place", "rebuilt_moved",
    "patched", "patch_short", "patch_size", "patch_fit",
    "record_refetches", "pool_compactions", "alive_compactions")


def _take_hier(h, info):
    try:
        lv = ctypes.c_int()
        _check(lib().ge_hier_levels(h, ctypes.byref(lv)))
        out = []
        for l in range(lv.value):
            r, c = ctypes.c_int(), ctypes.c_int()
            _check(lib().ge_hier_shape(h, l, ctypes.byref(r), ctypes.byref(c)))
            pip = np.empty(r.value + 1, dtype=np.int32)
            pix = np.empty(c.value, dtype=np.int32)
            _check(lib().ge_hier_copy(h, l, pip, pix))
            out.append((pip, pix, r.value, c.value))
        if not info:
            return out
        path, rounds = ctypes.c_int(), ctypes.c_int()
        rebuilt = (ctypes.c_longlong * 3)()
        _check(lib().ge_hier_info(h, ctypes.byref(path), ctypes.byref(rounds), rebuilt))
        g = _vp()
        _check(lib().ge_hier_final_graph(h, ctypes.byref(g)))
        final_graph = _take_csr(g)
        alpha = np.empty(len(final_graph[0]) - 1, dtype=np.float64)
        _check(lib().ge_hier_final_alpha(h, alpha))
        census = (ctypes.c_longlong * len(CENSUS_FIELDS))()
        _check(lib().ge_hier_census(h, ctypes.cast(census, _vp)))
        return out, {"path": path.value, "rounds": rounds.value, "rebuilt": list(rebuilt),
                     "census": dict(zip(CENSUS_FIELDS, (int(v) for v in census))),
                     "final_graph": final_graph, "final_alpha": alpha}
    finally:
        lib().ge_hier_free(h)


def partition(A, coarsening_factor, printing=False, positive_merging=True, stall=1.0,
              matching_iterations=2, merge_leaves=False, ctx=None, info=False):
    """Hierarchy of P_T matrices as (indptr, indices, rows, cols) tuples.  With a
    Context the hierarchy is built on its device (symmetric A with finite weights:
    integers by the exact contraction, other reals by the ordered one); without
    one, or for other inputs, by the library's host path.  info=True returns
    (hierarchy, dict): path (PATH_*), rounds, rebuilt (lists rebuilt by the
    device's wave / block / global kernels), census (CENSUS_FIELDS: which kernel
    class of the device partition handled what; all zeros unless
    GE_PARTITION_CENSUS=1 is set at the call) and the quotient graph the round loop
    ended with, final_graph (CSR by the last P_T's row numbers) and final_alpha."""
    ip, ix, dx = _csr(A)
    h = _vp()
    _check(lib().ge_partition(ctx.h if ctx is not None else None, len(ip) - 1, ip, ix, dx,
                              coarsening_factor, int(printing),
                              int(positive_merging), stall, matching_iterations,
                              int(merge_leaves), ctypes.byref(h)))
    return _take_hier(h, info)


def partition_single(A, num_parts=None, printing=False, positive_merging=True, stall=1.0,
                     matching_iterations=2, merge_leaves=False, ctx=None, info=False):
    """One P_T as (indptr, indices, rows, cols): partition::partition(A, printing,
    ...) for num_parts=None, partition(A, numParts, ...) otherwise (the rounds
    also stop once at most num_parts aggregates are left).  Paths and info as in
    partition()."""
    ip, ix, dx = _csr(A)
    h = _vp()
    _check(lib().ge_partition_single(ctx.h if ctx is not None else None, len(ip) - 1, ip, ix, dx,
                                     0 if num_parts is None else int(num_parts), int(printing),
                                     int(positive_merging), stall, matching_iterations,
                                     int(merge_leaves), ctypes.byref(h)))
    res = _take_hier(h, info)
    return (res[0][0], res[1]) if info else res[0]


def interpolation_matrix(num_cols, sets):
    offs = np.zeros(len(sets) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(s) for s in sets])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in sets])
                                if sets else np.zeros(0, np.int32), dtype=np.int32)
    h = _vp()
    _check(lib().ge_interpolation_matrix(num_cols, len(sets), offs, flat, ctypes.byref(h)))
    return _take_csr(h)


def modularity(A, vertex_A, m):
    ip, ix, dx = _csr(A)
    q = ctypes.c_double()
    _check(lib().ge_modularity(len(ip) - 1, ip, ix, dx, m,
                               np.ascontiguousarray(vertex_A, dtype=np.int32), ctypes.byref(q)))
    return q.value


def radius_step(coords_A, dim, coarse_is_base, PTc=None, coords_Ac=None, r_Ac=None, Ac=None):
    """Returns (r_A, coords_A after the rescale)."""
    cA = np.array(coords_A, dtype=np.float64, copy=True).reshape(-1)
    m = cA.size // dim
    rA = np.zeros(m)
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(_vp)

    mc = 0 if PTc is None else len(PTc[0]) - 1
    _check(lib().ge_radius_step(
        m, cA, rA, dim, int(coarse_is_base), mc,
        ptr(None if PTc is None else PTc[0], np.int32), ptr(None if PTc is None else PTc[1], np.int32),
        ptr(coords_Ac, np.float64), ptr(r_Ac, np.float64),
        ptr(None if Ac is None else Ac[0], np.int32), ptr(None if Ac is None else Ac[1], np.int32)))
    return rA, cA.reshape(m, dim)


def embed_via_minimization(A, dim, coords=None, iterations=10, seed=12345):
    """partition::embedViaMinimization(A, d, coords, ITER) (src/embed.cpp:341-559);
    coords=None draws the reference's random start from mt19937(seed)."""
    ip, ix, _ = _csr(A)
    n = len(ip) - 1
    X = np.zeros((n, dim)) if coords is None else np.array(coords, dtype=np.float64)
    X = np.ascontiguousarray(X)
    _check(lib().ge_embed_via_minimization(n, ip, ix, dim, X.reshape(-1), int(coords is None),
                                           seed, iterations))
    return X


def embed_via_minimization_ml(A, PT, vertex_A, coords_A, r_A, dim, iterations=1000, ctx=None,
                              info=False):
    """anyToMultilevel(embedViaMinimization) on one level (src/embed.cpp:23-83 over
    :341-559): per aggregate of PT, `iterations` sweeps from a zero start on the
    members' internal edges, normalised and placed in the aggregate's ball.  With a
    Context the level is one batched device call; without one (or GE_MINIMIZE_HOST=1)
    the library's host path, with the same bits.  info=True also returns the classes:
    aggregates that ran packed / one wave per direction / on the host, and the path
    (0 host, 1 device)."""
    ip = np.ascontiguousarray(A[0], dtype=np.int32)
    ix = np.ascontiguousarray(A[1], dtype=np.int32)
    pip = np.ascontiguousarray(PT[0], dtype=np.int32)
    pix = np.ascontiguousarray(PT[1], dtype=np.int32)
    n, m = len(ip) - 1, len(pip) - 1
    vA = np.ascontiguousarray(vertex_A, dtype=np.int32)
    cA = np.ascontiguousarray(coords_A, dtype=np.float64).reshape(-1)
    rA = np.ascontiguousarray(r_A, dtype=np.float64).reshape(-1)
    if len(vA) != n or len(cA) != m * dim or len(rA) != m or len(pix) != n:
        raise GeError("embed_via_minimization_ml: array sizes do not match n, m and dim")
    X = np.zeros((n, dim))
    classes = (ctypes.c_int * 4)()
    _check(lib().ge_embed_via_minimization_ml(ctx.h if ctx is not None else None, n, ip, ix, m,
                                              pip, pix, vA, cA, rA, dim, iterations,
                                              X.reshape(-1), classes))
    if not info:
        return X
    return X, dict(zip(("packed", "wave", "host", "path"), classes))


def uniform_stream(seed, count):
    out = np.empty(count, dtype=np.float64)
    _check(lib().ge_uniform_stream(seed, count, out))
    return out


def rmat_csr(n, draws, seed=12345):
    h = _vp()
    _check(lib().ge_rmat_csr(n, draws, seed, ctypes.byref(h)))
    return _take_csr(h)


def largest_component(A):
    ip, ix, dx = _csr(A)
    h = _vp()
    _check(lib().ge_largest_component(len(ip) - 1, ip, ix, dx, ctypes.byref(h)))
    return _take_csr(h)


def vertex_of(PT):
    pip, pix = np.asarray(PT[0]), np.asarray(PT[1])
    v = np.empty(len(pix), dtype=np.int32)
    sizes = np.diff(pip)
    v[pix] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return v


def concat_levels(As, hier):
    a_n = np.array([len(a[0]) - 1 for a in As], dtype=np.int32)
    a_off = np.cumsum([0] + [len(a[0]) for a in As])[:-1].astype(np.int32)
    a_nz = np.cumsum([0] + [len(a[1]) for a in As])[:-1].astype(np.int32)
    a_ip = np.concatenate([np.asarray(a[0]) for a in As]).astype(np.int32)
    a_ix = np.concatenate([np.asarray(a[1]) for a in As]).astype(np.int32)
    a_dx = np.concatenate([np.asarray(a[2]) for a in As]).astype(np.float64)
    p_rows = np.array([p[2] for p in hier] + [0], dtype=np.int32)
    p_off = np.cumsum([0] + [len(p[0]) for p in hier]).astype(np.int32)
    p_nz = np.cumsum([0] + [len(p[1]) for p in hier]).astype(np.int32)
    p_ip = np.concatenate([np.asarray(p[0]) for p in hier] + [np.zeros(1)]).astype(np.int32)
    p_ix = np.concatenate([np.asarray(p[1]) for p in hier] + [np.zeros(1)]).astype(np.int32)
    return a_n, a_off, a_nz, a_ip, a_ix, a_dx, p_rows, p_off, p_nz, p_ip, p_ix


def header_symbols():
    """Function names declared in include/ge.h."""
    import re
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(ge_\w+)\s*\(", txt, re.M)))
