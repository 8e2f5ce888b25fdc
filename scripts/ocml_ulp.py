#!/usr/bin/env python3
"""Largest relative error, in units of u = 2^-53, of the device's log1p and pow(a, 0.5) in the
file scripts/micro/ocml_ulp writes, against np.longdouble (tests/energy_cases.py doubles
these figures for its LOG1P_ULP and POW_ULP)."""
import sys

import numpy as np

LD = np.longdouble
v = np.fromfile(sys.argv[1], dtype=np.float64).reshape(-1, 2)
n = len(v) // 2
for name, (x, y), ref in (("log1p", v[:n].T, lambda x: np.log1p(x)),
                          ("pow(a, 0.5)", v[n:].T, lambda x: np.sqrt(x))):
    r = ref(x.astype(LD))
    err = np.abs(y.astype(LD) - r) / np.abs(r) / LD(2.0 ** -53)
    k = int(np.argmax(err))
    print(f"{name}: {n} operands in [{x.min():g}, {x.max():g}], largest relative error "
          f"{float(err[k]):.3f} u at {float(x[k])!r}")
