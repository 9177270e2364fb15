"""ctypes wrapper of the device-primitive probe (csrc/probe/rt_probe.hip, build/librtprobe.so).
TEST INFRASTRUCTURE ONLY: one C function per inline device function of rt_kernel.h / rt_rng.h,
so a GPU test can run the product's own primitive on arrays and compare it with a reference.

Every probe takes n records of IN doubles and returns n records of OUT doubles (integers,
booleans and f32 values cross as f64, exactly). Loading the library needs no GPU; calling a
probe does.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
PROBE_SO = REPO / "build" / "librtprobe.so"

# name -> (doubles per input record, doubles per output record); rt_probe.hip PROBE(name, IN, OUT)
PROBES = {
    "rcp_nr": (1, 1), "div_nr": (2, 1), "rsq_nr": (1, 1), "sqrt_nr": (1, 1), "rcp_w": (1, 1),
    "rcp_wt": (1, 1), "rsq_wt": (1, 1),
    "sincos2pi": (1, 2), "log_u01": (1, 1), "pow5_cr": (1, 1), "f2i_sat": (1, 1), "f2u_sat": (1, 1),
    "rng_stream": (4, 22), "rng_draws": (5, 3),
    "random_cosine_direction": (4, 5), "random_unit_vector": (4, 5),
    "sphere_test_v": (13, 5), "aquad_test": (16, 4), "quad_test": (28, 2), "aabb_hit": (14, 2),
    "rotate_y_in": (8, 6), "rotate_y_out": (8, 6), "reflect": (6, 3), "refract": (7, 3),
    "unit_vector": (3, 3), "onb_local": (12, 3),
    "sphere_uv_f": (3, 2), "quad_light_w": (8, 1), "sphere_light_w": (1, 1),
    "perlin_turb": (3, 1),  # plus the table bytes
}
PERLIN_BYTES = 4096 + 768  # rt_layout.h RTL_PERLIN_BYTES

_lib = None


def symbols() -> list[str]:
    return [f"rtp_{n}" for n in PROBES]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not PROBE_SO.exists():
            subprocess.run(["make", "-C", str(REPO), "probe"], check=True)
        L = C.CDLL(str(PROBE_SO))
        for name in PROBES:
            f = getattr(L, f"rtp_{name}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rtp_perlin_turb.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _lib = L
    return _lib


def _records(name, x):
    n_in, n_out = PROBES[name]
    a = np.ascontiguousarray(x, np.float64).reshape(-1, n_in)
    return a, np.zeros((a.shape[0], n_out), np.float64)


def run(name: str, x) -> np.ndarray:
    """probe `name` on the records x (any shape with n * IN elements) -> [n, OUT] float64."""
    a, out = _records(name, x)
    rc = getattr(lib(), f"rtp_{name}")(a.ctypes.data, out.ctypes.data, a.shape[0])
    if rc != 0:
        raise RuntimeError(f"rtp_{name}: HIP error {rc}")
    return out


def perlin_turb(table: np.ndarray, points) -> np.ndarray:
    t = np.ascontiguousarray(table, np.uint8)
    assert t.size == PERLIN_BYTES
    a, out = _records("perlin_turb", points)
    rc = lib().rtp_perlin_turb(t.ctypes.data, a.ctypes.data, out.ctypes.data, a.shape[0])
    if rc != 0:
        raise RuntimeError(f"rtp_perlin_turb: HIP error {rc}")
    return out[:, 0]
