"""Shared by the tests of the f32 weight mirrors (rt_layout.h RTL_MATF_SOLID_W): the flattened
material / texture tables of a scene through the probe library, the device's to_w3 on an array,
the edge values both tests use, and a host-built scene with every material kind over solid,
checker and noise textures."""
from __future__ import annotations

import ctypes as C

import numpy as np

import probe_lib as P
import surely_rt as rt

MAT_WORDS, TEX_WORDS = 20, 12           # rt_layout.h RTL_MAT_WORDS, RTL_TEX_WORDS
MATF_NEEDS_UV, MATF_SOLID_W = 0x100, 0x200
MAT_WZ = 18                             # the mirror's third word (low word of d7)
MAT_SLOTS = TEX_SLOTS = 8               # rt_mi355x.h
LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT, ISOTROPIC = 1, 2, 3, 4, 5
SOLID, CHECKER, IMAGE, NOISE = 1, 2, 3, 4

F32_MAX = float(np.finfo(np.float32).max)
F32_OVF = F32_MAX + 2.0 ** 103  # FLT_MAX + ulp/2, exact: the tie that rounds (to even) to inf
# doubles whose f32 rounding is the interesting part: signed zeros, f32 subnormals (kept, not
# flushed) and the f64 values below them, ties of round-to-nearest-even at 1, at the smallest
# normal and at the overflow threshold F32_OVF (the first double that rounds to inf), inf
# and NaN
EDGE = np.array([
    0.0, -0.0, 1.0, -1.0, 0.73, 0.65, 15.0,
    1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 2.0 ** -151, 1e-320,
    2.0 ** -126, np.nextafter(2.0 ** -126, 0.0), 2.0 ** -126 * (1 - 2.0 ** -25),
    1.0 + 2.0 ** -24, np.nextafter(1.0 + 2.0 ** -24, 2.0), 1.0 + 3 * 2.0 ** -24, 1.0 - 2.0 ** -25,
    F32_MAX, np.nextafter(F32_OVF, 0.0), F32_OVF, 1e39, -1e39,
    1.7e308, np.inf, -np.inf, np.nan,
], np.float64)


def f32_bits(x) -> np.ndarray:
    """The bits of the host cast (float)x: round to nearest even, subnormals kept."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).view(np.uint32)


def _bind():
    L = P.lib()
    L.rtp_flat_tables.restype = C.c_int
    L.rtp_flat_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rtp_to_w3_bits.restype = C.c_int
    L.rtp_to_w3_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return L


def flat_tables(blob) -> tuple[np.ndarray, np.ndarray]:
    """(materials [n, 20], textures [n, 12]) as uint32, as rt_flatten.cpp lays them out. No GPU."""
    L = _bind()
    h = blob.header()
    mats = np.zeros(h["n_materials"] * MAT_WORDS, np.uint32)
    texs = np.zeros(h["n_textures"] * TEX_WORDS, np.uint32)
    nm, nt = C.c_int(-1), C.c_int(-1)
    rc = L.rtp_flat_tables(C.cast(blob.ref(), C.c_void_p), mats.ctypes.data, mats.size,
                           texs.ctypes.data, texs.size, C.byref(nm), C.byref(nt))
    assert rc == 0, rc
    assert (nm.value, nt.value) == (mats.size, texs.size)  # record sizes unchanged
    return mats.reshape(-1, MAT_WORDS), texs.reshape(-1, TEX_WORDS)


def to_w3_bits(x) -> np.ndarray:
    """The device's to_w3 (rt_kernel.h) on each double -> the f32 result's bits. Needs a GPU."""
    a = np.ascontiguousarray(x, np.float64).ravel()
    assert a.size <= 4096
    out = np.zeros(a.size, np.float64)
    rc = _bind().rtp_to_w3_bits(a.ctypes.data, out.ctypes.data, a.size)
    assert rc == 0, f"rtp_to_w3_bits: HIP error {rc}"
    return out.astype(np.uint32)


def every_kind_scene(colors=None, seed=17):
    """Lambertian, DiffuseLight and Isotropic over a solid, a checker and a noise texture each,
    metals and dielectrics, the solid colours / albedos / tints taken three at a time from
    `colors` (default: EDGE, so subnormal, overflowing, NaN and -0.0 components occur in every
    kind). All of it is in the world, so every material is serialised. Returns the blob."""
    c = np.resize(EDGE if colors is None else np.asarray(colors, np.float64), 3 * 16).reshape(-1, 3)
    sc = rt.Scene(seed)
    k = iter(range(len(c)))
    mats = []
    for make in (sc.lambertian, sc.diffuse_light, sc.isotropic):
        mats.append(make(tuple(c[next(k)])))
        mats.append(make(tuple(c[next(k)])))
        mats.append(make(tex=sc.checker_from_color(0.8, tuple(c[next(k)]), tuple(c[next(k)]))))
        mats.append(make(tex=sc.noise_texture(3.0)))
    mats.append(sc.metal(tuple(c[next(k)]), 0.25))
    mats.append(sc.metal(tuple(c[next(k)]), 0.0))
    mats.append(sc.dielectric(1.5, tuple(c[next(k)])))
    mats.append(sc.dielectric(1.33, tuple(c[next(k)])))
    objs = [sc.sphere((1.1 * i, 0.5, 0.0), 0.5, m) for i, m in enumerate(mats)]
    lq = sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), sc.diffuse_light((7, 7, 7)))
    return sc.serialize(sc.hittable_list(*objs, lq), sc.hittable_list(lq))
