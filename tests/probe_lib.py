"""ctypes wrapper of the device probes (csrc/probe/rt_probe.hip and rt_probe_scene.hip,
build/librtprobe.so). TEST INFRASTRUCTURE ONLY: one C function per inline device function of
rt_kernel.h / rt_rng.h, so a GPU test can run the product's own primitive on arrays and compare
it with a reference, and one per scene-level function (traverse, frame_ray / frame_out,
volume_two_hits, light_pdf, tex_value), which take a serialised scene as well.

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
    "rcp_nr": (1, 1), "rcp_nr1": (1, 1), "div_nr": (2, 1), "rsq_nr": (1, 1), "sqrt_nr": (1, 1), "rcp_w": (1, 1),
    "rcp_wt": (1, 1), "rsq_wt": (1, 1),
    "sincos2pi": (1, 2), "log_u01": (1, 1), "pow5_cr": (1, 1), "f2i_sat": (1, 1), "f2u_sat": (1, 1),
    "rng_stream": (4, 22), "rng_draws": (5, 3),
    "random_cosine_direction": (4, 5), "random_unit_vector": (4, 5),
    "sphere_test_v": (13, 5), "aquad_test": (16, 4),
    "aquad_test_nr1": (16, 4), "quad_test": (28, 2), "aabb_hit": (14, 2),
    "rotate_y_in": (8, 6), "rotate_y_out": (8, 6), "reflect": (6, 3), "refract": (7, 3),
    "unit_vector": (3, 3), "onb_local": (12, 3),
    "sphere_uv_f": (3, 2), "quad_light_w": (8, 1), "sphere_light_w": (1, 1),
    "perlin_turb": (3, 1),  # plus the table bytes
}
PERLIN_BYTES = 4096 + 768  # rt_layout.h RTL_PERLIN_BYTES
# rt_probe_scene.hip SCENE_PROBE(name, IN, OUT): these take the scene blob first
SCENE_PROBES = {
    "world_hit": (13, 14), "frame": (13, 12), "volume_bounds": (7, 8),  # volume_bounds: plus the node
    "light_pdf": (7, 2), "tex_value": (6, 6),
    "world_hit_bvh": (13, 14), "bvh_walks": (9, 22),  # bvh_walks: plus the node
}
NODE_PROBES = ("volume_bounds", "bvh_walks")  # these take a record's word offset after the blob
# refusals of the scene probes (negative; a positive code is a HIP error): rt_probe_scene.hip
ERR_ARG, ERR_BVH, ERR_NESTED, ERR_RECORD = -100, -101, -102, -103
# rt_layout.h record types, as scene_records reports them
RTL_END, RTL_QUAD, RTL_SPHERE, RTL_BVH, RTL_TRANSLATE, RTL_ROTATE_Y, RTL_EXIT, RTL_VOLUME, RTL_QUADS, RTL_DUP = (
    0, 1, 2, 3, 4, 5, 6, 7, 9, 10)
RTL_XFORM_LONG = 1  # header flag bits as scene_records reports them (header word 0 >> 8)
RTL_VOLF_SPHERE, RTL_VOLF_QUADS = 1, 2

_lib = None


def symbols() -> list[str]:
    return [f"rtp_{n}" for n in list(PROBES) + list(SCENE_PROBES)] + ["rtp_scene_records"]


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
        for name in SCENE_PROBES:
            f = getattr(L, f"rtp_{name}")
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        for name in NODE_PROBES:
            getattr(L, f"rtp_{name}").argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.rtp_scene_records.restype = C.c_int
        L.rtp_scene_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rtp_scene_header.restype = C.c_int
        L.rtp_scene_header.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
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


class ProbeRefused(RuntimeError):
    """A scene probe refused its input on the host (nothing was launched)."""

    def __init__(self, name, code):
        super().__init__(f"rtp_{name}: refused with {code}")
        self.code = code


def _scene_call(name, blob, x, *lead):
    n_in, n_out = SCENE_PROBES[name]
    a = np.ascontiguousarray(x, np.float64).reshape(-1, n_in)
    out = np.zeros((a.shape[0], n_out), np.float64)
    rc = getattr(lib(), f"rtp_{name}")(C.cast(blob.ref(), C.c_void_p), *lead, a.ctypes.data,
                                         out.ctypes.data, a.shape[0])
    if rc < 0:
        raise ProbeRefused(name, rc)
    if rc != 0:
        raise RuntimeError(f"rtp_{name}: HIP error {rc}")
    return out


def scene_run(name: str, blob, x) -> np.ndarray:
    """scene probe `name` of the serialised scene `blob` on the records x -> [n, OUT] float64."""
    assert name not in NODE_PROBES
    return _scene_call(name, blob, x)


def volume_bounds(blob, node: int, rays7) -> np.ndarray:
    """volume_two_hits and the two boundary passes for the top-level VOLUME record at `node`."""
    return _scene_call("volume_bounds", blob, rays7, int(node))


def bvh_walks(blob, node: int, rays9) -> np.ndarray:
    """cbvh_walk, obvh_walk and the reference-order traverse of the top-level BVH subtree root at
    `node` on the records (o3, d3, time, tmin, tmax) -> [n, 22]: with MAIN = true, then with MAIN =
    false (hit node -1): [hit, t, hit node, tie flag] of the LDS walk, of the streams walk, then
    [hit, t, hit node] of the reference-order walk."""
    return _scene_call("bvh_walks", blob, rays9, int(node))


def scene_records(blob) -> np.ndarray:
    """The flattened world's records in memory order -> [n, 5] int64: word, type, header word 0 >> 8,
    word 2, enclosing frame. A BVH record (they come first) has its ordered BVH's word offset (0 =
    none) in column 3 and as its frame the one the top-level walk reaches it in, -2 for a node that
    walk does not reach (inside a subtree or a boundary). Needs no GPU."""
    cap = 4096
    out = np.zeros((cap, 5), np.float64)
    n = lib().rtp_scene_records(C.cast(blob.ref(), C.c_void_p), out.ctypes.data, cap)
    if n < 0:
        raise ProbeRefused("scene_records", n)
    assert n <= cap
    return out[:n].astype(np.int64)


# rt_layout.h rtl_scene_header, word by word
SCENE_HEADER = ("root", "n_node_words", "n_mats", "n_texs", "n_perlins", "n_lights", "lights_is_list",
                "has_bvh", "has_volume", "max_chain", "n_texel_bytes", "pdf_materials",
                "has_textures", "bvh_words", "volume_in_bvh", "volumes_one_walk_spheres",
                "has_isotropic", "n_rec_words", "lights_nested", "nested_volumes", "cbvh_word0",
                "cbvh_words", "cbvh_stack")


def scene_header(blob) -> dict:
    """The rtl_scene_header the product's flattener gives the scene (any scene it takes, nested
    volumes included) -> {field: int}. Needs no GPU."""
    out = np.zeros(len(SCENE_HEADER), np.uint32)
    n = lib().rtp_scene_header(C.cast(blob.ref(), C.c_void_p), out.ctypes.data, out.size)
    if n < 0:
        raise ProbeRefused("scene_header", n)
    assert n == len(SCENE_HEADER), f"rtl_scene_header has {n} words, SCENE_HEADER {len(SCENE_HEADER)}"
    return {k: int(v) for k, v in zip(SCENE_HEADER, out)}
