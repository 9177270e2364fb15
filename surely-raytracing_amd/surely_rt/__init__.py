"""surely_rt — Python host over the two C ABIs of this repository.

* ``include/rt_host.h``   -> ``build/librthost.so``  : the scene-construction API of the
  reference (Quad, Sphere, make_box, RotateY, Translate, ConstantMedium, HittableList,
  create_bvh, Lambertian, Metal, Dielectric, DiffuseLight, Isotropic, textures, Camera::new,
  write_color) restated in C++ and serialised into the flat scene blob.
* ``include/rt_mi355x.h`` -> ``build/librtmi355x.so`` : the gfx950 render loop behind
  ``rt_render`` (the drop-in for render_par_lights, /root/reference/src/render.rs:144-216).

Nothing here computes pixels: the render path is the HIP library, and it fails loudly (raises)
when that library or a GPU is missing — there is no CPU fallback in the product.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent
REPO = PKG_DIR.parent
BUILD = Path(os.environ.get("RT_BUILD_DIR", REPO / "build"))

# ---------------------------------------------------------------------------- ABI structs
RT_OK = 0
RT_ERR_INVALID_ARG = -1
RT_ERR_BAD_BLOB = -2
RT_ERR_UNSUPPORTED = -3
RT_ERR_EMPTY_LIGHTS = -4
RT_ERR_HIP = -5
RT_ERR_NO_DEVICE = -6

RT_FLAG_OVERWRITE = 0x1
RT_FLAG_COUNT_OPS = 0x2
# exact reference semantics: empty lights -> error, Isotropic scattering_pdf = 0 (S1 / S2).
# S9: a path whose throughput is exactly zero in all channels and that carries no special value
# ends with radiance 0; the reference goes on and returns NaN if a later bounce has a zero or NaN
# pdf; RT_FLAG_SEMANTICS_REFERENCE keeps the reference's behaviour.
RT_FLAG_SEMANTICS_REFERENCE = 0x4
RT_FLAG_INTERPRETER = 0x8  # product render with the interpreter walker (no scene-specialised kernel)
RT_FLAG_REFERENCE_BVH = 0x10  # product render walks BVH subtrees in the reference tree and order

# first-hit AOV pass (include/rt_mi355x.h RT_AOV_*): channels per pixel and their offsets
AOV_CHANNELS = 12
AOV_HITS, AOV_T, AOV_NORMAL, AOV_ALBEDO, AOV_EMISSION, AOV_MATID = 0, 1, 2, 5, 8, 11
AOV_NAMES = ("hits", "t", "nx", "ny", "nz", "albedo_r", "albedo_g", "albedo_b",
             "emission_r", "emission_g", "emission_b", "matid")

# edge-avoiding a-trous denoiser (include/rt_mi355x.h RT_DENOISE_*)
DENOISE_MAX_LEVELS = 8
DENOISE_DEMODULATE = 0x1  # filter (beauty - emission) / max(albedo, 1e-3), re-modulate after

# device output stage (rt_output*)
RT_OUTPUT_EXPOSURE = 0x1  # x = 1 - E^(-exposure * x) before the gamma
RT_OUTPUT_AUTO_EXPOSE = 0x2  # exposure = auto_expose(frame), computed on the device
RT_OUTPUT_RGBA = 0x4  # 4 bytes per pixel, alpha 255; else 3

# temporal accumulation (rt_temporal_*)
RT_TEMPORAL_RESET = 0x1  # discard the history before the call
RT_TEMPORAL_VARIANCE_OF_MEAN = 0x2  # out_m2 in the scale of the accumulated mean's variance

OP_NAMES = [
    "samples", "world_queries", "quad_tests", "quad_plane", "quad_interval", "quad_hits",
    "sphere_tests", "sphere_roots", "sphere_hits", "aabb_tests", "translate", "rotate_y",
    "volume_tests", "volume_draws", "misses", "emissive_hits", "lambertian", "metal",
    "dielectric", "isotropic", "light_pdf_quad", "light_pdf_sphere", "light_gen", "cosine_gen",
    "noise_evals", "depth_cutoff",
]


class RtSceneBlob(C.Structure):
    _fields_ = [("slots", C.POINTER(C.c_uint64)), ("n_slots", C.c_uint64),
                ("texels", C.POINTER(C.c_uint8)), ("n_texels", C.c_uint64)]


class RtCamera(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32),
                ("samples_per_pixel", C.c_int32), ("sqrt_spp", C.c_int32),
                ("max_depth", C.c_int32), ("_pad0", C.c_int32),
                ("recip_sqrt_spp", C.c_double), ("center", C.c_double * 3),
                ("pixel00_loc", C.c_double * 3), ("pixel_delta_u", C.c_double * 3),
                ("pixel_delta_v", C.c_double * 3), ("defocus_angle", C.c_double),
                ("defocus_disk_u", C.c_double * 3), ("defocus_disk_v", C.c_double * 3),
                ("background", C.c_double * 3)]

    def copy(self) -> "RtCamera":
        c = RtCamera()
        C.pointer(c)[0] = self
        return c


class RtRenderOpts(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("row_begin", C.c_int32), ("row_step", C.c_int32),
                ("n_rows", C.c_int32), ("flags", C.c_uint32), ("sj_begin", C.c_int32),
                ("sj_count", C.c_int32), ("device", C.c_int32), ("_pad0", C.c_int32)]


class RtStats(C.Structure):
    _fields_ = [("ms_kernel", C.c_double), ("ms_total", C.c_double), ("samples", C.c_uint64),
                ("ops", C.c_uint64 * 32), ("out_bytes", C.c_uint64), ("launches", C.c_uint32),
                ("_pad0", C.c_uint32)]

    def op_counts(self) -> dict:
        return {n: int(self.ops[i]) for i, n in enumerate(OP_NAMES)}


class RtDenoiseParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32),
                ("flags", C.c_uint32), ("beauty_samples", C.c_double),
                ("aov_samples", C.c_double), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float)]


class RtDenoiseVarParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32),
                ("flags", C.c_uint32), ("beauty_samples", C.c_double),
                ("aov_samples", C.c_double), ("beauty_rows", C.c_int32), ("_pad0", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float)]


class RtAdaptiveParams(C.Structure):
    _fields_ = [("passes", C.c_int32), ("min_passes", C.c_int32), ("threshold", C.c_double),
                ("floor", C.c_double)]


class RtOutputParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_uint32),
                ("_pad0", C.c_int32), ("samples_per_pixel", C.c_double),
                ("exposure", C.c_double)]


class RtTemporalParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_uint32),
                ("beauty_rows", C.c_int32), ("max_history", C.c_float), ("depth_tol", C.c_float),
                ("normal_tol", C.c_float), ("min_weight", C.c_float)]


class RtRay(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("dir", C.c_double * 3), ("time", C.c_double),
                ("tmin", C.c_double), ("tmax", C.c_double), ("pixel", C.c_uint32),
                ("sample", C.c_uint32)]


class RtHit(C.Structure):
    _fields_ = [("t", C.c_double), ("distance", C.c_double), ("p", C.c_double * 3),
                ("normal", C.c_double * 3), ("hit", C.c_int32), ("front_face", C.c_int32),
                ("material", C.c_int32), ("prim", C.c_int32)]


class RtQueryParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("flags", C.c_uint32), ("mode", C.c_uint32)]


class RtRaysParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("flags", C.c_uint32), ("mode", C.c_uint32),
                ("sqrt_paths", C.c_int32), ("max_depth", C.c_int32),
                ("stream_skip", C.c_uint32), ("_pad0", C.c_uint32),
                ("background", C.c_double * 3)]


class RthAoParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("radius", C.c_double), ("tmin", C.c_double),
                ("dir_index", C.c_uint32), ("_pad0", C.c_uint32)]


class RthProjection(C.Structure):
    _fields_ = [("kind", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("sqrt_spp", C.c_int32), ("origin", C.c_double * 3),
                ("forward", C.c_double * 3), ("up", C.c_double * 3), ("fov", C.c_double)]


class RtProjection(C.Structure):  # the layout of RthProjection
    _fields_ = [("kind", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("sqrt_spp", C.c_int32), ("origin", C.c_double * 3),
                ("forward", C.c_double * 3), ("up", C.c_double * 3), ("fov", C.c_double)]


class RtAoParams(C.Structure):  # the layout of RthAoParams
    _fields_ = [("seed", C.c_uint64), ("radius", C.c_double), ("tmin", C.c_double),
                ("dir_index", C.c_uint32), ("_pad0", C.c_uint32)]


class RtAoFrameParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("radius", C.c_double), ("tmin", C.c_double),
                ("directions", C.c_uint32), ("flags", C.c_uint32), ("channels", C.c_uint32),
                ("chunk_rays", C.c_uint32)]


# ray renders (rt_render_rays*)
RT_RAYS_STREAM_TIME = 0x1  # a path's time is the last skipped draw, not ray.time
RT_RAYS_MAX_SKIP = 16
# host ray generator (rt_host.h rth_projection_rays)
RTH_PROJ_PINHOLE, RTH_PROJ_ORTHO, RTH_PROJ_PANORAMA, RTH_PROJ_FISHEYE = 0, 1, 2, 3
# device ray generator (rt_projection_rays_device): the same values
RT_PROJ_PINHOLE, RT_PROJ_ORTHO, RT_PROJ_PANORAMA, RT_PROJ_FISHEYE = 0, 1, 2, 3
PROJECTIONS = {"pinhole": RTH_PROJ_PINHOLE, "ortho": RTH_PROJ_ORTHO,
               "panorama": RTH_PROJ_PANORAMA, "fisheye": RTH_PROJ_FISHEYE}

# ray queries (rt_query_rays*): numpy views of rt_ray / rt_hit, 80 bytes each
RT_QUERY_OCCLUSION = 0x1  # out is one uint8 per ray: 1 hit, 0 miss, 255 invalid
RT_QUERY_ANY_HIT = 0x2  # with RT_QUERY_OCCLUSION only: the same bytes, the walk leaves at its first accept
RAY_DTYPE = np.dtype([("origin", "<f8", 3), ("dir", "<f8", 3), ("time", "<f8"), ("tmin", "<f8"),
                      ("tmax", "<f8"), ("pixel", "<u4"), ("sample", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("distance", "<f8"), ("p", "<f8", 3), ("normal", "<f8", 3),
                      ("hit", "<i4"), ("front_face", "<i4"), ("material", "<i4"), ("prim", "<i4")])


def make_rays(origins, dirs, time=0.0, tmin=1e-4, tmax=float("inf"), pixel=None,
              sample=0) -> np.ndarray:
    """A RAY_DTYPE array from (n, 3) origins and directions; the other fields broadcast. `pixel`
    defaults to the ray's index, so every ray draws from its own random stream."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"] = o
    rays["dir"] = np.asarray(dirs, np.float64).reshape(-1, 3)
    rays["time"], rays["tmin"], rays["tmax"] = time, tmin, tmax
    rays["pixel"] = np.arange(len(o), dtype=np.uint32) if pixel is None else pixel
    rays["sample"] = sample
    return rays


def make_rays_params(seed: int = 1, sqrt_paths: int = 1, max_depth: int = 50,
                     background=(0.0, 0.0, 0.0), flags: int = RT_FLAG_OVERWRITE,
                     stream_skip: int = 0, stream_time: bool = False) -> RtRaysParams:
    """rt_rays_params. stream_skip=3 with stream_time=True renders rays exactly as the camera ray
    of the same (pixel, sample) key is rendered (projection_rays makes such rays)."""
    rp = RtRaysParams()
    rp.seed, rp.flags, rp.mode = seed, flags, RT_RAYS_STREAM_TIME if stream_time else 0
    rp.sqrt_paths, rp.max_depth, rp.stream_skip = sqrt_paths, max_depth, stream_skip
    rp.background = _D3(*[float(x) for x in background])
    return rp


def projection_rays(kind, seed: int = 1, s_i: int = 0, s_j: int = 0, cam: "RtCamera | None" = None,
                    width: int = 0, height: int = 0, sqrt_spp: int = 1, origin=(0.0, 0.0, 0.0),
                    forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov: float = 0.0) -> np.ndarray:
    """rth_projection_rays: the RAY_DTYPE rays [height * width] of one stratum (s_i, s_j) of a
    frame. kind: "pinhole" (cam's own rays without its lens), "ortho" (fov = height of the view
    volume), "panorama" (equirectangular) or "fisheye" (equidistant, fov = full angle in degrees).
    Render them with make_rays_params(stream_skip=3, stream_time=True)."""
    pr = RthProjection()
    pr.kind = PROJECTIONS[kind] if isinstance(kind, str) else int(kind)
    pr.width, pr.height, pr.sqrt_spp, pr.fov = width, height, sqrt_spp, fov
    pr.origin, pr.forward, pr.up = _d3(origin), _d3(forward), _d3(up)
    if pr.kind == RTH_PROJ_PINHOLE and cam is not None:
        width, height = cam.image_width, cam.image_height
    rays = np.zeros(max(0, width) * max(0, height), RAY_DTYPE)
    _check_host(host_lib().rth_projection_rays(C.byref(pr), C.byref(cam) if cam is not None else None,
                                               seed, s_i, s_j, rays.ctypes.data))
    return rays


def ao_rays(rays: np.ndarray, hits: np.ndarray, k: int, seed: int = 1, radius: float = float("inf"),
            tmin: float = 1e-4) -> np.ndarray:
    """rth_ao_rays: the k-th ambient-occlusion batch for primary `rays` (RAY_DTYPE) and their
    records `hits` (HIT_DTYPE, DeviceScene.query): per hit a cosine-distributed direction about the
    normal over [tmin, radius], per non-hit an invalid ray. Query it with occlusion=True,
    any_hit=True; a pixel's ambient occlusion is the share of 0 bytes over K batches."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    if len(rays) != len(hits):
        raise ValueError("ao_rays: rays and hits differ in length")
    out = np.zeros(len(rays), RAY_DTYPE)
    if not len(rays):
        return out
    ap = RthAoParams(seed, radius, tmin, k, 0)
    _check_host(host_lib().rth_ao_rays(rays.ctypes.data, hits.ctypes.data, len(rays), C.byref(ap),
                                       out.ctypes.data))
    return out


def _query_mode(occlusion: bool, any_hit: bool) -> int:
    return (RT_QUERY_OCCLUSION if occlusion else 0) | (RT_QUERY_ANY_HIT if any_hit else 0)


class RtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rt error {code}: {msg}")
        self.code = code


# ---------------------------------------------------------------------------- library loading
_host = None
_dev = None

_D3 = C.c_double * 3


def _d3(v) -> "C.Array":
    return _D3(*[float(x) for x in v])


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        path = BUILD / "librthost.so"
        if not path.exists():
            raise RuntimeError(f"{path} missing: run `make host` (or __graft_entry__.build())")
        lib = C.CDLL(str(path))
        i32, f64, p = C.c_int32, C.c_double, C.c_void_p
        dp = C.POINTER(C.c_double)
        sig = {
            "rth_last_error": (C.c_char_p, []),
            "rth_scene_new": (p, [C.c_uint64]),
            "rth_scene_free": (None, [p]),
            "rth_random_double": (f64, [p]),
            "rth_random_range": (f64, [p, f64, f64]),
            "rth_random_int": (C.c_int64, [p, C.c_int64, C.c_int64]),
            "rth_solid_color": (i32, [p, f64, f64, f64]),
            "rth_checker_texture": (i32, [p, f64, i32, i32]),
            "rth_noise_texture": (i32, [p, f64]),
            "rth_image_texture": (i32, [p, i32, i32, C.c_void_p]),
            "rth_lambertian": (i32, [p, f64, f64, f64]),
            "rth_lambertian_tex": (i32, [p, i32]),
            "rth_metal": (i32, [p, f64, f64, f64, f64]),
            "rth_dielectric": (i32, [p, f64, f64, f64, f64]),
            "rth_diffuse_light": (i32, [p, f64, f64, f64]),
            "rth_diffuse_light_tex": (i32, [p, i32]),
            "rth_isotropic": (i32, [p, f64, f64, f64]),
            "rth_isotropic_tex": (i32, [p, i32]),
            "rth_sphere": (i32, [p, dp, f64, i32]),
            "rth_sphere_moving": (i32, [p, dp, dp, f64, i32]),
            "rth_quad": (i32, [p, dp, dp, dp, i32]),
            "rth_make_box": (i32, [p, dp, dp, i32]),
            "rth_list_new": (i32, [p]),
            "rth_list_add": (i32, [p, i32, i32]),
            "rth_list_create_bvh": (i32, [p, i32]),
            "rth_list_len": (i32, [p, i32]),
            "rth_translate": (i32, [p, i32, dp]),
            "rth_rotate_y": (i32, [p, i32, f64]),
            "rth_constant_medium": (i32, [p, i32, f64, f64, f64, f64]),
            "rth_constant_medium_tex": (i32, [p, i32, f64, i32]),
            "rth_object_bbox": (C.c_int, [p, i32, dp]),
            "rth_serialize": (C.c_int, [p, i32, i32, C.POINTER(RtSceneBlob)]),
            "rth_camera_new": (C.c_int, [f64, i32, i32, i32, f64, dp, dp, dp, f64, f64, dp,
                                         C.POINTER(RtCamera)]),
            "rth_camera_orbit_y": (C.c_int, [C.POINTER(RtCamera), dp, f64, C.POINTER(RtCamera)]),
            "rth_preset": (C.c_int, [p, C.c_char_p, C.c_char_p, i32, i32, i32, f64,
                                     C.POINTER(i32), C.POINTER(i32), C.POINTER(RtCamera)]),
            "rth_auto_expose": (f64, [C.c_void_p, C.c_int64, i32]),
            "rth_write_color": (C.c_int, [C.c_void_p, C.c_int64, f64, C.c_int, f64, C.c_void_p]),
            "rth_write_ppm": (C.c_int, [C.c_char_p, C.c_void_p, i32, i32]),
            "rth_projection_rays": (C.c_int, [C.POINTER(RthProjection), C.POINTER(RtCamera),
                                              C.c_uint64, i32, i32, C.c_void_p]),
            "rth_ao_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RthAoParams),
                                      C.c_void_p]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _host = lib
    return _host


def device_lib() -> C.CDLL:
    """The product library. Raises if it is not built: there is no CPU fallback."""
    global _dev
    if _dev is None:
        _dev = load_device_lib(BUILD / "librtmi355x.so")
    return _dev


def load_device_lib(path: Path) -> C.CDLL:
    path = Path(path)
    if not path.exists():
        raise RuntimeError(f"{path} missing: the HIP library is required (run `make device`)")
    lib = C.CDLL(str(path))
    p = C.c_void_p
    sig = {
        "rt_abi_version": (C.c_int, []),
        "rt_last_error": (C.c_char_p, []),
        "rt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "rt_scene_validate": (C.c_int, [C.POINTER(RtSceneBlob)]),
        "rt_scene_create": (C.c_int, [C.POINTER(RtSceneBlob), C.c_int, C.POINTER(p)]),
        "rt_scene_destroy": (None, [p]),
        "rt_scene_device_bytes": (C.c_uint64, [p]),
        "rt_render": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_void_p,
                                C.POINTER(RtStats)]),
        "rt_render_device": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                       C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_aov": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_void_p,
                                    C.POINTER(RtStats)]),
        "rt_render_aov_device": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                           C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_denoise_default_params": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double,
                                                C.POINTER(RtDenoiseParams)]),
        "rt_denoiser_create": (C.c_int, [C.c_int, C.POINTER(p)]),
        "rt_denoiser_destroy": (None, [p]),
        "rt_denoise_device": (C.c_int, [p, C.POINTER(RtDenoiseParams), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_denoise": (C.c_int, [p, C.POINTER(RtDenoiseParams), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_moments": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                        C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_moments_device": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                               C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(RtStats)]),
        "rt_denoise_var_default_params": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int,
                                                    C.c_double, C.POINTER(RtDenoiseVarParams)]),
        "rt_denoise_var_device": (C.c_int, [p, C.POINTER(RtDenoiseVarParams), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(RtStats)]),
        "rt_denoise_var": (C.c_int, [p, C.POINTER(RtDenoiseVarParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_tiles_device": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                             C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_adaptive_schedule": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "rt_adaptive_create": (C.c_int, [C.c_int, C.POINTER(p)]),
        "rt_adaptive_destroy": (None, [p]),
        "rt_adaptive_tile_error": (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_uint64), C.c_void_p]),
        "rt_adaptive_resolve_device": (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_render_adaptive_device": (C.c_int, [p, p, C.POINTER(RtCamera),
                                                C.POINTER(RtRenderOpts),
                                                C.POINTER(RtAdaptiveParams), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_adaptive": (C.c_int, [p, p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                         C.POINTER(RtAdaptiveParams), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(RtStats)]),
        "rt_output_create": (C.c_int, [C.c_int, C.POINTER(p)]),
        "rt_output_destroy": (None, [p]),
        "rt_output_device": (C.c_int, [p, C.POINTER(RtOutputParams), C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_double), C.c_void_p, C.POINTER(RtStats)]),
        "rt_output": (C.c_int, [p, C.POINTER(RtOutputParams), C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_double), C.POINTER(RtStats)]),
        "rt_temporal_default_params": (C.c_int, [C.c_int, C.c_int, C.POINTER(RtTemporalParams)]),
        "rt_temporal_create": (C.c_int, [C.c_int, C.POINTER(p)]),
        "rt_temporal_destroy": (None, [p]),
        "rt_temporal_info": (C.c_int, [p, C.POINTER(C.c_uint64), C.c_int]),
        "rt_temporal_accumulate_device": (C.c_int, [p, C.POINTER(RtTemporalParams),
                                                    C.POINTER(RtCamera), C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_temporal_accumulate": (C.c_int, [p, C.POINTER(RtTemporalParams), C.POINTER(RtCamera),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_blob": (C.c_int, [C.POINTER(RtSceneBlob), C.POINTER(RtCamera),
                                     C.POINTER(RtRenderOpts), C.c_void_p,
                                     C.POINTER(RtStats)]),
        "rt_scene_layout_stats": (C.c_int, [C.POINTER(RtSceneBlob), C.POINTER(C.c_uint32),
                                            C.c_int]),
        "rt_scene_prof_counters": (C.c_int, [p, C.POINTER(C.c_uint64), C.c_int]),
        "rt_render_multi": (C.c_int, [C.POINTER(RtSceneBlob), C.POINTER(RtCamera),
                                      C.POINTER(RtRenderOpts), C.POINTER(C.c_int), C.c_int,
                                      C.c_void_p, C.POINTER(RtStats)]),
        "rt_scene_trace_ms": (C.c_int, [p, C.POINTER(C.c_float), C.c_int,
                                        C.POINTER(C.c_int)]),
        "rt_scene_jit_info": (C.c_int, [p, C.POINTER(C.c_int), C.c_char_p, C.c_uint32]),
        "rt_multi_create": (C.c_int, [C.POINTER(RtSceneBlob), C.POINTER(C.c_int), C.c_int,
                                      C.POINTER(p)]),
        "rt_multi_render": (C.c_int, [p, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_void_p,
                                      C.c_void_p, C.POINTER(RtStats)]),
        "rt_multi_info": (C.c_int, [p, C.POINTER(C.c_uint64), C.c_int]),
        "rt_multi_destroy": (None, [p]),
        "rt_jit_check": (C.c_int, [C.POINTER(RtSceneBlob), C.c_char_p, C.POINTER(C.c_int),
                                   C.c_char_p, C.c_uint32]),
        "rt_scene_lds_check": (C.c_int, [C.POINTER(RtSceneBlob), C.c_uint32, C.c_uint32,
                                         C.c_uint64, C.POINTER(C.c_uint64), C.c_int, C.c_char_p,
                                         C.c_uint32]),
        "rt_query_rays_device": (C.c_int, [p, C.POINTER(RtQueryParams), C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_query_rays": (C.c_int, [p, C.POINTER(RtQueryParams), C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.POINTER(RtStats)]),
        "rt_scene_prim_map": (C.c_int, [C.POINTER(RtSceneBlob), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_uint32,
                                        C.POINTER(C.c_uint32)]),
        "rt_render_rays_device": (C.c_int, [p, C.POINTER(RtRaysParams), C.c_void_p, C.c_uint64,
                                            C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_render_rays": (C.c_int, [p, C.POINTER(RtRaysParams), C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.POINTER(RtStats)]),
        "rt_raygen_create": (C.c_int, [C.c_int, C.POINTER(p)]),
        "rt_raygen_destroy": (None, [p]),
        "rt_projection_rays_device": (C.c_int, [p, C.POINTER(RtProjection), C.POINTER(RtCamera),
                                                C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_void_p, C.c_void_p,
                                                C.POINTER(RtStats)]),
        "rt_ao_rays_device": (C.c_int, [p, C.POINTER(RtAoParams), C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_ao_accumulate_device": (C.c_int, [p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.POINTER(RtStats)]),
        "rt_ambient_occlusion_device": (C.c_int, [p, p, C.POINTER(RtAoFrameParams), C.c_void_p,
                                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(RtStats)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.rt_abi_version() != 3:
        raise RuntimeError("librtmi355x ABI version mismatch")
    return lib


def _check_host(rc: int) -> int:
    if rc < 0:
        raise RtError(rc, host_lib().rth_last_error().decode())
    return rc


def _check_dev(rc: int) -> int:
    if rc != RT_OK:
        raise RtError(rc, device_lib().rt_last_error().decode())
    return rc


# ---------------------------------------------------------------------------- scene blob
class Blob:
    """Owns a copy of the serialised scene (rt_scene_blob) and exposes the C view."""

    def __init__(self, slots: np.ndarray, texels: np.ndarray):
        self.slots = np.ascontiguousarray(slots, dtype=np.uint64)
        self.texels = np.ascontiguousarray(texels, dtype=np.uint8)
        self._c = RtSceneBlob()
        self._c.slots = self.slots.ctypes.data_as(C.POINTER(C.c_uint64))
        self._c.n_slots = self.slots.size
        self._c.texels = (self.texels.ctypes.data_as(C.POINTER(C.c_uint8))
                          if self.texels.size else C.POINTER(C.c_uint8)())
        self._c.n_texels = self.texels.size

    @property
    def c(self) -> RtSceneBlob:
        return self._c

    def ref(self):
        return C.byref(self._c)

    def header(self) -> dict:
        s = self.slots
        return dict(n_slots=int(s[2]), n_textures=int(s[3]), n_materials=int(s[5]),
                    n_perlin=int(s[7]), world_off=int(s[9]),
                    lights_off=int(np.int64(s[10].view(np.int64))))


class Scene:
    """Reference-named scene construction (main.rs vocabulary) over librthost.

    Ids returned are handles: textures, materials and objects live in separate id spaces.
    """

    def __init__(self, build_seed: int = 1):
        self._lib = host_lib()
        self._h = self._lib.rth_scene_new(C.c_uint64(build_seed))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.rth_scene_free(h)

    # utils.rs
    def random_double(self) -> float:
        return self._lib.rth_random_double(self._h)

    def random_range(self, a: float, b: float) -> float:
        return self._lib.rth_random_range(self._h, a, b)

    def random_int(self, a: int, b: int) -> int:
        return self._lib.rth_random_int(self._h, a, b)

    # texture.rs
    def solid_color(self, rgb) -> int:
        return _check_host(self._lib.rth_solid_color(self._h, *map(float, rgb)))

    def checker_texture(self, scale: float, even: int, odd: int) -> int:
        return _check_host(self._lib.rth_checker_texture(self._h, scale, even, odd))

    def checker_from_color(self, scale: float, c1, c2) -> int:
        return self.checker_texture(scale, self.solid_color(c1), self.solid_color(c2))

    def noise_texture(self, scale: float) -> int:
        return _check_host(self._lib.rth_noise_texture(self._h, scale))

    def image_texture(self, rgb8: np.ndarray | None) -> int:
        if rgb8 is None:
            return _check_host(self._lib.rth_image_texture(self._h, 0, 0, None))
        a = np.ascontiguousarray(rgb8, dtype=np.uint8)
        h, w = a.shape[:2]
        return _check_host(self._lib.rth_image_texture(self._h, w, h, a.ctypes.data))

    # material.rs
    def lambertian(self, rgb=None, tex: int | None = None) -> int:
        if tex is not None:
            return _check_host(self._lib.rth_lambertian_tex(self._h, tex))
        return _check_host(self._lib.rth_lambertian(self._h, *map(float, rgb)))

    def metal(self, rgb, fuzz: float) -> int:
        return _check_host(self._lib.rth_metal(self._h, *map(float, rgb), fuzz))

    def dielectric(self, ir: float, tint=(1.0, 1.0, 1.0)) -> int:
        return _check_host(self._lib.rth_dielectric(self._h, ir, *map(float, tint)))

    def diffuse_light(self, rgb=None, tex: int | None = None) -> int:
        if tex is not None:
            return _check_host(self._lib.rth_diffuse_light_tex(self._h, tex))
        return _check_host(self._lib.rth_diffuse_light(self._h, *map(float, rgb)))

    def isotropic(self, rgb=None, tex: int | None = None) -> int:
        if tex is not None:
            return _check_host(self._lib.rth_isotropic_tex(self._h, tex))
        return _check_host(self._lib.rth_isotropic(self._h, *map(float, rgb)))

    # object.rs / hittable.rs / transform.rs / constant_medium.rs
    def sphere(self, center, radius: float, mat: int) -> int:
        return _check_host(self._lib.rth_sphere(self._h, _d3(center), radius, mat))

    def sphere_moving(self, c1, c2, radius: float, mat: int) -> int:
        return _check_host(self._lib.rth_sphere_moving(self._h, _d3(c1), _d3(c2), radius, mat))

    def quad(self, q, u, v, mat: int) -> int:
        return _check_host(self._lib.rth_quad(self._h, _d3(q), _d3(u), _d3(v), mat))

    def make_box(self, a, b, mat: int) -> int:
        return _check_host(self._lib.rth_make_box(self._h, _d3(a), _d3(b), mat))

    def hittable_list(self, *objs: int) -> int:
        lst = _check_host(self._lib.rth_list_new(self._h))
        for o in objs:
            self.add(lst, o)
        return lst

    def add(self, lst: int, obj: int) -> None:
        _check_host(self._lib.rth_list_add(self._h, lst, obj))

    def create_bvh(self, lst: int) -> int:
        return _check_host(self._lib.rth_list_create_bvh(self._h, lst))

    def list_len(self, lst: int) -> int:
        return _check_host(self._lib.rth_list_len(self._h, lst))

    def translate(self, obj: int, offset) -> int:
        return _check_host(self._lib.rth_translate(self._h, obj, _d3(offset)))

    def rotate_y(self, obj: int, angle_deg: float) -> int:
        return _check_host(self._lib.rth_rotate_y(self._h, obj, angle_deg))

    def constant_medium(self, boundary: int, density: float, rgb=None,
                        tex: int | None = None) -> int:
        if tex is not None:
            return _check_host(self._lib.rth_constant_medium_tex(self._h, boundary, density, tex))
        return _check_host(self._lib.rth_constant_medium(self._h, boundary, density,
                                                         *map(float, rgb)))

    def bbox(self, obj: int) -> np.ndarray:
        out = _D3()
        buf = (C.c_double * 6)()
        _check_host(self._lib.rth_object_bbox(self._h, obj, buf))
        del out
        return np.array(buf[:])

    def serialize(self, world: int, lights: int | None = None) -> Blob:
        b = RtSceneBlob()
        _check_host(self._lib.rth_serialize(self._h, world, -1 if lights is None else lights,
                                            C.byref(b)))
        slots = np.ctypeslib.as_array(b.slots, shape=(b.n_slots,)).copy()
        tex = (np.ctypeslib.as_array(b.texels, shape=(b.n_texels,)).copy() if b.n_texels
               else np.zeros(0, np.uint8))
        return Blob(slots, tex)

    def preset(self, name: str, variant: str = "", width: int = 0, spp: int = 0, depth: int = 0,
               aspect: float = 0.0):
        """main.rs scene function -> (world list id, lights id or None, RtCamera)."""
        w, l = C.c_int32(), C.c_int32()
        cam = RtCamera()
        _check_host(self._lib.rth_preset(self._h, name.encode(), variant.encode(), width, spp,
                                         depth, aspect, C.byref(w), C.byref(l), C.byref(cam)))
        return w.value, (None if l.value < 0 else l.value), cam


def camera_new(aspect_ratio, image_width, samples_per_pixel, max_depth, vfov, lookfrom, lookat,
               vup, defocus_angle, focus_dist, background) -> RtCamera:
    """Camera::new (render.rs:62-133)."""
    cam = RtCamera()
    _check_host(host_lib().rth_camera_new(aspect_ratio, image_width, samples_per_pixel,
                                          max_depth, vfov, _d3(lookfrom), _d3(lookat), _d3(vup),
                                          defocus_angle, focus_dist, _d3(background),
                                          C.byref(cam)))
    return cam


def camera_orbit_y(cam: RtCamera, pivot, degrees: float) -> RtCamera:
    """rth_camera_orbit_y: `cam` turned `degrees` about the vertical axis through `pivot` (center
    and pixel00_loc about the pivot, the pixel deltas and defocus vectors about the origin).
    0 degrees is a bitwise copy."""
    out = RtCamera()
    _check_host(host_lib().rth_camera_orbit_y(C.byref(cam), _d3(pivot), float(degrees),
                                              C.byref(out)))
    return out


def preset_blob(name: str, variant: str = "", width: int = 0, spp: int = 0, depth: int = 0,
                aspect: float = 0.0, build_seed: int = 1):
    """Build a main.rs preset and serialise it: returns (Blob, RtCamera)."""
    sc = Scene(build_seed)
    w, l, cam = sc.preset(name, variant, width, spp, depth, aspect)
    return sc.serialize(w, l), cam


def make_opts(cam: RtCamera, seed: int = 1, row_begin: int = 0, row_step: int = 1,
              n_rows: int | None = None, flags: int = RT_FLAG_OVERWRITE, sj_begin: int = 0,
              sj_count: int = 0, device: int = 0) -> RtRenderOpts:
    o = RtRenderOpts()
    o.seed = seed
    o.row_begin = row_begin
    o.row_step = row_step
    if n_rows is None:
        n_rows = len(range(row_begin, cam.image_height, row_step))
    o.n_rows = n_rows
    o.flags = flags
    o.sj_begin = sj_begin
    o.sj_count = sj_count
    o.device = device
    return o


# ---------------------------------------------------------------------------- device render
class DeviceScene:
    """A flattened scene resident on one GPU (rt_scene_create)."""

    def __init__(self, blob: Blob, device: int = 0):
        self._lib = device_lib()
        self._blob = blob
        h = C.c_void_p()
        _check_dev(self._lib.rt_scene_create(blob.ref(), device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def device_bytes(self) -> int:
        return int(self._lib.rt_scene_device_bytes(self._h))

    def render(self, cam: RtCamera, opts: RtRenderOpts, accum: np.ndarray | None = None):
        """Synchronous render into a host float32 (n_rows, W, 3) array; returns (accum, stats)."""
        shape = (opts.n_rows, cam.image_width, 3)
        if accum is None:
            accum = np.zeros(shape, np.float32)
        assert accum.shape == shape and accum.dtype == np.float32 and accum.flags.c_contiguous
        st = RtStats()
        _check_dev(self._lib.rt_render(self._h, C.byref(cam), C.byref(opts), accum.ctypes.data,
                                       C.byref(st)))
        return accum, st

    def render_device(self, cam: RtCamera, opts: RtRenderOpts, dev_ptr: int, stream: int = 0,
                      stats: bool = False):
        """Asynchronous render into a device buffer (e.g. a torch tensor's data_ptr())."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_render_device(self._h, C.byref(cam), C.byref(opts),
                                              C.c_void_p(dev_ptr), C.c_void_p(stream or None),
                                              C.byref(st) if st is not None else None))
        return st

    def render_moments(self, cam: RtCamera, opts: RtRenderOpts, accum: np.ndarray | None = None,
                       m2: np.ndarray | None = None, stats: bool = False):
        """Synchronous rt_render_moments into host float32 (n_rows, W, 3) arrays: the beauty sums
        exactly as render() gives them, and per pixel and channel the sum over the call's stratum
        rows of the squared row totals. Without RT_FLAG_OVERWRITE both are added into the arrays
        passed in. Returns (accum, m2), or (accum, m2, stats) with stats=True. With n rows and B
        samples held, max(0, m2 - accum**2 / n) * n / ((n - 1) * B**2) estimates the variance of
        the pixel mean."""
        shape = (opts.n_rows, cam.image_width, 3)
        if accum is None:
            accum = np.zeros(shape, np.float32)
        if m2 is None:
            m2 = np.zeros(shape, np.float32)
        for a in (accum, m2):
            assert a.shape == shape and a.dtype == np.float32 and a.flags.c_contiguous
        st = RtStats()
        _check_dev(self._lib.rt_render_moments(self._h, C.byref(cam), C.byref(opts),
                                               accum.ctypes.data, m2.ctypes.data, C.byref(st)))
        return (accum, m2, st) if stats else (accum, m2)

    def render_moments_device(self, cam: RtCamera, opts: RtRenderOpts, accum_ptr: int,
                              m2_ptr: int, stream: int = 0, stats: bool = False):
        """Asynchronous rt_render_moments_device into two device buffers of n_rows * W * 3
        floats."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_render_moments_device(
            self._h, C.byref(cam), C.byref(opts), C.c_void_p(accum_ptr), C.c_void_p(m2_ptr),
            C.c_void_p(stream or None), C.byref(st) if st is not None else None))
        return st

    def render_tiles_device(self, cam: RtCamera, opts: RtRenderOpts, tiles, sj_step: int,
                            accum_ptr: int, m2_ptr: int = 0, stream: int = 0,
                            stats: bool = False):
        """Asynchronous rt_render_tiles_device: the 8x8 tiles listed in `tiles` (strictly
        ascending indices of the call's tile grid, ty * ceil(W / 8) + tx) over the stratum rows
        opts.sj_begin + k * sj_step, k < opts.sj_count (>= 1), into device buffers of
        n_rows * W * 3 floats of which only the listed tiles' pixels are touched (m2_ptr 0 = no
        second moments)."""
        t = np.ascontiguousarray(tiles, np.uint32)
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_render_tiles_device(
            self._h, C.byref(cam), C.byref(opts), t.ctypes.data, t.size, sj_step,
            C.c_void_p(accum_ptr), C.c_void_p(m2_ptr or None), C.c_void_p(stream or None),
            C.byref(st) if st is not None else None))
        return st

    def render_aov(self, cam: RtCamera, opts: RtRenderOpts, aov: np.ndarray | None = None):
        """Synchronous first-hit AOV pass (rt_render_aov) into a host float32
        (n_rows, W, AOV_CHANNELS) array: per-pixel sums over the call's samples of hits, t (the
        ray parameter of the unnormalised camera ray), normal, albedo and emission, and the first
        sample's material id (aov_planes names them); returns (aov, stats). Without
        RT_FLAG_OVERWRITE the sums are added into `aov`."""
        shape = (opts.n_rows, cam.image_width, AOV_CHANNELS)
        if aov is None:
            aov = np.zeros(shape, np.float32)
        assert aov.shape == shape and aov.dtype == np.float32 and aov.flags.c_contiguous
        st = RtStats()
        _check_dev(self._lib.rt_render_aov(self._h, C.byref(cam), C.byref(opts), aov.ctypes.data,
                                           C.byref(st)))
        return aov, st

    def render_aov_device(self, cam: RtCamera, opts: RtRenderOpts, dev_ptr: int, stream: int = 0,
                          stats: bool = False):
        """Asynchronous AOV pass into a device buffer of n_rows * W * AOV_CHANNELS floats."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_render_aov_device(self._h, C.byref(cam), C.byref(opts),
                                                  C.c_void_p(dev_ptr), C.c_void_p(stream or None),
                                                  C.byref(st) if st is not None else None))
        return st

    def query(self, rays: np.ndarray, seed: int = 1, flags: int = 0, occlusion: bool = False,
              stats: bool = False, any_hit: bool = False):
        """Synchronous rt_query_rays: the closest hit of every ray of a RAY_DTYPE array
        (make_rays) as a HIT_DTYPE array, or with occlusion=True one uint8 per ray (1 hit, 0 miss,
        255 invalid ray). any_hit=True (with occlusion=True only): the same bytes from a walk that
        leaves at the first accepted primitive. `flags`: RT_FLAG_REFERENCE_BVH or 0. Returns the
        array, or (array, stats) with stats=True."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(len(rays), np.uint8 if occlusion else HIT_DTYPE)
        qp = RtQueryParams(seed, flags, _query_mode(occlusion, any_hit))
        st = RtStats()
        if len(rays):
            _check_dev(self._lib.rt_query_rays(self._h, C.byref(qp), rays.ctypes.data, len(rays),
                                               out.ctypes.data, C.byref(st)))
        return (out, st) if stats else out

    def query_device(self, rays_ptr: int, n: int, out_ptr: int, seed: int = 1, flags: int = 0,
                     occlusion: bool = False, stream: int = 0, stats: bool = False,
                     any_hit: bool = False):
        """Asynchronous rt_query_rays_device: n rt_ray records at rays_ptr (16-byte aligned, e.g. a
        torch tensor's data_ptr()) into n rt_hit records, or n bytes with occlusion=True (any_hit=
        True: the early-exit walk, the same bytes), at out_ptr, on `stream` (e.g.
        torch.cuda.current_stream().cuda_stream)."""
        qp = RtQueryParams(seed, flags, _query_mode(occlusion, any_hit))
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_query_rays_device(
            self._h, C.byref(qp), C.c_void_p(rays_ptr), n, C.c_void_p(out_ptr),
            C.c_void_p(stream or None), C.byref(st) if st is not None else None))
        return st

    def render_rays(self, rays: np.ndarray, params: RtRaysParams, rgb: np.ndarray | None = None,
                    stats: bool = False):
        """Synchronous rt_render_rays: the path-traced radiance sums of a RAY_DTYPE array
        (make_rays, projection_rays) under `params` (make_rays_params) as float32 [n, 3]. Without
        RT_FLAG_OVERWRITE the sums are added into `rgb`. An invalid ray's three values are NaN.
        Returns rgb, or (rgb, stats) with stats=True."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        if rgb is None:
            rgb = np.zeros((len(rays), 3), np.float32)
        assert rgb.shape == (len(rays), 3) and rgb.dtype == np.float32 and rgb.flags.c_contiguous
        st = RtStats()
        if len(rays):
            _check_dev(self._lib.rt_render_rays(self._h, C.byref(params), rays.ctypes.data,
                                                len(rays), rgb.ctypes.data, C.byref(st)))
        return (rgb, st) if stats else rgb

    def render_rays_device(self, rays_ptr: int, n: int, rgb_ptr: int, params: RtRaysParams,
                           stream: int = 0, stats: bool = False):
        """Asynchronous rt_render_rays_device: n rt_ray records at rays_ptr (16-byte aligned, e.g.
        a torch tensor's data_ptr()) into n * 3 floats at rgb_ptr, on `stream`."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_render_rays_device(
            self._h, C.byref(params), C.c_void_p(rays_ptr), n, C.c_void_p(rgb_ptr),
            C.c_void_p(stream or None), C.byref(st) if st is not None else None))
        return st

    def jit_info(self) -> tuple[int, str]:
        """(state, message) of the scene-specialised kernel: 1 compiled and in use, 0 not compiled
        yet, -1 not generated for this scene, -2 compilation failed (rt_scene_jit_info)."""
        st = C.c_int(0)
        buf = C.create_string_buffer(1 << 16)
        _check_dev(self._lib.rt_scene_jit_info(self._h, C.byref(st), buf, len(buf)))
        return st.value, buf.value.decode(errors="replace")

    def trace_ms(self, n: int) -> list[float]:
        """Device ms of the rt_trace kernel alone for the last n renders (oldest first)."""
        buf = (C.c_float * max(1, n))()
        got = C.c_int(0)
        _check_dev(self._lib.rt_scene_trace_ms(self._h, buf, n, C.byref(got)))
        return [float(buf[i]) for i in range(got.value)]


def aov_planes(aov: np.ndarray) -> dict:
    """Named views of an AOV array [..., AOV_CHANNELS]: hits, t, normal (3), albedo (3),
    emission (3), matid. Views, not copies; divide the sums by the call's samples per pixel
    (normal, albedo and t by `hits` for a per-hit mean)."""
    assert aov.shape[-1] == AOV_CHANNELS
    return dict(hits=aov[..., AOV_HITS], t=aov[..., AOV_T],
                normal=aov[..., AOV_NORMAL:AOV_NORMAL + 3],
                albedo=aov[..., AOV_ALBEDO:AOV_ALBEDO + 3],
                emission=aov[..., AOV_EMISSION:AOV_EMISSION + 3], matid=aov[..., AOV_MATID])


def denoise_default_params(width: int, height: int, beauty_samples: float,
                           aov_samples: float | None = None) -> RtDenoiseParams:
    """rt_denoise_default_params (host only): 5 levels, DENOISE_DEMODULATE, sigmas 4.0 / 0.3 /
    0.1 / 0.1 for colour / normal / depth / albedo. aov_samples defaults to beauty_samples."""
    p = RtDenoiseParams()
    _check_dev(device_lib().rt_denoise_default_params(
        width, height, beauty_samples, beauty_samples if aov_samples is None else aov_samples,
        C.byref(p)))
    return p


def denoise_var_default_params(width: int, height: int, beauty_samples: float, beauty_rows: int,
                               aov_samples: float | None = None) -> RtDenoiseVarParams:
    """rt_denoise_var_default_params (host only): 5 levels, DENOISE_DEMODULATE, sigmas 4.0 / 0.3 /
    0.1 / 0.1; sigma_color is in units of a pixel pair's standard deviation. beauty_rows: the
    stratum rows the beauty and m2 sums hold (cam.sqrt_spp for a whole render)."""
    p = RtDenoiseVarParams()
    _check_dev(device_lib().rt_denoise_var_default_params(
        width, height, beauty_samples, beauty_rows,
        beauty_samples if aov_samples is None else aov_samples, C.byref(p)))
    return p


class Denoiser:
    """The edge-avoiding a-trous denoiser on one GPU (rt_denoiser_create): a workspace that grows
    to the largest frame it has seen. Calls on one Denoiser are serialised and ordered; several
    Denoisers run concurrently."""

    def __init__(self, device: int = 0):
        self._lib = device_lib()
        h = C.c_void_p()
        _check_dev(self._lib.rt_denoiser_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_denoiser_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def denoise(self, beauty: np.ndarray, aov: np.ndarray, params: RtDenoiseParams,
                stats: bool = False):
        """Synchronous rt_denoise over host arrays: beauty (H, W, 3) raw sums as render()
        returns them, aov (H, W, AOV_CHANNELS) as render_aov() returns them. Returns the denoised
        (H, W, 3) float32 frame in the scale of the beauty sums (write_color(out, spp) as for the
        beauty), or (frame, RtStats) with stats=True."""
        shape = (params.height, params.width)
        assert beauty.shape == shape + (3,) and aov.shape == shape + (AOV_CHANNELS,)
        b = np.ascontiguousarray(beauty, np.float32)
        a = np.ascontiguousarray(aov, np.float32)
        out = np.zeros(shape + (3,), np.float32)
        st = RtStats()
        _check_dev(self._lib.rt_denoise(self._h, C.byref(params), b.ctypes.data, a.ctypes.data,
                                        out.ctypes.data, C.byref(st)))
        return (out, st) if stats else out

    def denoise_device(self, params: RtDenoiseParams, beauty_ptr: int, aov_ptr: int,
                       out_ptr: int, stream: int = 0, stats: bool = False):
        """Asynchronous rt_denoise_device over device buffers (out_ptr may equal beauty_ptr)."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_denoise_device(self._h, C.byref(params), C.c_void_p(beauty_ptr),
                                               C.c_void_p(aov_ptr), C.c_void_p(out_ptr),
                                               C.c_void_p(stream or None),
                                               C.byref(st) if st is not None else None))
        return st


    def denoise_var(self, beauty: np.ndarray, m2: np.ndarray, aov: np.ndarray,
                    params: RtDenoiseVarParams, var_out: bool = False, stats: bool = False):
        """Synchronous rt_denoise_var over host arrays: beauty and m2 (H, W, 3) as
        render_moments() returns them, aov as render_aov() returns it. Returns the denoised frame,
        followed by the (H, W) variance of the filtered value with var_out=True and by RtStats
        with stats=True."""
        shape = (params.height, params.width)
        assert beauty.shape == shape + (3,) and m2.shape == shape + (3,)
        assert aov.shape == shape + (AOV_CHANNELS,)
        b = np.ascontiguousarray(beauty, np.float32)
        q = np.ascontiguousarray(m2, np.float32)
        a = np.ascontiguousarray(aov, np.float32)
        out = np.zeros(shape + (3,), np.float32)
        var = np.zeros(shape, np.float32) if var_out else None
        st = RtStats()
        _check_dev(self._lib.rt_denoise_var(self._h, C.byref(params), b.ctypes.data,
                                            q.ctypes.data, a.ctypes.data, out.ctypes.data,
                                            var.ctypes.data if var_out else None, C.byref(st)))
        res = (out,) + ((var,) if var_out else ()) + ((st,) if stats else ())
        return res if len(res) > 1 else out

    def denoise_var_device(self, params: RtDenoiseVarParams, beauty_ptr: int, m2_ptr: int,
                           aov_ptr: int, out_ptr: int, var_out_ptr: int = 0, stream: int = 0,
                           stats: bool = False):
        """Asynchronous rt_denoise_var_device over device buffers (out_ptr may equal beauty_ptr;
        var_out_ptr 0 = no variance output)."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_denoise_var_device(
            self._h, C.byref(params), C.c_void_p(beauty_ptr), C.c_void_p(m2_ptr),
            C.c_void_p(aov_ptr), C.c_void_p(out_ptr), C.c_void_p(var_out_ptr or None),
            C.c_void_p(stream or None), C.byref(st) if st is not None else None))
        return st


# ---------------------------------------------------------------------------- temporal accumulation
def temporal_default_params(width: int, height: int) -> RtTemporalParams:
    """rt_temporal_default_params (host only): no flags, beauty_rows 0, max_history 4, depth_tol
    0.1, normal_tol 0.3, min_weight 0.01."""
    p = RtTemporalParams()
    _check_dev(device_lib().rt_temporal_default_params(width, height, C.byref(p)))
    return p


class Temporal:
    """Temporal accumulation on one GPU (rt_temporal_create): the handle keeps the accumulated
    frame, its guides and its camera, and each accumulate() reprojects that history into the new
    frame and blends. Calls on one Temporal are serialised and ordered; several run concurrently."""

    def __init__(self, device: int = 0):
        self._lib = device_lib()
        h = C.c_void_p()
        _check_dev(self._lib.rt_temporal_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_temporal_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def info(self) -> dict:
        out = (C.c_uint64 * 4)()
        _check_dev(self._lib.rt_temporal_info(self._h, out, 4))
        return dict(frames=int(out[0]), width=int(out[1]), height=int(out[2]),
                    moments=bool(out[3]))

    def accumulate(self, cam: RtCamera, beauty: np.ndarray, aov: np.ndarray,
                   params: RtTemporalParams, m2: np.ndarray | None = None,
                   hist_len: bool = False, stats: bool = False):
        """Synchronous rt_temporal_accumulate over host arrays: beauty (and m2) (H, W, 3) as
        render_moments() returns them, aov as render_aov() returns it, cam the camera that
        rendered them. Returns the accumulated beauty, followed by the accumulated m2 when m2 is
        given, by the (H, W) history lengths with hist_len=True and by RtStats with stats=True."""
        shape = (params.height, params.width)
        assert beauty.shape == shape + (3,) and aov.shape == shape + (AOV_CHANNELS,)
        assert m2 is None or m2.shape == shape + (3,)
        b = np.ascontiguousarray(beauty, np.float32)
        a = np.ascontiguousarray(aov, np.float32)
        q = None if m2 is None else np.ascontiguousarray(m2, np.float32)
        out = np.zeros(shape + (3,), np.float32)
        out_q = None if m2 is None else np.zeros(shape + (3,), np.float32)
        ln = np.zeros(shape, np.float32) if hist_len else None
        st = RtStats()
        _check_dev(self._lib.rt_temporal_accumulate(
            self._h, C.byref(params), C.byref(cam), b.ctypes.data,
            None if q is None else q.ctypes.data, a.ctypes.data, out.ctypes.data,
            None if out_q is None else out_q.ctypes.data, None if ln is None else ln.ctypes.data,
            C.byref(st)))
        res = ((out,) + ((out_q,) if m2 is not None else ()) + ((ln,) if hist_len else ()) +
               ((st,) if stats else ()))
        return res if len(res) > 1 else out

    def accumulate_device(self, params: RtTemporalParams, cam: RtCamera, beauty_ptr: int,
                          aov_ptr: int, out_beauty_ptr: int, m2_ptr: int = 0, out_m2_ptr: int = 0,
                          hist_len_ptr: int = 0, stream: int = 0, stats: bool = False):
        """Asynchronous rt_temporal_accumulate_device over device buffers (out_beauty_ptr may equal
        beauty_ptr, out_m2_ptr may equal m2_ptr; 0 = not given)."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_temporal_accumulate_device(
            self._h, C.byref(params), C.byref(cam), C.c_void_p(beauty_ptr),
            C.c_void_p(m2_ptr or None), C.c_void_p(aov_ptr), C.c_void_p(out_beauty_ptr),
            C.c_void_p(out_m2_ptr or None), C.c_void_p(hist_len_ptr or None),
            C.c_void_p(stream or None), C.byref(st) if st is not None else None))
        return st


# ---------------------------------------------------------------------------- adaptive sampling
def adaptive_schedule(sqrt_spp: int, passes: int, pass_: int) -> tuple[int, int, int]:
    """rt_adaptive_schedule (host only): (sj_begin, sj_step, sj_count) of pass `pass_` of `passes`
    over sqrt_spp stratum rows: rows pass_, pass_ + passes, ... Valid for 1 <= passes <=
    sqrt_spp // 2."""
    b, s, n = C.c_int(0), C.c_int(0), C.c_int(0)
    _check_dev(device_lib().rt_adaptive_schedule(sqrt_spp, passes, pass_, C.byref(b), C.byref(s),
                                                 C.byref(n)))
    return b.value, s.value, n.value


def tile_grid(width: int, height: int) -> tuple[int, int]:
    """(tiles_x, tiles_y) of the 8x8 tile grid of a width x height call."""
    return (width + 7) // 8, (height + 7) // 8


class Adaptive:
    """Adaptive sampling on one GPU (rt_adaptive_create): per-tile error estimates from the sample
    moments, the resolve of unevenly sampled sums and the driver that renders only the tiles that
    have not converged. Calls on one Adaptive are serialised."""

    def __init__(self, device: int = 0):
        self._lib = device_lib()
        self.device = device
        h = C.c_void_p()
        _check_dev(self._lib.rt_adaptive_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_adaptive_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def tile_error(self, width: int, height: int, sqrt_spp: int, floor: float, accum_ptr: int,
                   m2_ptr: int, rows_held, stream: int = 0):
        """Synchronous rt_adaptive_tile_error over device sums: returns (err, n_invalid), err a
        float32 array of one value per tile (the largest relative standard error of its valid
        pixels; +inf where rows_held < 2)."""
        rows = np.ascontiguousarray(rows_held, np.uint32)
        tx, ty = tile_grid(width, height)
        assert rows.size == tx * ty
        err = np.zeros(tx * ty, np.float32)
        inv = C.c_uint64(0)
        _check_dev(self._lib.rt_adaptive_tile_error(
            self._h, width, height, sqrt_spp, floor, C.c_void_p(accum_ptr), C.c_void_p(m2_ptr),
            rows.ctypes.data, err.ctypes.data, C.byref(inv), C.c_void_p(stream or None)))
        return err, int(inv.value)

    def resolve_device(self, width: int, height: int, sqrt_spp: int, rows_held, accum_ptr: int,
                       out_ptr: int, samples_ptr: int = 0, stream: int = 0):
        """Asynchronous rt_adaptive_resolve_device: out = accum * sqrt_spp**2 / samples held, in
        the scale of a full-spp render (out_ptr may equal accum_ptr); samples_ptr (0 = none)
        receives the samples each pixel holds."""
        rows = np.ascontiguousarray(rows_held, np.uint32)
        tx, ty = tile_grid(width, height)
        assert rows.size == tx * ty
        _check_dev(self._lib.rt_adaptive_resolve_device(
            self._h, width, height, sqrt_spp, rows.ctypes.data, C.c_void_p(accum_ptr),
            C.c_void_p(out_ptr), C.c_void_p(samples_ptr or None), C.c_void_p(stream or None)))

    def render_device(self, scene: "DeviceScene", cam: RtCamera, opts: RtRenderOpts,
                      params: RtAdaptiveParams, accum_ptr: int, m2_ptr: int, out_ptr: int = 0,
                      samples_ptr: int = 0, stream: int = 0):
        """Synchronous rt_render_adaptive_device over device buffers. Returns (rows_held,
        tiles_per_pass, stats): the stratum rows each tile ended with, the number of tiles each
        pass rendered, and RtStats (samples = pixel-samples actually traced)."""
        tx, ty = tile_grid(cam.image_width, opts.n_rows)
        rows = np.zeros(tx * ty, np.uint32)
        per = np.zeros(max(1, params.passes), np.uint32)
        st = RtStats()
        _check_dev(self._lib.rt_render_adaptive_device(
            self._h, scene._h, C.byref(cam), C.byref(opts), C.byref(params),
            C.c_void_p(accum_ptr), C.c_void_p(m2_ptr), C.c_void_p(out_ptr or None),
            C.c_void_p(samples_ptr or None), rows.ctypes.data, per.ctypes.data,
            C.c_void_p(stream or None), C.byref(st)))
        return rows, per, st

    def render(self, scene: "DeviceScene", cam: RtCamera, opts: RtRenderOpts,
               params: RtAdaptiveParams):
        """The driver with host results: returns (out, samples, rows_held, tiles_per_pass, stats),
        out the resolved (n_rows, W, 3) float32 frame in the scale of a full-spp render
        (write_color(out, spp)), samples the (n_rows, W) samples each pixel holds."""
        shape = (opts.n_rows, cam.image_width)
        acc, m2, out = (np.zeros(shape + (3,), np.float32) for _ in range(3))
        smp = np.zeros(shape, np.float32)
        tx, ty = tile_grid(cam.image_width, opts.n_rows)
        rows = np.zeros(tx * ty, np.uint32)
        per = np.zeros(max(1, params.passes), np.uint32)
        st = RtStats()
        _check_dev(self._lib.rt_render_adaptive(
            self._h, scene._h, C.byref(cam), C.byref(opts), C.byref(params), acc.ctypes.data,
            m2.ctypes.data, out.ctypes.data, smp.ctypes.data, rows.ctypes.data, per.ctypes.data,
            C.byref(st)))
        return out, smp, rows, per, st


def render_par_lights(blob: Blob, cam: RtCamera, seed: int = 1, device: int = 0,
                      flags: int = RT_FLAG_OVERWRITE):
    """Drop-in for render_par_lights (render.rs:144-216) minus the PPM side effect:
    returns the raw per-pixel sums (H, W, 3) float32, as the reference's `pixels` vector."""
    ds = DeviceScene(blob, device)
    try:
        accum, st = ds.render(cam, make_opts(cam, seed=seed, flags=flags, device=device))
    finally:
        ds.close()
    return accum, st


LAYOUT_STATS = ["node_words", "bvh_words", "bvh_records", "dup_records", "volumes",
                "volumes_one_walk_sphere", "volumes_one_walk_quads", "lights", "ordered_bvhs",
                "compact_bvhs", "compact_bvh_bytes"]
# rt_scene_lds_check (include/rt_mi355x.h RT_LDS_CHECK)
LDS_CHECK = ["block", "static_lds", "stage_bytes", "cbvh_lds_off", "cbvh_bytes", "stack_lds_off",
             "cbvh_stack", "lds_bytes", "lds_total", "lds_cu", "trees", "max_depth", "errors",
             "max_store_slot", "max_live", "rays", "steps", "max_read", "row_lds_off"]


def render_multi(blob: "Blob", cam: RtCamera, opts: RtRenderOpts, devices,
                 accum: np.ndarray | None = None):
    """rt_render_multi: the call's rows dealt cyclically over `devices` (one process, N GPUs),
    gathered into one host frame. Returns (accum [n_rows, W, 3] float32, RtStats)."""
    devs = (C.c_int * len(devices))(*devices)
    if accum is None:
        accum = np.zeros((opts.n_rows, cam.image_width, 3), np.float32)
    st = RtStats()
    _check_dev(device_lib().rt_render_multi(blob.ref(), C.byref(cam), C.byref(opts), devs,
                                            len(devices), accum.ctypes.data, C.byref(st)))
    return accum, st


class MultiScene:
    """rt_multi_*: the scene resident on several GPUs of one process, frame after frame; rows are
    dealt cyclically and gathered peer to peer into a buffer on devices[0]."""

    def __init__(self, blob: "Blob", devices):
        self._lib = device_lib()
        self._blob = blob
        self.devices = list(devices)
        devs = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check_dev(self._lib.rt_multi_create(blob.ref(), devs, len(self.devices), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def render_device(self, cam: RtCamera, opts: RtRenderOpts, dev_ptr: int, stream: int = 0,
                      stats: bool = False):
        """Asynchronous frame into a devices[0] buffer (e.g. a torch tensor's data_ptr())."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_multi_render(self._h, C.byref(cam), C.byref(opts),
                                             C.c_void_p(dev_ptr), C.c_void_p(stream or None),
                                             C.byref(st) if st is not None else None))
        return st

    def info(self) -> dict:
        out = (C.c_uint64 * 4)()
        _check_dev(self._lib.rt_multi_info(self._h, out, 4))
        return dict(zip(("frames", "uploads", "stage_allocs", "devices"), (int(v) for v in out)))


def validate(blob: "Blob") -> int:
    """rt_scene_validate: RT_OK, or raises RtError with the library's status and message."""
    return _check_dev(device_lib().rt_scene_validate(blob.ref()))


def layout_stats(blob: "Blob") -> dict:
    """Host-only counts of the flattened device layout (rt_scene_layout_stats)."""
    out = (C.c_uint32 * len(LAYOUT_STATS))()
    _check_dev(device_lib().rt_scene_layout_stats(blob.ref(), out, len(LAYOUT_STATS)))
    return dict(zip(LAYOUT_STATS, (int(v) for v in out)))


def prim_map(blob: "Blob") -> tuple[np.ndarray, np.ndarray]:
    """Host-only: the table behind RtHit.prim (rt_scene_prim_map) as (node_word, prim), two uint32
    arrays: every leaf record of the flattened world by word offset, ascending, and its prim."""
    n = C.c_uint32(0)
    _check_dev(device_lib().rt_scene_prim_map(blob.ref(), None, None, 0, C.byref(n)))
    word, prim = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    if n.value:
        _check_dev(device_lib().rt_scene_prim_map(blob.ref(), word.ctypes.data_as(u32p),
                                                  prim.ctypes.data_as(u32p), n.value, C.byref(n)))
    return word, prim


def lds_check(blob: "Blob", flags: int = 0, n_rays: int = 4096, seed: int = 1) -> dict:
    """Host-only: the product render's LDS plan and a check of the compact BVHs the LDS walk
    reads, with a host restatement of the walk's stack and region addressing over random rays
    (rt_scene_lds_check). `first_error` is empty when every tree is well formed."""
    out = (C.c_uint64 * len(LDS_CHECK))()
    msg = C.create_string_buffer(512)
    _check_dev(device_lib().rt_scene_lds_check(blob.ref(), flags, n_rays, seed, out,
                                               len(LDS_CHECK), msg, len(msg)))
    d = dict(zip(LDS_CHECK, (int(v) for v in out)))
    d["first_error"] = msg.value.decode(errors="replace")
    return d


def jit_check(blob: "Blob", arch: str = "gfx950") -> tuple[int, str]:
    """Host-only: generate the scene-specialised walker for `blob` and compile it with hiprtc
    (rt_jit_check). (1, walker source) | (-1, why not generated); raises on a compile error."""
    st = C.c_int(0)
    buf = C.create_string_buffer(1 << 20)
    _check_dev(device_lib().rt_jit_check(blob.ref(), arch.encode(), C.byref(st), buf, len(buf)))
    return st.value, buf.value.decode(errors="replace")


def device_count() -> int:
    n = C.c_int(0)
    device_lib().rt_device_count(C.byref(n))
    return n.value


# ---------------------------------------------------------------------------- output stage
def write_color(accum: np.ndarray, samples_per_pixel: float,
                exposure: float | None = None) -> np.ndarray:
    """color.rs write_color over a whole frame: raw sums -> sRGB8 (H, W, 3) uint8."""
    a = np.ascontiguousarray(accum, dtype=np.float32)
    out = np.zeros(a.shape, np.uint8)
    n = a.size // 3
    host_lib().rth_write_color(a.ctypes.data, n, float(samples_per_pixel),
                               0 if exposure is None else 1,
                               0.0 if exposure is None else float(exposure), out.ctypes.data)
    return out


def auto_expose(accum: np.ndarray, samples_per_pixel: int) -> float:
    """render.rs:325-339."""
    a = np.ascontiguousarray(accum, dtype=np.float32)
    return host_lib().rth_auto_expose(a.ctypes.data, a.size // 3, int(samples_per_pixel))


def output_params(width: int, height: int, samples_per_pixel: float,
                  exposure: float | None = None, auto: bool = False,
                  rgba: bool = False) -> RtOutputParams:
    """rt_output_params: exposure=None and auto=False is write_color without an exposure step;
    auto=True computes auto_expose on the device (exposure is then ignored)."""
    p = RtOutputParams()
    p.width, p.height, p.samples_per_pixel = width, height, samples_per_pixel
    p.flags = ((RT_OUTPUT_AUTO_EXPOSE if auto else 0) | (RT_OUTPUT_RGBA if rgba else 0) |
               (RT_OUTPUT_EXPOSURE if exposure is not None and not auto else 0))
    p.exposure = 0.0 if exposure is None or auto else exposure
    return p


class Output:
    """The output stage on one GPU (rt_output_create): raw sums -> exposure, gamma, RGB8 or RGBA8,
    with auto_expose as a fixed-order device reduction. write_color and auto_expose above stay
    the host reference. Calls on one Output are serialised and ordered."""

    def __init__(self, device: int = 0):
        self._lib = device_lib()
        h = C.c_void_p()
        _check_dev(self._lib.rt_output_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_output_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _has_exposure(params: RtOutputParams) -> bool:
        return bool(params.flags & (RT_OUTPUT_EXPOSURE | RT_OUTPUT_AUTO_EXPOSE))

    def output(self, sums: np.ndarray, params: RtOutputParams, stats: bool = False):
        """Synchronous rt_output over a host array of (H, W, 3) raw sums. Returns (rgb8, ev):
        the (H, W, 3) or, with RT_OUTPUT_RGBA, (H, W, 4) uint8 frame and the exposure applied
        (None without an exposure step); (rgb8, ev, RtStats) with stats=True."""
        shape = (params.height, params.width)
        assert sums.shape == shape + (3,)
        a = np.ascontiguousarray(sums, np.float32)
        out = np.zeros(shape + (4 if params.flags & RT_OUTPUT_RGBA else 3,), np.uint8)
        ev = C.c_double(0.0)
        st = RtStats()
        _check_dev(self._lib.rt_output(self._h, C.byref(params), a.ctypes.data, out.ctypes.data,
                                       C.byref(ev), C.byref(st)))
        res = (out, ev.value if self._has_exposure(params) else None)
        return res + (st,) if stats else res

    def output_device(self, params: RtOutputParams, sums_ptr: int, rgb8_ptr: int, stream: int = 0,
                      want_exposure: bool = False, stats: bool = False):
        """rt_output_device over device buffers: asynchronous on `stream` unless want_exposure or
        stats, which synchronise. Returns None, the exposure applied (want_exposure; None without
        an exposure step), RtStats (stats), or (exposure, RtStats)."""
        ev = C.c_double(0.0) if want_exposure else None
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_output_device(
            self._h, C.byref(params), C.c_void_p(sums_ptr), C.c_void_p(rgb8_ptr),
            C.byref(ev) if ev is not None else None, C.c_void_p(stream or None),
            C.byref(st) if st is not None else None))
        res = ()
        if want_exposure:
            res += (ev.value if self._has_exposure(params) else None,)
        if stats:
            res += (st,)
        return None if not res else res[0] if len(res) == 1 else res


# ---------------------------------------------------------------------------- ray generators
def make_projection(kind, width: int = 0, height: int = 0, sqrt_spp: int = 1,
                    origin=(0.0, 0.0, 0.0), forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0),
                    fov: float = 0.0) -> RtProjection:
    """rt_projection (the fields of projection_rays above). kind: a PROJECTIONS name or value."""
    pr = RtProjection()
    pr.kind = PROJECTIONS[kind] if isinstance(kind, str) else int(kind)
    pr.width, pr.height, pr.sqrt_spp, pr.fov = width, height, sqrt_spp, fov
    pr.origin, pr.forward, pr.up = _d3(origin), _d3(forward), _d3(up)
    return pr


def make_ao_frame_params(directions: int, seed: int = 1, radius: float = float("inf"),
                         tmin: float = 1e-4, flags: int = RT_FLAG_OVERWRITE, channels: int = 3,
                         chunk_rays: int = 0) -> RtAoFrameParams:
    """rt_ao_frame_params: K directions per ray over [tmin, radius]; flags: RT_FLAG_OVERWRITE
    and RT_FLAG_REFERENCE_BVH; chunk_rays 0 = the default chunk."""
    return RtAoFrameParams(seed, radius, tmin, directions, flags, channels, chunk_rays)


_hip_rt = None


def _hip() -> C.CDLL:
    """The HIP runtime the device library links, for RayGen.ambient_occlusion's staging."""
    global _hip_rt
    if _hip_rt is None:
        device_lib()  # loads libamdhip64.so.7 as a dependency
        h = C.CDLL("libamdhip64.so.7")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipSetDevice.argtypes = [C.c_int]
        _hip_rt = h
    return _hip_rt


class RayGen:
    """The ray generators on one GPU (rt_raygen_create): projection rays, ambient-occlusion ray
    batches and the count of unoccluded directions formed in device buffers, and the AO frame
    driver over DeviceScene's queries. projection_rays and ao_rays above stay the host reference.
    Calls on one RayGen are serialised and ordered."""

    def __init__(self, device: int = 0):
        self._lib = device_lib()
        self.device = device
        h = C.c_void_p()
        _check_dev(self._lib.rt_raygen_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_raygen_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def projection_rays_device(self, proj: RtProjection, rays_ptr: int, seed: int = 1,
                               s_i: int = 0, s_j: int = 0, row_begin: int = 0,
                               n_rows: int | None = None, cam: "RtCamera | None" = None,
                               stream: int = 0, stats: bool = False):
        """Asynchronous rt_projection_rays_device: the rays of rows [row_begin, row_begin + n_rows)
        (default: to the last row) of stratum (s_i, s_j) into n_rows * width rt_ray records at
        rays_ptr (16-byte aligned). cam: the camera of a "pinhole" projection."""
        if n_rows is None:
            pin = proj.kind == RT_PROJ_PINHOLE and cam is not None
            n_rows = (cam.image_height if pin else proj.height) - row_begin
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_projection_rays_device(
            self._h, C.byref(proj), C.byref(cam) if cam is not None else None, seed, s_i, s_j,
            row_begin, n_rows, C.c_void_p(rays_ptr), C.c_void_p(stream or None),
            C.byref(st) if st is not None else None))
        return st

    def ao_rays_device(self, primary_ptr: int, hits_ptr: int, n: int, out_ptr: int, k: int,
                       seed: int = 1, radius: float = float("inf"), tmin: float = 1e-4,
                       stream: int = 0, stats: bool = False):
        """Asynchronous rt_ao_rays_device: the k-th AO batch of n primary rays and their records
        into n rt_ray records at out_ptr (which may be primary_ptr)."""
        ap = RtAoParams(seed, radius, tmin, k, 0)
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_ao_rays_device(
            self._h, C.byref(ap), C.c_void_p(primary_ptr), C.c_void_p(hits_ptr), n,
            C.c_void_p(out_ptr), C.c_void_p(stream or None),
            C.byref(st) if st is not None else None))
        return st

    def ao_accumulate_device(self, occ_ptr: int, n: int, sums_ptr: int, channels: int = 3,
                             flags: int = 0, stream: int = 0, stats: bool = False):
        """Asynchronous rt_ao_accumulate_device: every 0 byte of the n at occ_ptr adds 1 to the
        `channels` floats of its ray at sums_ptr (RT_FLAG_OVERWRITE: replaces them)."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_ao_accumulate_device(
            self._h, C.c_void_p(occ_ptr), n, channels, flags, C.c_void_p(sums_ptr),
            C.c_void_p(stream or None), C.byref(st) if st is not None else None))
        return st

    def ambient_occlusion_device(self, scene: "DeviceScene", params: RtAoFrameParams,
                                 primary_ptr: int, n: int, sums_ptr: int, hits_ptr: int = 0,
                                 stream: int = 0, stats: bool = False):
        """Asynchronous rt_ambient_occlusion_device: per ray the number of unoccluded directions
        of params.directions, params.channels floats per ray at sums_ptr; the primaries' records
        at hits_ptr if it is given."""
        st = RtStats() if stats else None
        _check_dev(self._lib.rt_ambient_occlusion_device(
            self._h, scene._h, C.byref(params), C.c_void_p(primary_ptr), n, C.c_void_p(sums_ptr),
            C.c_void_p(hits_ptr or None), C.c_void_p(stream or None),
            C.byref(st) if st is not None else None))
        return st

    def ambient_occlusion(self, scene: "DeviceScene", rays: np.ndarray, K: int, seed: int = 1,
                          radius: float = float("inf"), tmin: float = 1e-4, flags: int = 0,
                          channels: int = 1, chunk_rays: int = 0, want_hits: bool = False,
                          stats: bool = False):
        """Synchronous, host buffers: the AO frame of a RAY_DTYPE array, staged through device
        memory. Returns float32 [n, channels] counts of unoccluded directions out of K (a ray
        that sees no surface: 0); with want_hits also the HIT_DTYPE records, with stats RtStats."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        n = len(rays)
        sums = np.zeros((n, channels), np.float32)
        hits = np.zeros(n if want_hits else 0, HIT_DTYPE)
        st = RtStats()
        if n:
            params = make_ao_frame_params(K, seed, radius, tmin, flags | RT_FLAG_OVERWRITE,
                                          channels, chunk_rays)
            h = _hip()
            if h.hipSetDevice(self.device) != 0:
                raise RtError(RT_ERR_HIP, "hipSetDevice failed")
            sizes = [rays.nbytes, sums.nbytes, hits.nbytes]
            offs = [0, (sizes[0] + 255) & ~255]
            offs.append(offs[1] + ((sizes[1] + 255) & ~255))
            base = C.c_void_p()
            if h.hipMalloc(C.byref(base), offs[2] + max(sizes[2], 256)) != 0:
                raise RtError(RT_ERR_HIP, "hipMalloc of the staging buffer failed")
            try:
                d_rays, d_sums, d_hits = (base.value + o for o in offs)
                if h.hipMemcpy(C.c_void_p(d_rays), rays.ctypes.data, sizes[0], 1) != 0:
                    raise RtError(RT_ERR_HIP, "upload of the rays failed")
                st = self.ambient_occlusion_device(scene, params, d_rays, n, d_sums,
                                                   d_hits if want_hits else 0, stats=True)
                if h.hipMemcpy(sums.ctypes.data, C.c_void_p(d_sums), sizes[1], 2) != 0 or (
                        want_hits and
                        h.hipMemcpy(hits.ctypes.data, C.c_void_p(d_hits), sizes[2], 2) != 0):
                    raise RtError(RT_ERR_HIP, "download of the AO frame failed")
            finally:
                h.hipFree(base)
        res = (sums,) + ((hits,) if want_hits else ()) + ((st,) if stats else ())
        return res[0] if len(res) == 1 else res


def write_ppm(path: str, rgb8: np.ndarray) -> None:
    """P3 text exactly as render.rs:151 + write_color lines."""
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w = a.shape[:2]
    _check_host(host_lib().rth_write_ppm(str(path).encode(), a.ctypes.data, w, h))
