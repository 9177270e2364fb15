"""The device ray generators, the parts that need no device: the mirrors of rt_projection,
rt_ao_params and rt_ao_frame_params, and the argument checks that are made before the handle is
read and before any HIP call (so they answer RT_ERR_INVALID_ARG with no GPU present, given a
garbage handle, a garbage scene and garbage buffer pointers)."""
import ctypes as C
import re
from pathlib import Path

import surely_rt as rt

HEADER = (Path(__file__).resolve().parent.parent / "include" / "rt_mi355x.h").read_text()
BOGUS = C.c_void_p(0x1000)  # a "handle" / "scene": never dereferenced, the checks come first
BUF = C.c_void_p(0x2000)  # a 16-byte aligned "buffer" the checks never reach
ODD = C.c_void_p(0x2008)  # one that is not 16-byte aligned
INF, NAN = float("inf"), float("nan")
INVALID = rt.RT_ERR_INVALID_ARG


def _bad(rc, what):
    assert rc == INVALID, what
    assert rt.device_lib().rt_last_error().decode(), what  # a message goes with the code


def test_struct_sizes_and_layouts():
    assert C.sizeof(rt.RtProjection) == 96 and "96 bytes, the layout of rth_projection" in HEADER
    assert C.sizeof(rt.RtAoParams) == 32 and "32 bytes, the layout of rth_ao_params" in HEADER
    assert C.sizeof(rt.RtAoFrameParams) == 40 and "40 bytes, no padding" in HEADER
    for dev, host in ((rt.RtProjection, rt.RthProjection), (rt.RtAoParams, rt.RthAoParams)):
        assert [n for n, _ in dev._fields_] == [n for n, _ in host._fields_]
        for name, ty in dev._fields_:
            assert getattr(dev, name).offset == getattr(host, name).offset, name
            assert getattr(dev, name).size == getattr(host, name).size, name
    off = 0
    for name, ty in rt.RtAoFrameParams._fields_:  # no padding before any field
        assert getattr(rt.RtAoFrameParams, name).offset == off, name
        off += C.sizeof(ty)
    assert off == 40


def test_frame_params_mirror_the_header():
    body = re.search(r"typedef struct rt_ao_frame_params \{(.*?)\} rt_ao_frame_params;", HEADER,
                     re.S)
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    types = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
    fields = [tuple(d.split()) for d in (d.strip() for d in text.split(";")) if d]
    assert [(n, types[t]) for t, n in fields] == list(rt.RtAoFrameParams._fields_)


def test_projection_constants_match_the_header_and_the_host():
    defs = dict(re.findall(r"#define (RT_PROJ_\w+) (\d+)", HEADER))
    assert len(defs) == 4
    for name, value in defs.items():
        assert getattr(rt, name) == int(value) == getattr(rt, name.replace("RT_", "RTH_")), name


# ---------------------------------------------------------------- rt_projection_rays_device
def _proj(kind="panorama", **kw):
    pr = rt.make_projection(kind, width=20, height=12, sqrt_spp=3, fov=90.0)
    for k, v in kw.items():
        setattr(pr, k, rt._d3(v) if k in ("origin", "forward", "up") else v)
    return pr


def _projection(g, pr, rays, cam=None, s_i=0, s_j=0, row_begin=0, n_rows=12):
    return rt.device_lib().rt_projection_rays_device(
        g, C.byref(pr) if pr is not None else None, C.byref(cam) if cam is not None else None, 7,
        s_i, s_j, row_begin, n_rows, rays, None, None)


def test_projection_arguments_are_checked_before_the_handle():
    _bad(_projection(None, _proj(), BUF), "null handle")
    _bad(_projection(BOGUS, None, BUF), "null projection")
    _bad(_projection(BOGUS, _proj(), None), "null rays")
    _bad(_projection(BOGUS, _proj(), ODD), "misaligned rays")
    _bad(_projection(BOGUS, _proj("pinhole"), BUF), "pinhole without a camera")
    for kind in (-1, 4, 1 << 20):
        _bad(_projection(BOGUS, _proj(kind), BUF), kind)
    bad = [dict(width=0), dict(height=0), dict(sqrt_spp=0), dict(width=-5),
           dict(width=65536, height=32768),  # width * height = 2^31
           dict(forward=(0, 0, 0)), dict(forward=(NAN, 0, 1)), dict(forward=(INF, 0, 0)),
           dict(up=(0, 0, 0)), dict(up=(0, 0, -2)),  # parallel to forward
           dict(origin=(0, NAN, 0)), dict(origin=(INF, 0, 0))]
    for kw in bad:
        _bad(_projection(BOGUS, _proj(**kw), BUF, n_rows=0), kw)
    for kind in ("ortho", "fisheye"):
        for fov in (0.0, -1.0, NAN, INF):
            _bad(_projection(BOGUS, _proj(kind, fov=fov), BUF), (kind, fov))
    for s_i, s_j in ((-1, 0), (3, 0), (0, -1), (0, 3)):
        _bad(_projection(BOGUS, _proj(), BUF, s_i=s_i, s_j=s_j), (s_i, s_j))
    for row_begin, n_rows in ((-1, 1), (0, -1), (0, 13), (12, 1), (5, 8), (2 ** 31 - 1, 2 ** 31 - 1)):
        _bad(_projection(BOGUS, _proj(), BUF, row_begin=row_begin, n_rows=n_rows),
             (row_begin, n_rows))
    # the pinhole's frame is the camera's
    _, cam = rt.preset_blob("cornell_box", width=20, spp=9)
    assert (cam.image_height, cam.sqrt_spp) == (20, 3)
    _bad(_projection(BOGUS, _proj("pinhole"), BUF, cam, s_i=3), "stratum outside the camera's")
    _bad(_projection(BOGUS, _proj("pinhole"), BUF, cam, row_begin=12, n_rows=9), "past the camera's rows")


def test_an_empty_band_is_ok_and_reads_nothing():
    for row_begin in (0, 5, 12):
        assert _projection(BOGUS, _proj(), BUF, row_begin=row_begin, n_rows=0) == rt.RT_OK
    # the panorama reads no fov
    assert _projection(BOGUS, _proj(fov=NAN), BUF, n_rows=0) == rt.RT_OK
    _, cam = rt.preset_blob("cornell_box", width=20, spp=9)
    assert _projection(BOGUS, _proj("pinhole", width=0, height=0, sqrt_spp=0), BUF, cam,
                       row_begin=20, n_rows=0) == rt.RT_OK


# ---------------------------------------------------------------- rt_ao_rays_device
def _ao(g, ap, primary, hits, n, out):
    return rt.device_lib().rt_ao_rays_device(g, C.byref(ap) if ap is not None else None, primary,
                                             hits, n, out, None, None)


BAD_INTERVALS = [dict(tmin=NAN), dict(tmin=INF), dict(tmin=-INF), dict(tmin=-1e-9),
                 dict(radius=NAN), dict(radius=1e-4), dict(radius=0.0), dict(radius=-INF),
                 dict(tmin=2.0, radius=1.0)]


def test_ao_rays_arguments_are_checked_before_the_handle():
    good = lambda **kw: rt.RtAoParams(**{**dict(seed=1, radius=INF, tmin=1e-4, dir_index=0,  # noqa: E731
                                                 _pad0=0), **kw})
    _bad(_ao(None, good(), BUF, BUF, 4, BUF), "null handle")
    _bad(_ao(BOGUS, None, BUF, BUF, 4, BUF), "null params")
    _bad(_ao(BOGUS, good(), None, BUF, 4, BUF), "null primary")
    _bad(_ao(BOGUS, good(), BUF, None, 4, BUF), "null hits")
    _bad(_ao(BOGUS, good(), BUF, BUF, 4, None), "null out")
    _bad(_ao(BOGUS, good(), ODD, BUF, 4, BUF), "misaligned primary")
    _bad(_ao(BOGUS, good(), BUF, ODD, 4, BUF), "misaligned hits")
    _bad(_ao(BOGUS, good(), BUF, BUF, 4, ODD), "misaligned out")
    _bad(_ao(BOGUS, good(), BUF, BUF, 2 ** 31, BUF), "n = 2^31")
    _bad(_ao(BOGUS, good(_pad0=1), BUF, BUF, 4, BUF), "_pad0")
    for kw in BAD_INTERVALS:
        _bad(_ao(BOGUS, good(**kw), BUF, BUF, 4, BUF), kw)
        _bad(_ao(BOGUS, good(**kw), BUF, BUF, 0, BUF), kw)  # checked even for no rays
    assert _ao(BOGUS, good(), BUF, BUF, 0, BUF) == rt.RT_OK
    assert _ao(BOGUS, good(radius=1.0, tmin=0.0, dir_index=2 ** 32 - 1), BUF, BUF, 0, BUF) == rt.RT_OK


# ---------------------------------------------------------------- rt_ao_accumulate_device
def _acc(g, occ, n, channels, flags, sums):
    return rt.device_lib().rt_ao_accumulate_device(g, occ, n, channels, flags, sums, None, None)


def test_accumulate_arguments_are_checked_before_the_handle():
    _bad(_acc(None, BUF, 4, 3, 0, BUF), "null handle")
    _bad(_acc(BOGUS, None, 4, 3, 0, BUF), "null occ")
    _bad(_acc(BOGUS, BUF, 4, 3, 0, None), "null sums")
    _bad(_acc(BOGUS, BUF, 2 ** 31, 3, 0, BUF), "n = 2^31")
    for channels in (0, 2, 4, 2 ** 32 - 1):
        _bad(_acc(BOGUS, BUF, 4, channels, 0, BUF), channels)
    for flags in (rt.RT_FLAG_REFERENCE_BVH, rt.RT_FLAG_COUNT_OPS, 0x80000000,
                  rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_INTERPRETER):
        _bad(_acc(BOGUS, BUF, 4, 1, flags, BUF), flags)
    for channels in (1, 3):
        for flags in (0, rt.RT_FLAG_OVERWRITE):
            assert _acc(BOGUS, ODD, 0, channels, flags, BUF) == rt.RT_OK  # bytes need no alignment


# ---------------------------------------------------------------- rt_ambient_occlusion_device
def _frame(g, sc, fp, primary, n, sums, hits=None):
    return rt.device_lib().rt_ambient_occlusion_device(
        g, sc, C.byref(fp) if fp is not None else None, primary, n, sums, hits, None, None)


def test_ao_frame_arguments_are_checked_before_the_handle_and_the_scene():
    def good(**kw):
        fp = rt.make_ao_frame_params(4)
        for k, v in kw.items():
            setattr(fp, k, v)
        return fp

    _bad(_frame(None, BOGUS, good(), BUF, 4, BUF), "null handle")
    _bad(_frame(BOGUS, None, good(), BUF, 4, BUF), "null scene")
    _bad(_frame(BOGUS, BOGUS, None, BUF, 4, BUF), "null params")
    _bad(_frame(BOGUS, BOGUS, good(), None, 4, BUF), "null primary")
    _bad(_frame(BOGUS, BOGUS, good(), BUF, 4, None), "null sums")
    _bad(_frame(BOGUS, BOGUS, good(), ODD, 4, BUF), "misaligned primary")
    _bad(_frame(BOGUS, BOGUS, good(), BUF, 4, BUF, ODD), "misaligned hits_out")
    _bad(_frame(BOGUS, BOGUS, good(), BUF, 2 ** 31, BUF), "n = 2^31")
    _bad(_frame(BOGUS, BOGUS, good(directions=0), BUF, 4, BUF), "directions == 0")
    for channels in (0, 2, 4):
        _bad(_frame(BOGUS, BOGUS, good(channels=channels), BUF, 4, BUF), channels)
    for flags in (rt.RT_FLAG_COUNT_OPS, rt.RT_FLAG_INTERPRETER, rt.RT_FLAG_SEMANTICS_REFERENCE,
                  0x80000000, rt.RT_FLAG_OVERWRITE | 0x20):
        _bad(_frame(BOGUS, BOGUS, good(flags=flags), BUF, 4, BUF), flags)
    for kw in BAD_INTERVALS:
        _bad(_frame(BOGUS, BOGUS, good(**kw), BUF, 4, BUF), kw)
    for flags in (0, rt.RT_FLAG_OVERWRITE, rt.RT_FLAG_REFERENCE_BVH,
                  rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_REFERENCE_BVH):
        for channels in (1, 3):
            fp = good(flags=flags, channels=channels, chunk_rays=197)
            assert _frame(BOGUS, BOGUS, fp, BUF, 0, BUF) == rt.RT_OK
            assert _frame(BOGUS, BOGUS, fp, BUF, 0, BUF, BUF) == rt.RT_OK


def test_create_checks_its_out_pointer_and_the_abi_version_is_unchanged():
    assert rt.device_lib().rt_raygen_create(0, None) == INVALID
    rt.device_lib().rt_raygen_destroy(None)  # a null handle is ignored
    assert rt.device_lib().rt_abi_version() == 3
    assert re.search(r"#define RT_ABI_VERSION 3\b", HEADER)
