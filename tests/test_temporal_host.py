"""Temporal accumulation, the parts that need no device: the mirror of rt_temporal_params, the
constants and defaults, the argument checks that are made before the handle is read and before any
HIP call (so they answer with no GPU present, given a garbage handle and garbage buffer pointers),
the properties of the reference tests/temporal_ref.py itself, the fragile share of every synthetic
case, and rth_camera_orbit_y."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import surely_rt as rt
import temporal_cases as TC
import temporal_ref as TR

HEADER = (Path(__file__).resolve().parent.parent / "include" / "rt_mi355x.h").read_text()
BOGUS = C.c_void_p(0x1000)  # never dereferenced: the checks come first
BUF = C.c_void_p(0x2000)  # a "buffer" the checks never reach
INF, NAN = float("inf"), float("nan")


def test_params_struct_mirrors_the_header():
    body = re.search(r"typedef struct rt_temporal_params \{(.*?)\} rt_temporal_params;", HEADER,
                     re.S)
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    sizes = {"int32_t": (4, C.c_int32), "uint32_t": (4, C.c_uint32), "float": (4, C.c_float)}
    fields = []  # (type, name), a declaration may name several fields
    for decl in (d.strip() for d in text.split(";")):
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(ty, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in rt.RtTemporalParams._fields_]
    off = 0
    for (ty, name), (_, pty) in zip(fields, rt.RtTemporalParams._fields_):
        size, cty = sizes[ty]
        assert pty is cty and off % size == 0, name  # no padding before any field
        assert getattr(rt.RtTemporalParams, name).offset == off, name
        off += size
    assert off == 32 == C.sizeof(rt.RtTemporalParams)
    assert "rt_temporal_params {   /* 32 bytes, no padding */" in HEADER


def test_flag_constants_match_the_header():
    defs = dict(re.findall(r"#define (RT_TEMPORAL_\w+) (0x[0-9a-fA-F]+)u", HEADER))
    assert defs == {"RT_TEMPORAL_RESET": "0x1", "RT_TEMPORAL_VARIANCE_OF_MEAN": "0x2"}
    for name, value in defs.items():
        assert getattr(rt, name) == int(value, 16), name


def test_defaults_are_the_header_s():
    p = rt.temporal_default_params(33, 17)
    assert (p.width, p.height, p.flags, p.beauty_rows) == (33, 17, 0, 0)
    text = re.search(r"/\* host only: flags 0, beauty_rows 0, max_history (\d+), depth_tol ([\d.]+) "
                     r"and normal_tol ([\d.]+).*?min_weight ([\d.]+) \*/\s*int  "
                     r"rt_temporal_default_params", HEADER, re.S)
    assert text, "the header states the defaults above rt_temporal_default_params"
    want = [np.float32(float(v)) for v in text.groups()]
    assert [p.max_history, p.depth_tol, p.normal_tol, p.min_weight] == want
    # the denoiser's edge widths
    d = rt.denoise_default_params(33, 17, 4)
    assert (p.depth_tol, p.normal_tol) == (d.sigma_depth, d.sigma_normal)
    assert p.min_weight == np.float32(0.01)
    lib = rt.device_lib()
    assert lib.rt_temporal_default_params(33, 17, None) == rt.RT_ERR_INVALID_ARG
    q = rt.RtTemporalParams()
    assert lib.rt_temporal_default_params(0, 17, C.byref(q)) == rt.RT_ERR_INVALID_ARG
    assert lib.rt_temporal_default_params(65536, 32768, C.byref(q)) == rt.RT_ERR_INVALID_ARG


def test_abi_version_is_unchanged():
    assert rt.device_lib().rt_abi_version() == 3
    assert re.search(r"#define RT_ABI_VERSION 3\b", HEADER)


# ------------------------------------------------------------------ argument checks
def _calls():
    lib = rt.device_lib()

    def ref(x):
        return C.byref(x) if x is not None else None

    def device(t, p, cam, b, q, a, ob, oq):
        return lib.rt_temporal_accumulate_device(t, ref(p), ref(cam), b, q, a, ob, oq, None, None,
                                                 None)

    def host(t, p, cam, b, q, a, ob, oq):
        return lib.rt_temporal_accumulate(t, ref(p), ref(cam), b, q, a, ob, oq, None, None)

    return {"rt_temporal_accumulate_device": device, "rt_temporal_accumulate": host}


def _params(**kw):
    p = rt.temporal_default_params(20, 12)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cam(H=12, W=20):
    return TC.camera(H, W)


def test_arguments_are_checked_before_the_handle():
    vom = rt.RT_TEMPORAL_VARIANCE_OF_MEAN
    bad_params = [dict(width=0), dict(width=-3), dict(height=-1),
                  dict(width=65536, height=32768),  # width * height = 2^31
                  dict(width=2 ** 31 - 1, height=2 ** 31 - 1),
                  dict(flags=0x4), dict(flags=0x80000000), dict(flags=rt.RT_TEMPORAL_RESET | 0x10),
                  dict(beauty_rows=-1),
                  dict(max_history=0.5), dict(max_history=0.0), dict(max_history=-2.0),
                  dict(max_history=NAN), dict(max_history=INF),
                  dict(depth_tol=NAN), dict(depth_tol=INF), dict(depth_tol=-INF),
                  dict(normal_tol=NAN), dict(normal_tol=INF),
                  dict(min_weight=NAN), dict(min_weight=INF), dict(min_weight=-0.25),
                  dict(min_weight=1.0), dict(min_weight=2.0)]
    cam = _cam()
    for name, call in _calls().items():
        ok = (BOGUS, _params(), cam, BUF, None, BUF, BUF, None)

        def with_(k, v):
            return ok[:k] + (v,) + ok[k + 1:]
        for k in (0, 1, 2, 3, 5, 6):  # handle, params, camera, beauty, aov, out_beauty
            assert call(*with_(k, None)) == rt.RT_ERR_INVALID_ARG, (name, k)
        for bad in bad_params:
            p = _params(**bad)
            c = cam.copy()
            c.image_width, c.image_height = p.width, p.height  # the size check is not the one met
            assert call(BOGUS, p, c, *ok[3:]) == rt.RT_ERR_INVALID_ARG, (name, bad)
        # m2 and out_m2 together or not at all
        assert call(BOGUS, _params(), cam, BUF, BUF, BUF, BUF, None) == rt.RT_ERR_INVALID_ARG, name
        assert call(BOGUS, _params(), cam, BUF, None, BUF, BUF, BUF) == rt.RT_ERR_INVALID_ARG, name
        # VARIANCE_OF_MEAN: needs m2 and beauty_rows >= 2
        assert call(BOGUS, _params(flags=vom, beauty_rows=2), cam, BUF, None, BUF, BUF,
                    None) == rt.RT_ERR_INVALID_ARG, name
        for rows in (0, 1):
            assert call(BOGUS, _params(flags=vom, beauty_rows=rows), cam, BUF, BUF, BUF, BUF,
                        BUF) == rt.RT_ERR_INVALID_ARG, (name, rows)
        # the camera: another size, a singular or non-finite M
        for H, W in ((12, 21), (11, 20)):
            assert call(*with_(2, _cam(H, W))) == rt.RT_ERR_INVALID_ARG, (name, H, W)
        flat = cam.copy()
        for k in range(3):
            flat.pixel_delta_v[k] = 2.0 * flat.pixel_delta_u[k]
        assert call(*with_(2, flat)) == rt.RT_ERR_INVALID_ARG, name
        for field, value in (("pixel_delta_u", NAN), ("pixel00_loc", INF), ("center", NAN)):
            c = cam.copy()
            getattr(c, field)[1] = value
            assert call(*with_(2, c)) == rt.RT_ERR_INVALID_ARG, (name, field)
    lib = rt.device_lib()
    assert lib.rt_temporal_create(0, None) == rt.RT_ERR_INVALID_ARG
    assert lib.rt_temporal_info(None, (C.c_uint64 * 4)(), 4) == rt.RT_ERR_INVALID_ARG
    assert lib.rt_temporal_info(BOGUS, None, 4) == rt.RT_ERR_INVALID_ARG


def test_an_empty_frame_is_ok_and_reads_nothing():
    cam = _cam()
    cam.image_height = 0
    for name, call in _calls().items():
        assert call(BOGUS, _params(height=0), cam, BUF, None, BUF, BUF, None) == rt.RT_OK, name
        assert call(BOGUS, _params(height=0, flags=rt.RT_TEMPORAL_RESET), cam, BUF, BUF, BUF, BUF,
                    BUF) == rt.RT_OK, name
        wide = cam.copy()
        wide.image_width = 2 ** 31 - 1  # the largest frame the checks let through
        assert call(BOGUS, _params(width=2 ** 31 - 1, height=0), wide, BUF, None, BUF, BUF,
                    None) == rt.RT_OK, name


# ------------------------------------------------------------------ the reference's own properties
@pytest.fixture(scope="module")
def seqs():
    return TC.sequences()


@pytest.mark.parametrize("size", [f"{H}x{W}" for H, W in TC.SIZES])
@pytest.mark.parametrize("variant", list(TC.VARIANTS))
def test_fragile_share_of_the_synthetic_cases(seqs, size, variant):
    """A condition on the inputs, checked on the CPU: at most 1 % of a case's pixels are fragile in
    any frame, and the history is in use (else the case tests nothing)."""
    s = seqs[size]
    m2, vom, kw = TC.VARIANTS[variant]
    ref, p = TR.TemporalRef(), s.params(m2=m2, vom=vom, **kw)
    used = 0
    for k in range(TC.FRAMES):
        r = ref.accumulate(s.cams[k], s.beauty[k], s.aov[k], p, m2=s.m2[k] if m2 else None)
        share = r["fragile"].mean()
        print(f"{size} {variant} frame {k}: fragile {share:.4f}, L > 1 at {np.mean(r['hist_len'] > 1):.3f}")
        assert share <= TR.FRAGILE_SHARE
        if k == 0:
            assert r["copied"].all() and (r["hist_len"] == 1).all()
        else:
            used += int((r["hist_len"] > 1).sum())
    assert used >= 0.5 * (TC.FRAMES - 1) * s.H * s.W  # most of a frame overlaps its predecessor


def test_static_camera_gives_the_running_mean():
    s = TC.Sequence(17, 33, frames=5, seed=7, static=True)
    ref, p = TR.TemporalRef(), s.params(m2=True, max_history=64.0)
    hit = s.aov[0][..., rt.AOV_HITS] > 0
    assert hit.any() and not hit.all()
    for k in range(5):
        r = ref.accumulate(s.cams[k], s.beauty[k], s.aov[k], p, m2=s.m2[k])
        mean = np.mean([b.astype(np.float64) for b in s.beauty[:k + 1]], axis=0)
        mean2 = np.mean([q.astype(np.float64) for q in s.m2[:k + 1]], axis=0)
        assert np.array_equal(r["hist_len"][hit], np.full(hit.sum(), k + 1.0))
        assert np.abs(r["beauty"][hit] - mean[hit]).max() <= 1e-12
        assert np.abs(r["m2"][hit] - mean2[hit]).max() <= 1e-11
        # a miss has no position: it never accumulates
        assert np.array_equal(r["hist_len"][~hit], np.ones((~hit).sum()))
        assert np.array_equal(r["beauty"][~hit], s.beauty[k][~hit].astype(np.float64))
        assert not r["fragile"].any()
    assert ref.info() == dict(frames=5, width=33, height=17, moments=True)


def test_max_history_saturates_into_a_moving_average():
    s = TC.Sequence(17, 33, frames=6, seed=8, static=True)
    ref, p = TR.TemporalRef(), s.params(max_history=3.0)
    hit = s.aov[0][..., rt.AOV_HITS] > 0
    want = None
    for k in range(6):
        r = ref.accumulate(s.cams[k], s.beauty[k], s.aov[k], p)
        L = min(k + 1.0, 3.0)
        b = s.beauty[k].astype(np.float64)
        want = b if k == 0 else (1 - 1 / L) * want + b / L
        assert np.array_equal(r["hist_len"][hit], np.full(hit.sum(), L))
        assert np.abs(r["beauty"][hit] - want[hit]).max() <= 1e-12


def test_half_pixel_shift_of_a_ramp():
    cams, aovs, beauties, expect, full = TC.ramp_shift()
    H, W = full.shape
    ref, p = TR.TemporalRef(), rt.temporal_default_params(W, H)
    ref.accumulate(cams[0], beauties[0], aovs[0], p)
    r = ref.accumulate(cams[1], beauties[1], aovs[1], p)
    assert full.any() and not full.all()
    assert np.array_equal(r["hist_len"][full], np.full(full.sum(), 2.0))
    assert np.abs(r["beauty"][full] - expect[full]).max() <= 1e-6  # the weights are f32
    gone = np.broadcast_to(np.arange(W) + TC.RAMP_K + 0.5 >= W, (H, W))  # no tap in the frame
    assert gone.any() and r["copied"][gone].all()
    assert np.array_equal(r["beauty"][gone], beauties[1][gone].astype(np.float64))


def test_reset_size_change_and_invalid_pixels_in_the_reference():
    s = TC.Sequence(17, 33, frames=3, seed=9, static=True)
    ref, p = TR.TemporalRef(), s.params()
    b1 = s.beauty[1].copy()
    b1[5, 7, 1], b1[6, 8, 0] = np.nan, np.inf
    ref.accumulate(s.cams[0], s.beauty[0], s.aov[0], p)
    r = ref.accumulate(s.cams[1], b1, s.aov[1], p)
    assert r["hist_len"][5, 7] == 0 and r["hist_len"][6, 8] == 0
    assert np.array_equal(TR.bits(r["beauty"][5, 7]), TR.bits(b1[5, 7]))
    r = ref.accumulate(s.cams[2], s.beauty[2], s.aov[2], p)
    assert r["hist_len"][5, 7] == 1 and r["copied"][5, 7]  # the NaN pixel was no one's tap
    assert np.isfinite(r["beauty"]).all()
    r = ref.accumulate(s.cams[2], s.beauty[2], s.aov[2], s.params(flags=rt.RT_TEMPORAL_RESET))
    assert r["copied"].all() and ref.info()["frames"] == 1
    t = TC.Sequence(3, 5, frames=1)
    r = ref.accumulate(t.cams[0], t.beauty[0], t.aov[0], t.params())
    assert r["copied"].all() and ref.info() == dict(frames=1, width=5, height=3, moments=False)


# ------------------------------------------------------------------ rth_camera_orbit_y
def _fields(cam):
    return {f: np.array(getattr(cam, f)[:]) for f in
            ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v", "defocus_disk_u",
             "defocus_disk_v")}


def test_orbit_helper():
    cam = rt.camera_new(1.5, 48, 16, 8, 40.0, (278, 278, -800), (270, 250, 0), (0, 1, 0), 0.6,
                        10.0, (0.1, 0.2, 0.3))
    pivot = np.array([277.5, 120.0, 281.25])
    same = rt.camera_orbit_y(cam, pivot, 0.0)
    assert bytes(same) == bytes(cam)  # a bitwise copy
    there = rt.camera_orbit_y(cam, pivot, 17.0)
    back = rt.camera_orbit_y(there, pivot, -17.0)
    assert bytes(there) != bytes(cam)
    for f, v in _fields(cam).items():
        scale = max(1.0, np.abs(v).max())
        assert np.abs(_fields(back)[f] - v).max() <= 1e-12 * scale, f
    # what does not turn stays bitwise
    for f in ("image_width", "image_height", "samples_per_pixel", "sqrt_spp", "max_depth",
              "recip_sqrt_spp", "defocus_angle"):
        assert getattr(there, f) == getattr(cam, f), f
    assert there.background[:] == cam.background[:]
    a, b = _fields(cam), _fields(there)
    # the distance to the pivot and the height are kept; vectors keep their length
    for f in ("center", "pixel00_loc"):
        assert abs(np.linalg.norm(a[f] - pivot) - np.linalg.norm(b[f] - pivot)) <= 1e-12 * 1e3
        assert a[f][1] == b[f][1]
    for f in ("pixel_delta_u", "pixel_delta_v", "defocus_disk_u", "defocus_disk_v"):
        assert abs(np.linalg.norm(a[f]) - np.linalg.norm(b[f])) <= 1e-15 + 1e-12 * np.linalg.norm(a[f])
    # the pivot projects to the same pixel at the same ray parameter
    s0, x0, y0 = TR.project(cam, pivot)
    s1, x1, y1 = TR.project(there, pivot)
    assert abs(s0 - s1) <= 1e-12 * abs(s0) and abs(x0 - x1) <= 1e-9 and abs(y0 - y1) <= 1e-9
    # RotateY's sense: +90 degrees takes +z to +x
    q = rt.camera_orbit_y(cam, (0, 0, 0), 90.0)
    c = np.array(cam.center[:])
    assert np.abs(np.array(q.center[:]) - np.array([c[2], c[1], -c[0]])).max() <= 1e-9
