"""Ray renders (rt_render_rays*, include/rt_mi355x.h) and the host ray generator
(rth_projection_rays, include/rt_host.h), the part that needs no GPU: rt_rays_params against the
header text, the exported symbols, every argument check (made before the scene is read: the scene
handle here is a dummy pointer), the generator's four projections, and the scene-specialised ray
kernels of the three benchmark scenes, generated and compiled for gfx950."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
from test_query_host import _c_fields

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "rt_mi355x.h").read_text()


def test_rays_params_mirrors_the_header():
    fields = _c_fields("rt_rays_params")
    assert sum(n for _, n in fields) == 56  # no padding: the fields alone fill it
    st = rt.RtRaysParams
    assert C.sizeof(st) == 56
    assert [(f, getattr(st, f).size) for f, _ in st._fields_] == fields
    assert [getattr(st, f).offset for f, _ in st._fields_] == \
        list(np.cumsum([0] + [n for _, n in fields])[:-1])
    assert re.search(r"#define RT_RAYS_STREAM_TIME 0x1u", HEADER) and rt.RT_RAYS_STREAM_TIME == 1
    assert re.search(r"#define RT_RAYS_MAX_SKIP 16\b", HEADER) and rt.RT_RAYS_MAX_SKIP == 16
    assert "#define RT_ABI_VERSION 3" in HEADER
    host = (REPO / "include" / "rt_host.h").read_text()
    assert C.sizeof(rt.RthProjection) == 96
    for k, name in enumerate(("PINHOLE", "ORTHO", "PANORAMA", "FISHEYE")):
        assert re.search(rf"#define RTH_PROJ_{name} {k}\b", host)
        assert getattr(rt, "RTH_PROJ_" + name) == k


def test_symbols_are_exported():
    so = C.CDLL(str(REPO / "build" / "librtmi355x.so"))
    for n in ("rt_render_rays_device", "rt_render_rays"):
        assert hasattr(so, n), n
    assert hasattr(C.CDLL(str(REPO / "build" / "librthost.so")), "rth_projection_rays")


def _call(fn, scene, rp, rays, n, out, device):
    lib = rt.device_lib()
    st = rt.RtStats()
    args = [C.c_void_p(scene), C.byref(rp) if rp is not None else None, C.c_void_p(rays), n,
            C.c_void_p(out)]
    if device:
        args.append(None)
    return getattr(lib, fn)(*args, C.byref(st)), st


def _rp(**kw):
    p = rt.make_rays_params(seed=1, sqrt_paths=kw.pop("S", 2), max_depth=kw.pop("depth", 5),
                            flags=kw.pop("flags", rt.RT_FLAG_OVERWRITE),
                            stream_skip=kw.pop("skip", 3), stream_time=kw.pop("st", True))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("fn,device", [("rt_render_rays_device", True), ("rt_render_rays", False)])
def test_argument_checks_run_before_the_scene_is_read(fn, device):
    """A dummy non-null scene pointer: a check that read the scene would fault the test."""
    dummy = 0x10
    rays = np.zeros(5, rt.RAY_DTYPE)  # 80-byte records: rays[k] stays 16-byte aligned
    out = np.zeros(15, np.float32)
    r, o = rays.ctypes.data, out.ctypes.data
    assert r % 16 == 0
    ok = _rp()
    allf = rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_INTERPRETER | rt.RT_FLAG_REFERENCE_BVH | \
        rt.RT_FLAG_SEMANTICS_REFERENCE
    bad = [
        (0, ok, r, 4, o), (dummy, None, r, 4, o), (dummy, ok, 0, 4, o), (dummy, ok, r, 4, 0),
        (dummy, ok, r, 1 << 31, o), (dummy, ok, r, 1 << 40, o),
        (dummy, _rp(flags=rt.RT_FLAG_COUNT_OPS), r, 4, o),
        (dummy, _rp(flags=allf | rt.RT_FLAG_COUNT_OPS), r, 4, o),
        (dummy, _rp(flags=0x20), r, 4, o), (dummy, _rp(flags=0x80000000), r, 4, o),
        (dummy, _rp(mode=2), r, 4, o), (dummy, _rp(mode=0x80000001), r, 4, o),
        (dummy, _rp(_pad0=1), r, 4, o),
        (dummy, _rp(S=0), r, 4, o), (dummy, _rp(S=-3), r, 4, o), (dummy, _rp(depth=-1), r, 4, o),
        (dummy, _rp(skip=rt.RT_RAYS_MAX_SKIP + 1), r, 4, o), (dummy, _rp(skip=0xffffffff), r, 4, o),
        (dummy, _rp(skip=0, st=True), r, 4, o),
        (dummy, ok, r + 8, 4, o), (dummy, ok, r + 4, 4, o),
    ]
    for scene, rp, rr, n, oo in bad:
        rc, st = _call(fn, scene, rp, rr, n, oo, device)
        assert rc == rt.RT_ERR_INVALID_ARG, (scene, rp and (rp.flags, rp.mode, rp.sqrt_paths,
                                                            rp.stream_skip), rr - r, n)
        assert st.launches == 0 and st.samples == 0
    for rp in (_rp(S=32769), _rp(depth=0x1000000)):
        rc, st = _call(fn, dummy, rp, r, 4, o, device)
        assert rc == rt.RT_ERR_UNSUPPORTED and st.launches == 0
    # an invalid argument is reported before an unsupported one
    assert _call(fn, dummy, _rp(S=32769, _pad0=1), r, 4, o, device)[0] == rt.RT_ERR_INVALID_ARG
    assert not out.any()
    # n_rays == 0 returns RT_OK and touches nothing, the scene included (checked with every legal
    # flag, a non-finite background, the largest skip, skip 0 without the time bit, S and depth at
    # their limits: a real call would read the dummy scene)
    good = [ok, _rp(flags=allf), _rp(flags=0), _rp(skip=rt.RT_RAYS_MAX_SKIP), _rp(skip=0, st=False),
            _rp(S=32768, depth=0xffffff), _rp(depth=0), _rp(skip=1, st=True)]
    nanbg = _rp()
    nanbg.background[0], nanbg.background[1] = float("nan"), float("inf")
    for rp in good + [nanbg]:
        rc, st = _call(fn, dummy, rp, r, 0, o, device)
        assert rc == rt.RT_OK and st.launches == 0
    assert not out.any()


# ---------------------------------------------------------------- the host ray generator
def test_pinhole_rays_equal_the_oracle_camera_ray():
    """20 x 12, S = 2: origin, direction and draw 3 (the time) bit for bit."""
    _, cam = rt.preset_blob("cornell_box", width=20, spp=4)
    cam = cam.copy()
    cam.image_height = 12
    assert cam.sqrt_spp == 2 and cam.defocus_angle <= 0.0
    for seed in (1, 0x123456789ABCDEF):
        for s_j in range(2):
            for s_i in range(2):
                rays = rt.projection_rays("pinhole", seed=seed, s_i=s_i, s_j=s_j, cam=cam)
                assert rays.shape == (240,)
                want = np.array([O.camera_ray(cam, seed, i, j, s_i, s_j)
                                 for j in range(12) for i in range(20)])
                got = np.concatenate([rays["origin"], rays["dir"], rays["time"][:, None]], axis=1)
                assert got.tobytes() == want.tobytes(), (seed, s_i, s_j)
                assert rays["pixel"].tolist() == list(range(240))
                assert (rays["sample"] == s_j * 2 + s_i).all()
                assert (rays["tmin"] == 1e-4).all() and np.isinf(rays["tmax"]).all()


def _frame(kind, W, H, S=1, s_i=0, s_j=0, seed=3, **kw):
    kw.setdefault("origin", (0.25, 1.25, 4.5))
    kw.setdefault("forward", (0.0, 0.0, -2.0))  # not unit: the generator normalises the frame
    kw.setdefault("up", (0.0, 3.0, 0.0))
    return rt.projection_rays(kind, seed=seed, s_i=s_i, s_j=s_j, width=W, height=H, sqrt_spp=S, **kw)


@pytest.mark.parametrize("kind,fov", [("ortho", 4.0), ("panorama", 0.0), ("fisheye", 180.0)])
def test_projection_norms_and_determinism(kind, fov):
    W, H = 16, 8
    a = _frame(kind, W, H, S=2, s_i=1, s_j=0, fov=fov)
    b = _frame(kind, W, H, S=2, s_i=1, s_j=0, fov=fov)
    assert a.tobytes() == b.tobytes()  # deterministic
    assert a.tobytes() != _frame(kind, W, H, S=2, s_i=0, s_j=1, fov=fov).tobytes()
    assert a.tobytes() != _frame(kind, W, H, S=2, s_i=1, s_j=0, fov=fov, seed=4).tobytes()
    n = np.linalg.norm(a["dir"], axis=1)
    print(kind, "direction norms", n.min(), n.max())
    unit = np.abs(n - 1.0) <= 4e-16 * 4  # unit length to a few roundings
    if kind == "fisheye":  # 16 x 8 at 180 degrees: the corners pass theta = pi (documented: zero)
        assert np.all(unit | (n == 0)) and unit.sum() >= W * H - 8
    else:
        assert np.all(unit)
    assert a["pixel"].tolist() == list(range(W * H)) and (a["sample"] == 1).all()
    assert (a["tmin"] == 1e-4).all() and np.isinf(a["tmax"]).all()
    assert ((a["time"] >= 0) & (a["time"] < 1)).all()
    if kind == "ortho":
        assert np.all(a["dir"] == np.array([0.0, 0.0, -1.0]))
    else:
        assert np.all(a["origin"] == np.array([0.25, 1.25, 4.5]))


def _centre(kind, fov, W=9, H=5):
    """Odd sizes, S = 1: the centre pixel's sample lies within half a pixel of the frame centre."""
    f = _frame(kind, W, H, fov=fov).reshape(H, W)
    return f, f[H // 2, W // 2]


def test_ortho_corners_and_centre():
    f, c = _centre("ortho", 4.0)
    # view volume 4 high and 4 * 9 / 5 wide about the origin, x to the right (f x up), y up
    assert np.all(np.abs(c["origin"] - (0.25, 1.25, 4.5)) <= (0.5 * 7.2 / 9, 0.5 * 4 / 5, 0))
    o = f["origin"] - np.array([0.25, 1.25, 4.5])
    assert np.all(o[..., 2] == 0)
    assert -3.6 <= o[0, 0, 0] < -3.6 + 0.8 and 3.6 - 0.8 <= o[0, -1, 0] < 3.6   # left, right
    assert 2.0 - 0.8 < o[0, 0, 1] <= 2.0 and -2.0 <= o[-1, 0, 1] < -2.0 + 0.8   # top, bottom
    assert np.all(np.diff(o[..., 0], axis=1) > 0) and np.all(np.diff(o[..., 1], axis=0) < 0)


def test_panorama_corners_and_centre():
    W, H = 9, 5
    f, c = _centre("panorama", 0.0, W, H)
    d = f["dir"]
    # the centre looks along forward (0, 0, -1) within half a pixel: 20 deg of longitude, 18 of latitude
    assert c["dir"][2] < -np.cos(np.radians(20)) * np.cos(np.radians(18)) - 1e-12 + 0.12
    assert abs(c["dir"][0]) <= np.sin(np.radians(20)) and abs(c["dir"][1]) <= np.sin(np.radians(18))
    assert np.all(d[0, :, 1] > np.sin(np.radians(90 - 36)))    # top row looks up
    assert np.all(d[-1, :, 1] < -np.sin(np.radians(90 - 36)))  # bottom row down
    # the left and right edges meet behind the viewer (+z), left column to the left (-x)
    assert d[H // 2, 0, 2] > 0 and d[H // 2, -1, 2] > 0
    assert d[H // 2, 0, 0] < 0 < d[H // 2, -1, 0]


def test_fisheye_corners_and_centre():
    W, H = 9, 5
    f, c = _centre("fisheye", 180.0, W, H)
    d = f["dir"]
    # centre: within half a pixel of the axis; theta = rho * 90 deg, rho <= hypot(1, 1) / 5
    assert c["dir"][2] <= -np.cos(np.radians(90 * np.hypot(1, 1) / 5))
    # the short side spans the fov: the top-centre pixel lies within a pixel of 90 deg off axis, upwards
    assert d[0, W // 2, 1] > np.cos(np.radians(90 * 2 / 5)) - 0.2 and d[0, W // 2, 1] > 0.7
    # corners: rho up to hypot(9, 5) / 5 = 2.06 > 2, i.e. theta may pass 180 deg: all-zero (invalid)
    # directions are what the header documents for such pixels, every other one is unit length
    n = np.linalg.norm(d, axis=2)
    assert np.all((np.abs(n - 1) <= 2e-15) | (n == 0))
    assert n[H // 2].all() and n[:, W // 2].all()
    wide = _frame("fisheye", W, H, fov=350.0).reshape(H, W)
    assert (np.linalg.norm(wide["dir"], axis=2) == 0).any()
    # left of centre looks to the left (-x), and behind the image plane (+z) past 90 deg
    assert d[H // 2, 0, 0] < 0 and d[H // 2, 0, 2] > 0


def test_projection_argument_checks():
    lib = rt.host_lib()
    out = np.zeros(4, rt.RAY_DTYPE)
    pr = rt.RthProjection()
    pr.kind, pr.width, pr.height, pr.sqrt_spp, pr.fov = rt.RTH_PROJ_ORTHO, 2, 2, 1, 1.0
    pr.forward[2], pr.up[1] = -1.0, 1.0
    call = lambda p, s_i=0, s_j=0, cam=None: lib.rth_projection_rays(  # noqa: E731
        C.byref(p), cam, 1, s_i, s_j, out.ctypes.data)
    assert call(pr) == 0
    assert call(pr, s_i=1) == -1 and call(pr, s_j=-1) == -1
    for field, v in (("kind", 7), ("kind", -1), ("width", 0), ("sqrt_spp", 0), ("fov", 0.0),
                     ("fov", float("nan"))):
        q = rt.RthProjection.from_buffer_copy(pr)
        setattr(q, field, v)
        assert call(q) == -1, (field, v)
    q = rt.RthProjection.from_buffer_copy(pr)
    q.up[1], q.up[2] = 0.0, 5.0  # parallel to forward
    assert call(q) == -1
    q = rt.RthProjection.from_buffer_copy(pr)
    q.kind = rt.RTH_PROJ_PINHOLE
    assert call(q) == -1  # no camera
    assert lib.rth_projection_rays(None, None, 1, 0, 0, out.ctypes.data) == -1


# ---------------------------------------------------------------- scene-specialised ray kernels
@pytest.mark.parametrize("name", ["cornell_box", "cornell_smoke", "final_scene"])
def test_ray_variant_of_the_specialised_kernel_compiles(name, monkeypatch):
    """RT_JIT_CHECK_RAYS=1: rt_jit_check also generates and compiles the ray variant for gfx950
    and returns that kernel's source, which instantiates trace_body with kLaunchRays."""
    monkeypatch.setenv("RT_JIT_CHECK_RAYS", "1")
    blob, _ = rt.preset_blob(name, width=32, spp=4)
    state, src = rt.jit_check(blob)
    assert state == 1, src[:400]
    assert "rt_trace_jit" in src and re.search(r"TravGen, kLaunchRays>\(P\)", src)
    monkeypatch.delenv("RT_JIT_CHECK_RAYS")
    state, plain = rt.jit_check(blob)
    assert state == 1 and "kLaunchRays" not in plain
