"""rt_render_rays* on the GPU (include/rt_mi355x.h, "ray renders").

The yardstick is the library's own pinhole render through a DEGENERATE camera: image_width 1, both
pixel deltas zero, no lens, center = o, pixel00_loc = o + d', row_begin = k. get_ray then forms
exactly the ray (o, pixel00_loc - o) for every sample, with the stream of pixel key k (the two
jitter draws are taken and multiply zero deltas), so rt_render / oracle_render of that one-pixel
"image" at sqrt_spp = S is what rt_render_rays must give for the ray (o, d, pixel = k, sample = 0)
with stream_skip = 3 and RT_RAYS_STREAM_TIME: bit for bit against the device, within
test_gpu_parity.TOL per path against the f64 oracle. d = pixel00_loc - center is formed here in
numpy, so the ray handed to rt_render_rays holds the very bits the kernels compute.

The internal limit the large batch must exceed: a pinhole render call is split into sub-calls of
rts::kRowsPerCall = 32760 rows (lane item keys hold the row in 15 bits); a ray batch is laid out
8 rays wide, so 32760 * 8 = 262,080 rays is where such a split would fall. Ray launches key their
items by ray index instead and are not split; BIG = 300,007 rays lies above it."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
import variant_scenes as V
from adaptive_cases import bits
from hip_buf import DevBuf, Stream
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

OW = rt.RT_FLAG_OVERWRITE
ROWS = V.parse_rows()
IDS = ["".join(map(str, k)) for k in ROWS]
EYE = np.array([0.25, 1.25, 4.5])
HEIGHT = 1 << 20  # the degenerate camera's image_height: every pixel key used here is below it
BIG = 300007
# the variant-scene rows of test 1: flat/staged, BVH, vol+tex+BVH, unstaged flat, both nested rows
ROWS_1 = [(0, 0, 0, 1, 0, 1, 0), (0, 0, 1, 0, 0, 1, 0), (1, 1, 1, 0, 1, 1, 0),
          (0, 0, 0, 0, 0, 1, 0), (1, 1, 0, 0, 1, 1, 2), (1, 1, 1, 0, 1, 1, 2)]
FLAT = (0, 0, 0, 1, 0, 1, 0)
assert all(k in ROWS for k in ROWS_1)


def same(a, b):
    """bit for bit, which includes equal NaN / inf masks"""
    return np.array_equal(bits(a), bits(b))


def exact_rays(origins, dprime, pixel=None, time=0.0):
    """(rays, pixel00_loc): p00 = o + d' rounded once, and the ray's dir = p00 - o, the exact bits
    a degenerate camera's get_ray computes"""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    p00 = o + np.asarray(dprime, np.float64).reshape(-1, 3)
    return rt.make_rays(o, p00 - o, time=time, pixel=pixel, sample=0), p00


def degenerate_cam(o, p00, S, depth, background):
    cam = rt.RtCamera()
    cam.image_width, cam.image_height = 1, HEIGHT
    cam.samples_per_pixel, cam.sqrt_spp, cam.max_depth = S * S, S, depth
    cam.recip_sqrt_spp = 1.0 / S
    for k in range(3):
        cam.center[k], cam.pixel00_loc[k], cam.background[k] = o[k], p00[k], background[k]
    return cam  # zero pixel deltas, no lens


def device_reference(ds, rays, p00, S, depth, seed, background=V.BACKGROUND):
    """One rt_render_device per ray through its degenerate camera, into one buffer"""
    buf = DevBuf((len(rays), 3))
    try:
        for k, r in enumerate(rays):
            cam = degenerate_cam(r["origin"], p00[k], S, depth, background)
            o = rt.make_opts(cam, seed=seed, row_begin=int(r["pixel"]), n_rows=1, flags=OW)
            ds.render_device(cam, o, buf.ptr + 12 * k)
        return buf.download()
    finally:
        buf.free()


def oracle_reference(blob, rays, p00, S, depth, seed, precision, background=V.BACKGROUND):
    """(values [n, 3] f32, op counts [n, 32]) of one oracle_render per ray"""
    out = np.zeros((len(rays), 3), np.float32)
    ops = np.zeros((len(rays), len(rt.OP_NAMES)), np.int64)
    for k, r in enumerate(rays):
        cam = degenerate_cam(r["origin"], p00[k], S, depth, background)
        o = rt.make_opts(cam, seed=seed, row_begin=int(r["pixel"]), n_rows=1)
        a, c = O.render(blob, cam, o, precision=precision, threads=1)
        out[k] = a[0, 0]
        ops[k] = [c[n] for n in rt.OP_NAMES]
    return out, ops


def params(seed, S=1, depth=V.DEPTH, flags=OW, skip=3, stream_time=True, background=V.BACKGROUND):
    return rt.make_rays_params(seed=seed, sqrt_paths=S, max_depth=depth, background=background,
                               flags=flags, stream_skip=skip, stream_time=stream_time)


def panorama(scale=1.5):
    """Test 3's rays: a 16 x 8 equirectangular panorama from EYE looking down -z, directions of
    length 1.5, keyed by pixel = index"""
    g = rt.projection_rays("panorama", seed=3, width=16, height=8, sqrt_spp=1, origin=EYE,
                           forward=(0, 0, -1), up=(0, 1, 0))
    return exact_rays(g["origin"], g["dir"] * scale, pixel=np.arange(128, dtype=np.uint32))


def arbitrary_rays():
    """Test 1's rays: 65 from near EYE towards the balls, the panorama, and probes that start on
    the floor quad (y = -0.3) pointing up; pixel keys spread out, none repeated"""
    rng = np.random.default_rng(7)
    o = EYE + 0.05 * rng.standard_normal((65, 3))
    target = np.array([0.0, 0.6, 0.8]) + rng.uniform(-2.5, 2.5, (65, 3)) * (1.0, 0.5, 1.0)
    a, pa = exact_rays(o, target - o, pixel=1000 + 37 * np.arange(65, dtype=np.uint32))
    b, pb = panorama()
    fo = np.array([[0.4, -0.3, 1.5], [-2.0, -0.3, 2.5], [1.7, -0.3, 0.9], [0.0, -0.3, -1.0]])
    fd = np.array([[0.05, 1.0, 0.02], [0.3, 1.0, -0.2], [0.0, 1.0, 0.0], [-0.1, 0.9, 0.3]])
    c, pc = exact_rays(fo, fd, pixel=700000 + np.arange(4, dtype=np.uint32))
    return np.concatenate([a, b, c]), np.concatenate([pa, pb, pc])


def ran_specialised(ds, key, what):
    """the scene-specialised kernel of the launch just made was the one that ran, except on the two
    nested rows (test_variant_matrix_gpu.py)"""
    state, msg = ds.jit_info()
    print(f"{key}: {what}: jit state {state}: {msg[:200]}")
    if "not launched:" not in msg:
        assert state == (-1 if key[6] else 1), (key, what, state, msg[:2000])


# ---------------------------------------------------------------- 1. arbitrary rays vs rt_render
@pytest.mark.parametrize("key", ROWS_1, ids=["".join(map(str, k)) for k in ROWS_1])
def test_arbitrary_rays_equal_the_degenerate_camera_render(gpu_available, key):
    t0 = time.perf_counter()
    blob = V.build(key)
    rays, p00 = arbitrary_rays()
    assert len(rays) == 65 + 128 + 4 and len(set(rays["pixel"].tolist())) == len(rays)
    ds = rt.DeviceScene(blob)
    try:
        for S in (1, 2, 9):  # 9: two kPoolSi blocks per stratum row
            want = device_reference(ds, rays, p00, S, V.DEPTH, seed=5)
            got, st = ds.render_rays(rays, params(5, S), stats=True)
            ran_specialised(ds, key, f"ray render S={S}")
            assert st.samples == len(rays) * S * S and st.launches >= 1
            nsp = int((~np.isfinite(want)).sum())
            print(f"{key} S={S}: {len(rays)} rays, {nsp} non-finite values, "
                  f"max value {np.nanmax(np.where(np.isfinite(want), want, 0)):.4g}, "
                  f"differing words {(bits(got) != bits(want)).sum()}")
            assert same(got, want), f"S={S}: rt_render_rays vs rt_render, default kernel"
            assert np.count_nonzero(want) > want.size // 2  # the rays do see the scene
            for f, name in ((rt.RT_FLAG_INTERPRETER, "interpreter"),
                            (rt.RT_FLAG_REFERENCE_BVH, "reference BVH")):
                assert same(ds.render_rays(rays, params(5, S, flags=OW | f)), want), (S, name)
    finally:
        ds.close()
    print(f"{key}: test wall time {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- 2. a pinhole frame
def lensless(cam, S):
    c = cam.copy()
    c.defocus_angle = 0.0
    c.sqrt_spp, c.samples_per_pixel, c.recip_sqrt_spp = S, S * S, 1.0 / S
    return c


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("key", ROWS, ids=IDS)
def test_pinhole_frame_equals_rt_render(gpu_available, key):
    blob = V.build(key)
    ds = rt.DeviceScene(blob)
    try:
        cam1 = lensless(V.camera(key, ROWS), 1)
        for seed in (1, 2):
            rays = rt.projection_rays("pinhole", seed=seed, cam=cam1)
            assert len(rays) == 240
            frame, _ = ds.render(cam1, rt.make_opts(cam1, seed=seed, flags=OW))
            got = ds.render_rays(rays, params(seed, 1, depth=cam1.max_depth))
            print(f"{key} seed {seed}: 1 spp, differing words "
                  f"{(bits(got) != bits(frame.reshape(-1, 3))).sum()}")
            assert same(got, frame.reshape(-1, 3)), f"seed {seed}: 1 spp frame"
        # 4 spp as four accumulating passes of one path per ray
        cam2 = lensless(V.camera(key, ROWS), 2)
        frame, _ = ds.render(cam2, rt.make_opts(cam2, seed=1, flags=OW))
        frame = frame.reshape(-1, 3)
        acc = np.zeros((240, 3), np.float32)
        total = np.zeros((240, 3), np.float32)
        for s_j in range(2):
            for s_i in range(2):
                rays = rt.projection_rays("pinhole", seed=1, s_i=s_i, s_j=s_j, cam=cam2)
                one = ds.render_rays(rays, params(1, 1, depth=cam2.max_depth))
                with np.errstate(invalid="ignore"):
                    total = total + one  # f32 arithmetic, in the frame's sample order
                ds.render_rays(rays, params(1, 1, depth=cam2.max_depth, flags=0), rgb=acc)
        for name, x in (("accumulated passes", acc), ("f32 sum of the four samples", total)):
            assert np.array_equal(np.isnan(x), np.isnan(frame)), name
            assert np.array_equal(np.isinf(x), np.isinf(frame)), name
            fin = np.isfinite(frame)
            d = np.abs(x[fin].astype(np.float64) - frame[fin].astype(np.float64)) / ulp32(frame[fin])
            print(f"{key}: {name} vs the 4 spp frame: max {d.max():.2f} ulp")
            assert d.max() <= 2.0, name
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. the f64 oracle
@pytest.mark.parametrize("key", ROWS, ids=IDS)
def test_panorama_against_the_oracle(gpu_available, key):
    t0 = time.perf_counter()
    blob = V.build(key)
    rays, p00 = panorama()
    assert len(rays) == 128
    n = np.linalg.norm(rays["dir"], axis=1)
    assert np.all(np.abs(n - 1.5) < 1e-12)
    ds = rt.DeviceScene(blob)
    try:
        for seed in (1, 2):
            want, ops = oracle_reference(blob, rays, p00, 2, V.DEPTH, seed, 64)
            # the precondition: no path decision of the set hangs on a last bit, so the oracle
            # with fused dot products agrees in op counts and in value
            want_f, ops_f = oracle_reference(blob, rays, p00, 2, V.DEPTH, seed, "64fma")
            assert np.array_equal(ops, ops_f), np.argwhere(ops != ops_f)[:8].tolist()
            assert np.array_equal(np.isnan(want), np.isnan(want_f))
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(want_f))
            assert np.abs(want[fin].astype(np.float64) - want_f[fin]).max() / 4 <= TOL
            got = ds.render_rays(rays, params(seed, 2))
            assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN masks"
            assert np.array_equal(np.isposinf(got), np.isposinf(want)), "+inf masks"
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), "-inf masks"
            d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) / 4
            print(f"{key} seed {seed}: 128 rays x 4 paths, {int((~fin).sum())} non-finite values, "
                  f"max |gpu - oracle| per path {d.max():.3e} (TOL {TOL})")
            assert d.max() <= TOL
    finally:
        ds.close()
    print(f"{key}: test wall time {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- 4. time
def moving_scene():
    sc = rt.Scene(11)
    white = sc.lambertian((0.73, 0.73, 0.73))
    light = sc.diffuse_light((7, 7, 7))
    world = sc.hittable_list(
        sc.quad((-6, -0.3, -6), (12, 0, 0), (0, 0, 12), sc.lambertian((0.5, 0.6, 0.4))),
        sc.sphere_moving((0.0, 0.5, 0.0), (0.6, 1.3, 0.0), 0.8, sc.lambertian((0.7, 0.2, 0.2))),
        sc.sphere((-1.8, 0.5, 0.5), 0.8, white),
        sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light))
    lights = sc.hittable_list(sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light))
    cam = rt.camera_new(5.0 / 3.0, 20, 1, 6, 27.0, (0.3, 2.0, 9.0), (0.0, 0.8, 0.0), (0, 1, 0),
                        0.0, 0.0, V.BACKGROUND)
    return sc.serialize(world, lights), cam


def test_time_of_a_moving_sphere(gpu_available):
    blob, cam = moving_scene()
    assert cam.sqrt_spp == 1 and (cam.image_width, cam.image_height) == (20, 12)
    rays = rt.projection_rays("pinhole", seed=4, cam=cam)
    want7 = np.array([O.camera_ray(cam, 4, i, j, 0, 0) for j in range(12) for i in range(20)])
    assert rays["time"].tobytes() == want7[:, 6].tobytes()  # the oracle camera ray's own time
    ds = rt.DeviceScene(blob)
    try:
        frame, _ = ds.render(cam, rt.make_opts(cam, seed=4, flags=OW))
        frame = frame.reshape(-1, 3)
        own = ds.render_rays(rays, params(4, 1, stream_time=False))
        junk = rays.copy()
        junk["time"] = np.linspace(-1e6, 1e6, len(junk))
        streamed = ds.render_rays(junk, params(4, 1, stream_time=True))
        frozen = ds.render_rays(junk, params(4, 1, stream_time=False))
        print(f"moving sphere: differing words, ray.time {(bits(own) != bits(frame)).sum()}, "
              f"stream time {(bits(streamed) != bits(frame)).sum()}, "
              f"garbage ray.time read {(bits(frozen) != bits(frame)).sum()}")
        assert same(own, frame), "ray.time = the camera ray's time"
        assert same(streamed, frame), "RT_RAYS_STREAM_TIME ignores ray.time"
        assert not same(frozen, frame)  # the time is read: the sphere is elsewhere at +-1e6
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. contract
@pytest.fixture(scope="module")
def flat(gpu_available):
    ds = rt.DeviceScene(V.build(FLAT))
    yield ds
    ds.close()


def probe_rays(n, seed=9, first_pixel=0):
    rng = np.random.default_rng(seed)
    o = EYE + 0.2 * rng.standard_normal((n, 3))
    target = np.array([0.0, 0.6, 0.8]) + rng.uniform(-3, 3, (n, 3)) * (1.0, 0.5, 1.0)
    return exact_rays(o, target - o, pixel=first_pixel + np.arange(n, dtype=np.uint32))[0]


def test_accumulation_depth_zero_and_sizes(flat):
    rays = probe_rays(513)
    whole = flat.render_rays(rays, params(3, 2))
    assert np.isfinite(whole).all() and np.count_nonzero(whole) > whole.size // 2
    # without RT_FLAG_OVERWRITE: (float)((double)old + sum); the f64 sum is not returned, but with
    # old = 0 the rule gives the overwritten value, and a second pass adds the same sum again
    acc = flat.render_rays(rays, params(3, 2, flags=0), rgb=np.zeros((513, 3), np.float32))
    assert same(acc, whole)
    old = np.full((513, 3), 0.375, np.float32)
    acc = flat.render_rays(rays, params(3, 2, flags=0), rgb=old.copy())
    # sum = whole + e with |e| <= ulp(whole) / 2: the f64-add rule bounds the result to the
    # roundings of 0.375 + (whole -+ ulp / 2)
    lo = (0.375 + whole.astype(np.float64) - ulp32(whole) / 2).astype(np.float32)
    hi = (0.375 + whole.astype(np.float64) + ulp32(whole) / 2).astype(np.float32)
    assert np.all((acc >= lo) & (acc <= hi))
    # at S = 1 the sum is one path's radiance, an f32 weight product widened to f64 (rt_kernel.h wt),
    # so the overwritten value IS the sum and the rule can be checked exactly
    one = flat.render_rays(rays, params(3, 1))
    acc1 = flat.render_rays(rays, params(3, 1, flags=0), rgb=old.copy())
    assert same(acc1, (old.astype(np.float64) + one.astype(np.float64)).astype(np.float32))
    zeros = flat.render_rays(rays, params(3, 2, depth=0), rgb=np.full((513, 3), 7.0, np.float32))
    assert not zeros.any(), "max_depth = 0 gives zeros"
    kept = flat.render_rays(rays, params(3, 2, depth=0, flags=0), rgb=np.full((513, 3), 7.0, np.float32))
    assert (kept == 7.0).all()
    for n in (1, 63, 64, 65, 513):
        got, st = flat.render_rays(rays[:n], params(3, 2), stats=True)
        assert same(got, whole[:n]), n
        assert st.samples == n * 4 and st.launches >= 1
    # a permuted batch and a sub-batch give the same records
    perm = np.random.default_rng(1).permutation(513)
    assert same(flat.render_rays(rays[perm], params(3, 2)), whole[perm])
    sub = np.arange(100, 400, 3)
    assert same(flat.render_rays(rays[sub], params(3, 2)), whole[sub])
    # skip 0 without the time bit is a different stream position: other values, same API
    other = flat.render_rays(rays, params(3, 2, skip=0, stream_time=False))
    assert np.isfinite(other).all() and not same(other, whole)


def test_large_batch_equals_its_halves(flat):
    """BIG = 300,007 rays > 32760 * 8 (see the module docstring), S = 1, depth 6"""
    assert BIG > 32760 * 8
    base = probe_rays(4099, seed=21)
    idx = np.arange(BIG) % 4099
    rays = base[idx].copy()
    rays["pixel"] = np.arange(BIG, dtype=np.uint32)
    t0 = time.perf_counter()
    whole, st = flat.render_rays(rays, params(8, 1), stats=True)
    print(f"{BIG} rays: {st.ms_kernel:.2f} ms kernel, {st.launches} launch(es), "
          f"{time.perf_counter() - t0:.2f} s wall")
    assert st.samples == BIG and st.launches == 1
    cut = 150001  # not a multiple of 64: the halves' tiles are other rays than the whole batch's
    a = flat.render_rays(rays[:cut], params(8, 1))
    b = flat.render_rays(rays[cut:], params(8, 1))
    assert same(whole[:cut], a) and same(whole[cut:], b)
    assert np.isfinite(whole).all() and np.count_nonzero(whole) > whole.size // 2
    # the same ray under another pixel key is another stream
    assert not same(whole[:4099], whole[4099:8198])


def test_invalid_rays_get_nan_and_leave_their_neighbours_alone(flat):
    rays = probe_rays(130)
    whole = flat.render_rays(rays, params(3, 2))
    bad = rays.copy()
    bad["origin"][3, 1] = np.nan
    bad["dir"][64, 0] = np.inf
    bad["dir"][65] = 0.0
    bad["dir"][66] = (0.0, -0.0, 0.0)
    bad["time"][129] = np.nan
    bad["origin"][100, 2] = -np.inf
    idx = [3, 64, 65, 66, 100, 129]
    ok = np.setdiff1d(np.arange(130), idx)
    for flags in (OW, 0):
        got = flat.render_rays(bad, params(3, 2, flags=flags), rgb=np.zeros((130, 3), np.float32))
        assert np.isnan(got[idx]).all(), flags
        assert (bits(got[idx]) == 0x7fc00000).all(), "quiet NaN"
        assert same(got[ok], whole[ok]), flags
    # tmin and tmax are not read
    odd = rays.copy()
    odd["tmin"], odd["tmax"] = np.nan, -1.0
    assert same(flat.render_rays(odd, params(3, 2)), whole)


def test_empty_lights_under_reference_semantics(gpu_available):
    blob, _ = rt.preset_blob("quads", width=16, spp=1)
    ds = rt.DeviceScene(blob)
    try:
        rays = rt.make_rays([[0, 0, 9]], [[0, 0, -1]])
        with pytest.raises(rt.RtError) as e:
            ds.render_rays(rays, params(1, 1, flags=OW | rt.RT_FLAG_SEMANTICS_REFERENCE))
        assert e.value.code == rt.RT_ERR_EMPTY_LIGHTS
        assert np.isfinite(ds.render_rays(rays, params(1, 1))).all()
    finally:
        ds.close()


def test_beauty_render_is_unchanged_around_a_ray_render(gpu_available):
    key = (1, 1, 1, 0, 1, 1, 0)
    blob, cam = V.build(key), V.camera(key, ROWS)
    ds = rt.DeviceScene(blob)
    try:
        before, _ = ds.render(cam, rt.make_opts(cam, seed=2, flags=OW))
        ds.render_rays(probe_rays(100), params(2, 3))
        after, _ = ds.render(cam, rt.make_opts(cam, seed=2, flags=OW))
        assert same(before, after)
    finally:
        ds.close()


def test_two_streams_at_once(flat):
    sets = [probe_rays(777, seed=31), probe_rays(1500, seed=32, first_pixel=5000)]
    serial = [flat.render_rays(r, params(6, 2)) for r in sets]
    streams = [Stream(), Stream()]
    bufs = []
    try:
        for r in sets:
            rb = DevBuf((len(r), 20), init=r.view(np.float32).reshape(len(r), 20))
            bufs.append((rb, DevBuf((len(r), 3))))
        for _ in range(3):  # interleaved: each call returns before its kernels finish
            for (rb, ob), r, s in zip(bufs, sets, streams):
                flat.render_rays_device(rb.ptr, len(r), ob.ptr, params(6, 2), stream=s.handle)
        for s in streams:
            s.sync()
        for (rb, ob), want in zip(bufs, serial):
            assert same(ob.download(), want)
    finally:
        for s in streams:
            s.destroy()
        for rb, ob in bufs:
            rb.free()
            ob.free()
