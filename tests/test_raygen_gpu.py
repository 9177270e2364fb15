"""The ray generators on the device (rt_projection_rays_device, rt_ao_rays_device,
rt_ao_accumulate_device, rt_ambient_occlusion_device; include/rt_mi355x.h) on the GPU, against the
host generators of rt_host.h, which are the definition.

Bitwise: pinhole and ortho rays; of the other kinds and of the AO rays every field that takes no
sin, cos, atan2 or hypot; the accumulation; the driver against its own steps issued through the
public entry points. Within DIR_BOUND: the panorama, fisheye and AO directions, where the device
math library's f64 functions stand against glibc's.

DIR_BOUND. The largest |dir_dev - dir_host| per component over tests 2 and 3 (every frame, band,
stratum, scene and dir_index below), measured on an MI355X against the host generators, is
MEASURED_MAX; the bound asserted is four times that (other r1, r2 and angle values than these),
capped at 1e-12 (a wrong draw order, axis or sign shows at 1e-3 or more)."""
import ctypes as C
import functools

import numpy as np
import pytest

import surely_rt as rt
import variant_scenes as VS
from hip_buf import DevBuf, Stream, hip

pytestmark = pytest.mark.gpu

MEASURED_MAX = 4.441e-16  # 2^-51, in the fisheye frames; panorama 2.220e-16, AO rays 2.220e-16
DIR_BOUND = min(4 * MEASURED_MAX, 1e-12)
SEED = 7
_seen = {"max": 0.0}  # the largest direction difference of this run, printed by every test


class RawBuf:
    """A device buffer of raw bytes (hipMalloc is 256-byte aligned: rt_ray and rt_hit ask for 16)."""

    def __init__(self, nbytes: int, init: np.ndarray | None = None, fill: int = 0xA5):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        assert hip().hipSetDevice(0) == 0
        assert hip().hipMalloc(C.byref(p), max(self.nbytes, 16)) == 0
        self.ptr = p.value
        self.upload(np.full(self.nbytes, fill, np.uint8) if init is None else init)

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a).view(np.uint8).ravel()
        assert a.nbytes == self.nbytes
        if self.nbytes:
            assert hip().hipMemcpy(C.c_void_p(self.ptr), a.ctypes.data, self.nbytes, 1) == 0

    def download(self, dtype=np.uint8) -> np.ndarray:
        hip().hipDeviceSynchronize()
        out = np.empty(self.nbytes, np.uint8)
        if self.nbytes:
            assert hip().hipMemcpy(out.ctypes.data, C.c_void_p(self.ptr), self.nbytes, 2) == 0
        return out.view(dtype)

    def free(self):
        if self.ptr:
            hip().hipFree(C.c_void_p(self.ptr))
            self.ptr = None


def _bytes(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def _same_fields(a, b, fields, what):
    for f in fields:
        assert _bytes(a[f]) == _bytes(b[f]), (what, f, np.nonzero(a[f] != b[f])[0][:8])


def _dir_diff(a, b, what):
    d = float(np.abs(a["dir"] - b["dir"]).max()) if len(a) else 0.0
    _seen["max"] = max(_seen["max"], d)
    print(f"{what}: max |dir_dev - dir_host| = {d:.3e} (run max {_seen['max']:.3e}, "
          f"bound {DIR_BOUND:.3e})")
    assert d <= DIR_BOUND, (what, d)


# ---------------------------------------------------------------- projections
FRAMES = [(20, 12), (1, 1), (65, 1)]
STRATA = [(0, 0), (2, 1)]
VIEW = dict(origin=(0.3, 2.0, 9.0), forward=(-0.3, -1.2, -9.0), up=(0.1, 1.0, 0.0))


def _bands(H):
    return [(0, H)] + ([(5, 4), (11, 1)] if H == 12 else [])


def _pinhole_cam(W, H):
    _, cam = rt.preset_blob("cornell_box", width=W, spp=9, aspect=W / H)
    assert (cam.image_width, cam.image_height, cam.sqrt_spp) == (W, H, 3)
    return cam


def _device_vs_host(gen, kind, W, H, fov=0.0):
    """[(what, device band, host band)] over the strata and the bands of one frame."""
    cam = _pinhole_cam(W, H) if kind == "pinhole" else None
    pr = rt.make_projection(kind, width=W, height=H, sqrt_spp=3, fov=fov, **VIEW)
    out = []
    for s_i, s_j in STRATA:
        host = rt.projection_rays(kind, seed=SEED, s_i=s_i, s_j=s_j, cam=cam, width=W, height=H,
                                  sqrt_spp=3, fov=fov, **VIEW)
        assert len(host) == W * H
        for row_begin, n_rows in _bands(H):
            buf = RawBuf(n_rows * W * 80 + 80)  # one record of slack: it must stay untouched
            try:
                st = gen.projection_rays_device(pr, buf.ptr, seed=SEED, s_i=s_i, s_j=s_j,
                                                row_begin=row_begin, n_rows=n_rows, cam=cam,
                                                stats=True)
                got = buf.download()
            finally:
                buf.free()
            assert (st.samples, st.launches, st.out_bytes) == (n_rows * W, 1, n_rows * W * 80)
            assert np.all(got[n_rows * W * 80:] == 0xA5), "wrote past the band"
            what = f"{kind} {W}x{H} stratum ({s_i},{s_j}) rows {row_begin}+{n_rows}"
            out.append((what, got[:n_rows * W * 80].view(rt.RAY_DTYPE),
                        host[row_begin * W:(row_begin + n_rows) * W]))
    return out


@pytest.mark.parametrize("kind", ["pinhole", "ortho"])
def test_pinhole_and_ortho_rays_are_the_hosts_bit_for_bit(gpu_available, kind):
    gen = rt.RayGen()
    try:
        for W, H in FRAMES:
            for what, dev, host in _device_vs_host(gen, kind, W, H, fov=3.5):
                bad = np.nonzero(dev.view(np.uint8).reshape(-1, 80) !=
                                 host.view(np.uint8).reshape(-1, 80))[0]
                assert len(bad) == 0, (what, bad[:8])
    finally:
        gen.close()


@pytest.mark.parametrize("kind,fov", [("panorama", 0.0), ("fisheye", 400.0)])
def test_panorama_and_fisheye_rays(gpu_available, kind, fov):
    gen = rt.RayGen()
    try:
        outside = 0
        for W, H in FRAMES:
            for what, dev, host in _device_vs_host(gen, kind, W, H, fov=fov):
                _same_fields(dev, host, ("origin", "time", "tmin", "tmax", "pixel", "sample"), what)
                zero_d, zero_h = (dev["dir"] == 0).all(1), (host["dir"] == 0).all(1)
                assert np.array_equal(zero_d, zero_h), (what, np.nonzero(zero_d != zero_h)[0][:8])
                assert _bytes(dev["dir"][zero_d]) == _bytes(host["dir"][zero_d]), what
                outside += int(zero_h.sum())
                _dir_diff(dev, host, what)
        # fov 400: the corners of the 20 x 12 frame lie outside the sphere, its centre inside
        assert (outside > 0) == (kind == "fisheye")
    finally:
        gen.close()


# ---------------------------------------------------------------- scenes and primaries
def _pixel_centre_rays(cam):
    """The rays of rt_render_cli --pick / --ao: through the pixel centres, no jitter, time 0."""
    W, H = cam.image_width, cam.image_height
    c, p00 = np.array(cam.center), np.array(cam.pixel00_loc)
    du, dv = np.array(cam.pixel_delta_u), np.array(cam.pixel_delta_v)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d = p00 + x.reshape(-1, 1) * du + y.reshape(-1, 1) * dv - c
    return rt.make_rays(np.broadcast_to(c, d.shape), d, pixel=np.arange(W * H, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(blob, 16 x 16 pixel-centre primaries). "spheres": the first BVH row of variant_scenes
    without a medium (balls under a BVH, a floor and a lamp quad)."""
    if name == "cornell_box":
        blob, cam = rt.preset_blob("cornell_box", width=16, spp=1)
    else:
        key = next(k for k in VS.parse_rows() if k[0] == 0 and k[2] == 1)
        blob = VS.build(key)
        cam = rt.camera_new(1.0, 16, 1, 6, 27.0, (0.3, 2.0, 9.0), (0.0, 0.8, 0.0), (0, 1, 0), 0.0,
                            0.0, VS.BACKGROUND)
    assert (cam.image_width, cam.image_height) == (16, 16)
    return blob, _pixel_centre_rays(cam)


def _with_misses_and_invalid(primary):
    """+ five rays that leave the scene (backwards and up) and two invalid rays."""
    extra = primary[[0, 50, 100, 150, 200, 7, 8]].copy()
    extra["dir"][:5] = -extra["dir"][:5]
    extra["dir"][:5, 1] = np.abs(extra["dir"][:5, 1]) + 10.0
    extra["dir"][5] = 0.0
    extra["origin"][6, 1] = np.nan
    extra["pixel"] = 1000 + np.arange(7)
    extra["time"] = np.linspace(0.1, 0.7, 7)
    return np.concatenate([primary, extra])


# ---------------------------------------------------------------- AO rays
@pytest.mark.parametrize("name", ["cornell_box", "spheres"])
def test_ao_rays_against_the_host_generator(gpu_available, name):
    blob, primary = _scene(name)
    primary = _with_misses_and_invalid(primary)
    n = len(primary)
    assert n == 263  # four waves and a 7-lane tail
    ds, gen = rt.DeviceScene(blob), rt.RayGen()
    d_prim, d_hits = RawBuf(n * 80, primary), RawBuf(n * 80)
    d_out, d_inplace = RawBuf(n * 80 + 80), RawBuf(n * 80, primary)
    try:
        ds.query_device(d_prim.ptr, n, d_hits.ptr, seed=SEED)  # one record query
        hits = d_hits.download(rt.HIT_DTYPE)
        surface = hits["hit"] == 1
        assert np.array_equal(hits["hit"][-7:], [0, 0, 0, 0, 0, -1, -1]) and surface.sum() > 100
        if name == "spheres":  # both arms of Onb::build_from_w's |w.x| > 0.9
            wx = np.abs(hits["normal"][surface, 0] / np.linalg.norm(hits["normal"][surface], axis=1))
            assert (wx > 0.9).any() and (wx <= 0.9).any() and ((wx > 0.05) & (wx <= 0.9)).any()
        for k in (0, 5):
            want = rt.ao_rays(primary, hits, k, seed=SEED, radius=150.0, tmin=1e-3)
            st = gen.ao_rays_device(d_prim.ptr, d_hits.ptr, n, d_out.ptr, k, seed=SEED,
                                    radius=150.0, tmin=1e-3, stats=True)
            raw = d_out.download()
            assert np.all(raw[n * 80:] == 0xA5), "wrote past the batch"
            got = raw[:n * 80].view(rt.RAY_DTYPE)
            assert (st.samples, st.launches, st.out_bytes) == (n, 1, n * 80)
            what = f"AO rays {name} dir_index {k}"
            _same_fields(got, want, ("origin", "time", "tmin", "tmax", "pixel", "sample"), what)
            assert np.all(got["sample"] == k) and np.all(got["tmax"] == 150.0)
            for f in ("origin", "dir"):  # no surface: all zero, bit for bit
                assert _bytes(got[f][~surface]) == bytes(24 * int((~surface).sum())), (what, f)
                assert _bytes(want[f][~surface]) == bytes(24 * int((~surface).sum()))
            _dir_diff(got[surface], want[surface], what)
            # in place: out_dev == primary_dev
            d_inplace.upload(primary)
            gen.ao_rays_device(d_inplace.ptr, d_hits.ptr, n, d_inplace.ptr, k, seed=SEED,
                               radius=150.0, tmin=1e-3)
            assert _bytes(d_inplace.download()) == _bytes(raw[:n * 80]), what
    finally:
        for b in (d_prim, d_hits, d_out, d_inplace):
            b.free()
        gen.close()
        ds.close()


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize("channels", [1, 3])
def test_accumulate_counts_the_zero_bytes(gpu_available, channels):
    n = 64 * 3 + 5
    rng = np.random.default_rng(11)
    occ = [np.array([0, 1, 255], np.uint8)[rng.integers(0, 3, n)] for _ in range(3)]
    assert all(len(set(o.tolist())) == 3 for o in occ)
    gen = rt.RayGen()
    d_occ = RawBuf(n + 3)  # an odd size: the bytes need no alignment
    sums = DevBuf((n + 1, channels), init=np.full((n + 1, channels), 7.0, np.float32))
    try:
        want = np.full((n, channels), 7.0, np.float32)
        for call, o in enumerate(occ):
            d_occ.upload(np.concatenate([o, np.zeros(3, np.uint8)]))
            flags = rt.RT_FLAG_OVERWRITE if call == 0 else 0
            st = gen.ao_accumulate_device(d_occ.ptr, n, sums.ptr, channels, flags, stats=True)
            add = (o == 0).astype(np.float32)[:, None]
            want = (np.float32(0.0) if call == 0 else want) + np.repeat(add, channels, 1)
            got = sums.download()
            assert _bytes(got[:n]) == _bytes(want.astype(np.float32)), call
            assert np.all(got[n] == 7.0), "wrote past the last ray"
            assert (st.samples, st.launches, st.out_bytes) == (n, 1, n * channels * 4)
        assert want.min() >= 0 and want.max() <= 3 and len(np.unique(want)) >= 3
    finally:
        d_occ.free()
        sums.free()
        gen.close()


# ---------------------------------------------------------------- the driver
def _compose(ds, gen, d_prim, n, K, channels, flags, radius, start):
    """The driver's steps issued one by one through the public entry points -> (sums, hits)."""
    d_hits, d_ao, d_occ = RawBuf(n * 80), RawBuf(n * 80), RawBuf(n)
    sums = DevBuf((n, channels), init=start)
    bvh = flags & rt.RT_FLAG_REFERENCE_BVH
    try:
        ds.query_device(d_prim.ptr, n, d_hits.ptr, seed=SEED, flags=bvh)
        for k in range(K):
            gen.ao_rays_device(d_prim.ptr, d_hits.ptr, n, d_ao.ptr, k, seed=SEED, radius=radius)
            ds.query_device(d_ao.ptr, n, d_occ.ptr, seed=SEED, flags=bvh, occlusion=True,
                            any_hit=True)
            over = rt.RT_FLAG_OVERWRITE if k == 0 and flags & rt.RT_FLAG_OVERWRITE else 0
            gen.ao_accumulate_device(d_occ.ptr, n, sums.ptr, channels, over)
        return sums.download(), d_hits.download()
    finally:
        for b in (d_hits, d_ao, d_occ, sums):
            b.free()


def _drive(ds, gen, d_prim, n, K, channels, flags, radius, start, chunk=0, want_hits=True,
           stream=0):
    d_hits = RawBuf(n * 80) if want_hits else None
    sums = DevBuf((n, channels), init=start)
    try:
        fp = rt.make_ao_frame_params(K, seed=SEED, radius=radius, flags=flags, channels=channels,
                                     chunk_rays=chunk)
        st = gen.ambient_occlusion_device(ds, fp, d_prim.ptr, n, sums.ptr,
                                          d_hits.ptr if want_hits else 0, stream=stream,
                                          stats=not stream)
        if stream:
            assert hip().hipStreamSynchronize(C.c_void_p(stream)) == 0
        return sums.download(), d_hits.download() if want_hits else None, st
    finally:
        sums.free()
        if d_hits:
            d_hits.free()


@pytest.mark.parametrize("name", ["cornell_box", "spheres"])
def test_the_driver_is_the_composition_of_its_steps(gpu_available, name):
    blob, primary = _scene(name)
    primary = _with_misses_and_invalid(primary)
    n, chunk = len(primary), 64 * 3 + 5  # two chunks: 197 + 66
    OVER, BVH = rt.RT_FLAG_OVERWRITE, rt.RT_FLAG_REFERENCE_BVH
    ds, gen = rt.DeviceScene(blob), rt.RayGen()
    d_prim = RawBuf(n * 80, primary)
    other = Stream()
    try:
        for K, channels, flags in ((1, 3, OVER), (5, 1, OVER), (5, 3, 0), (5, 3, OVER | BVH)):
            start = np.full((n, channels), 2.0, np.float32)
            want_s, want_h = _compose(ds, gen, d_prim, n, K, channels, flags, 150.0, start)
            what = (name, K, channels, flags)
            surface = want_h.view(rt.HIT_DTYPE)["hit"] == 1
            base = 0.0 if flags & OVER else 2.0
            assert np.all(want_s[~surface] == base) and want_s.max() <= base + K, what
            assert K == 1 or len(np.unique(want_s[surface])) > 2, what  # some of every count
            got_s, got_h, st = _drive(ds, gen, d_prim, n, K, channels, flags, 150.0, start)
            assert _bytes(got_s) == _bytes(want_s) and _bytes(got_h) == _bytes(want_h), what
            assert (st.samples, st.launches) == (n * K, 1 + 3 * K), what
            assert st.out_bytes == n * channels * 4 + n * 80 and st.ms_kernel > 0.0, what
            # chunks with a ragged seam, the records kept in the workspace, another stream
            got_s, got_h, st = _drive(ds, gen, d_prim, n, K, channels, flags, 150.0, start, chunk)
            assert _bytes(got_s) == _bytes(want_s) and _bytes(got_h) == _bytes(want_h), what
            assert (st.launches, st.out_bytes) == (2 * (1 + 3 * K), n * channels * 4 + n * 80)
            got_s, _, st = _drive(ds, gen, d_prim, n, K, channels, flags, 150.0, start, chunk,
                                  want_hits=False)
            assert _bytes(got_s) == _bytes(want_s) and st.out_bytes == n * channels * 4, what
            got_s, got_h, _ = _drive(ds, gen, d_prim, n, K, channels, flags, 150.0, start,
                                     stream=other.handle)
            assert _bytes(got_s) == _bytes(want_s) and _bytes(got_h) == _bytes(want_h), what
        # the reference BVH walk gives the same frame
        a = _drive(ds, gen, d_prim, n, 5, 3, OVER, 150.0, None)
        b = _drive(ds, gen, d_prim, n, 5, 3, OVER | BVH, 150.0, None)
        assert _bytes(a[0]) == _bytes(b[0]) and _bytes(a[1]) == _bytes(b[1])
        # no rays: nothing is touched
        start = np.full((n, 3), 2.0, np.float32)
        sums, d_hits = DevBuf((n, 3), init=start), RawBuf(n * 80)
        try:
            fp = rt.make_ao_frame_params(5, seed=SEED)
            assert gen.ambient_occlusion_device(ds, fp, d_prim.ptr, 0, sums.ptr, d_hits.ptr) is None
            st = gen.ambient_occlusion_device(ds, fp, d_prim.ptr, 0, sums.ptr, d_hits.ptr,
                                              stats=True)
            assert (st.samples, st.launches, st.out_bytes) == (0, 0, 0)
            assert np.all(sums.download() == 2.0) and np.all(d_hits.download() == 0xA5)
        finally:
            sums.free()
            d_hits.free()
    finally:
        other.destroy()
        d_prim.free()
        gen.close()
        ds.close()


def test_two_calls_of_one_handle_on_two_streams(gpu_available):
    """The second call's stream waits for the first call's use of the workspace: both frames are
    what each call gives alone, checked after both streams are synchronised."""
    blob, primary = _scene("spheres")
    n = len(primary)
    ds, gen = rt.DeviceScene(blob), rt.RayGen()
    d_prim = RawBuf(n * 80, primary)
    s1, s2 = Stream(), Stream()
    sums = [DevBuf((n, 1)), DevBuf((n, 1))]
    try:
        fps = [rt.make_ao_frame_params(K, seed=SEED, radius=r, channels=1, chunk_rays=100)
               for K, r in ((5, 150.0), (3, 2.0))]
        alone = [_drive(ds, gen, d_prim, n, K, 1, rt.RT_FLAG_OVERWRITE, r, None, 100)[0]
                 for K, r in ((5, 150.0), (3, 2.0))]
        assert _bytes(alone[0]) != _bytes(alone[1])
        for fp, out, s in zip(fps, sums, (s1, s2)):
            assert gen.ambient_occlusion_device(ds, fp, d_prim.ptr, n, out.ptr,
                                                stream=s.handle) is None
        s1.sync()
        s2.sync()
        for out, want in zip(sums, alone):
            assert _bytes(out.download()) == _bytes(want)
    finally:
        for b in sums + [d_prim]:
            b.free()
        s1.destroy()
        s2.destroy()
        gen.close()
        ds.close()


# ---------------------------------------------------------------- the host pipeline
def _host_pipeline(ds, primary, K, radius):
    """rt_render_cli --ao as it runs without --device-rays: rth_ao_rays, host-buffer queries and
    a count on the host."""
    hits = ds.query(primary, seed=SEED)
    count = np.zeros(len(primary), np.float32)
    for k in range(K):
        batch = rt.ao_rays(primary, hits, k, seed=SEED, radius=radius)
        count += ds.query(batch, seed=SEED, occlusion=True, any_hit=True) == 0
    return count, hits["hit"] == 1


@pytest.mark.parametrize("name", ["cornell_box", "spheres"])
def test_the_driver_against_the_host_pipeline(gpu_available, name):
    """The two pipelines take sin and cos from different libraries, so a grazing AO ray may flip:
    at most 2 % of the pixels with a surface may differ, by at most one count each. The host
    pipeline against itself differs in none."""
    blob, primary = _scene(name)
    K, radius = 5, 150.0
    ds, gen = rt.DeviceScene(blob), rt.RayGen()
    try:
        host, surface = _host_pipeline(ds, primary, K, radius)
        again, _ = _host_pipeline(ds, primary, K, radius)
        dev, hits = gen.ambient_occlusion(ds, primary, K, seed=SEED, radius=radius, want_hits=True)
    finally:
        gen.close()
        ds.close()
    assert np.array_equal(host, again)
    assert np.array_equal(hits["hit"] == 1, surface) and surface.sum() > 100
    assert dev.shape == (len(primary), 1) and np.all(dev[~surface] == 0) and np.all(host[~surface] == 0)
    diff = np.abs(dev[:, 0] - host)
    differ = int((diff[surface] != 0).sum())
    print(f"AO frame {name} 16 x 16, K = {K}: {differ} of {int(surface.sum())} surface pixels differ "
          f"from the host pipeline (largest difference {diff.max():.0f})")
    assert differ <= 0.02 * surface.sum() and diff.max() <= 1.0
