"""The variance-guided a-trous denoiser on the GPU (rt_denoise_var / rt_denoise_var_device) against
denoise_var_ref, the f64 numpy restatement of the filter in include/rt_mi355x.h.

Error measure: for `out`, denoise_ref.mean_error (max |got - ref| / max(1, |ref|) on the mean
radiance); for `var_out` the same relative form on the variance itself. The device computes in f32
(the per-pixel variance estimate alone in f64), the reference in f64; the project's per-pixel
parity bound, 1e-4, is the ceiling. The rule of tests/test_denoise_gpu.py: MEASURED_MAX is the
largest figure over every case of this file in one run on an MI355X, and the asserted BOUND is 8 x
that, rounded up to one significant digit, for run-to-run and compiler drift. Measured: 6.313e-7
(`var_out` of the random 61x64 frame at 8 levels, demodulated; `out` reaches 6.0e-7 on the smooth
frames, the end-to-end cornell_box frame 2.1e-7), so BOUND = 6e-6. Every test prints its own
figure.

All frames are at most 64x64; the tile of the kernels is 32 wide and 8 high."""
import subprocess
import threading

import numpy as np
import pytest

import surely_rt as rt
from denoise_ref import clipped_rmse, mean_error
from denoise_var_ref import denoise_var_ref, moments_from_rows, var_error
from hip_buf import DevBuf, Stream
from test_moments_host import property_figures, property_frame

pytestmark = pytest.mark.gpu

MEASURED_MAX = 6.313e-7
BOUND = 6e-6
assert 8 * MEASURED_MAX <= BOUND < 1e-4

SIZES = [(1, 1), (3, 5), (17, 33), (64, 64), (61, 64)]  # (H, W)
LEVELS = [1, 2, 3, 5, 8]
ROWS = [2, 4, 7]


def guides_random(rng, H, W, A):
    """The AOVs of tests/test_denoise_gpu.py's `synth` recipe."""
    hits = rng.choice([0.0, A / 2, A], size=(H, W), p=[0.15, 0.15, 0.7])
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    aov = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
    aov[..., rt.AOV_HITS] = hits
    aov[..., rt.AOV_T] = rng.uniform(1.0, 10.0, (H, W)) * hits
    aov[..., rt.AOV_NORMAL:rt.AOV_NORMAL + 3] = n * hits[..., None]
    aov[..., rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] = rng.uniform(0.05, 1.0, (H, W, 3)) * A
    aov[..., rt.AOV_EMISSION:rt.AOV_EMISSION + 3] = rng.uniform(0.0, 0.2, (H, W, 3)) * A
    aov[..., rt.AOV_MATID] = rng.integers(-1, 5, (H, W))
    return aov


def synth(H, W, seed, n=4, B=4.0, A=4.0):
    """Seeded random frame: n row totals per pixel, uniform in [0, 2] B / n (S and Q are formed
    from them, so Q >= S^2 / n up to their f32 rounding), random guides."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(0.0, 2.0, (n, H, W, 3)) * (B / n)
    beauty, m2 = moments_from_rows(rows)
    return beauty, m2, guides_random(rng, H, W, A)


def smooth(H, W, seed, n=4, B=4.0, A=4.0):
    """A frame the filter does average: smooth colour plus noise of sd 0.15 per pixel (0.15 sqrt(n)
    per row mean), one surface (the AOVs of test_denoise_gpu.py's `smooth`)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.3 * np.sin(xx / 7.0)[..., None] * np.array([1.0, 0.7, 0.4])
    rows = (base + rng.normal(0, 0.15 * np.sqrt(n), (n, H, W, 3))) * (B / n)
    beauty, m2 = moments_from_rows(rows)
    aov = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
    aov[..., rt.AOV_HITS] = A
    aov[..., rt.AOV_T] = (5.0 + 0.01 * yy) * A
    aov[..., rt.AOV_NORMAL + 1] = A
    aov[..., rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] = np.array([0.7, 0.6, 0.5]) * A
    return beauty, m2, aov


def params(H, W, levels=5, n=4, B=4.0, A=4.0, **kw):
    p = rt.denoise_var_default_params(W, H, B, n, A)
    p.levels = levels
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def dn(gpu_available):
    d = rt.Denoiser(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(dn, beauty, m2, aov, p, what):
    got, var, st = dn.denoise_var(beauty, m2, aov, p, var_out=True, stats=True)
    ref, vref, valid = denoise_var_ref(beauty, m2, aov, p)
    m, mv = mean_error(got, ref, p), var_error(var, vref)
    print(f"{what}: out {m:.3e}, var_out {mv:.3e}")
    assert m <= BOUND and mv <= BOUND, (what, m, mv)
    assert (var[~valid] == 0).all() and (var >= 0).all()
    assert st.samples == p.width * p.height and st.launches == 2 + p.levels
    assert st.out_bytes == got.nbytes + var.nbytes and not any(st.ops[:])
    # without var_out: the same frame, 12 bytes per pixel written
    got2, st2 = dn.denoise_var(beauty, m2, aov, p, stats=True)
    assert np.array_equal(bits(got2), bits(got)) and st2.out_bytes == got.nbytes
    return got, var, ref


# ---------------------------------------------------------------- 1. synthetic frames
@pytest.mark.parametrize("demod", [True, False])
@pytest.mark.parametrize("H,W", SIZES)
def test_synthetic_frames_against_the_reference(dn, H, W, demod):
    for k, levels in enumerate(LEVELS):
        n = ROWS[(k + H) % 3]
        for name, make in (("random", synth), ("smooth", smooth)):
            beauty, m2, aov = make(H, W, seed=100 * H + W, n=n)
            p = params(H, W, levels, n=n, flags=rt.DENOISE_DEMODULATE if demod else 0)
            got, var, _ = check(dn, beauty, m2, aov, p,
                                f"{name} {H}x{W} L{levels} n={n} demod={demod}")
            assert np.isfinite(got).all()


@pytest.mark.parametrize("n", ROWS)
def test_every_row_count(dn, n):
    H, W = 17, 33
    for make in (synth, smooth):
        beauty, m2, aov = make(H, W, seed=7 + n, n=n)
        check(dn, beauty, m2, aov, params(H, W, 3, n=n), f"{make.__name__} n={n}")


@pytest.mark.parametrize("sigma", [0.0, -1.0])
def test_colour_term_switched_off(dn, sigma):
    H, W = 33, 17
    for make in (synth, smooth):
        beauty, m2, aov = make(H, W, seed=9)
        p = params(H, W, 3, sigma_color=sigma)
        got, _, ref = check(dn, beauty, m2, aov, p, f"{make.__name__} sigma_color={sigma}")
        if make is smooth:  # the switch is not ignored
            full, _, _ = denoise_var_ref(beauty, m2, aov, params(H, W, 3))
            assert mean_error(full, ref, p) > 100 * BOUND


# ---------------------------------------------------------------- 2. non-finite pixels
def test_non_finite_pixels_pass_through_bit_for_bit(dn):
    H, W = 24, 64
    beauty, m2, aov = smooth(H, W, seed=3)
    # interior, the frame's corners, and the four sides of the corner where four 32x8 tiles meet:
    # non-finite beauty sums and non-finite second moments alternate
    spots = {(13, 20): np.nan, (0, 0): np.inf, (H - 1, W - 1): -np.inf, (8, 32): np.inf,
             (7, 31): np.nan, (7, 32): np.inf, (8, 31): np.nan}
    for k, ((y, x), v) in enumerate(spots.items()):
        (beauty if k % 2 == 0 else m2)[y, x, k % 3] = v
    bad = ~(np.isfinite(beauty).all(axis=-1) & np.isfinite(m2).all(axis=-1))
    assert int(bad.sum()) == len(spots)
    for demod in (rt.DENOISE_DEMODULATE, 0):
        p = params(H, W, 4, flags=demod)
        got, var, _ = check(dn, beauty, m2, aov, p, f"non-finite flags={demod}")
        assert np.array_equal(bits(got[bad]), bits(beauty[bad]))
        assert np.array_equal(~np.isfinite(got), ~np.isfinite(beauty))
        assert (var[bad] == 0).all() and np.isfinite(var).all()
        assert mean_error(got, beauty, p) > 100 * BOUND  # the neighbours did average


# ---------------------------------------------------------------- 3. bitwise invariances
def _device_call(dn, beauty, m2, aov, p, stream=0, in_place=False):
    b, q, a = DevBuf(beauty.shape, init=beauty), DevBuf(m2.shape, init=m2), \
        DevBuf(aov.shape, init=aov)
    o = b if in_place else DevBuf(beauty.shape, init=np.full(beauty.shape, 7.25, np.float32))
    v = DevBuf(beauty.shape[:2], init=np.full(beauty.shape[:2], 7.25, np.float32))
    try:
        dn.denoise_var_device(p, b.ptr, q.ptr, a.ptr, o.ptr, v.ptr, stream=stream)
        out, var = o.download(), v.download()
        assert np.array_equal(bits(q.download()), bits(m2))
        assert np.array_equal(bits(a.download()), bits(aov))
        if not in_place:
            assert np.array_equal(bits(b.download()), bits(beauty))
        return out, var
    finally:
        for d in {b, q, a, o, v}:
            d.free()


def test_repeatable_device_host_and_in_place_bitwise(dn):
    H, W = 33, 17
    beauty, m2, aov = smooth(H, W, seed=11)
    beauty[5, 5, 1] = np.nan
    p = params(H, W, 3)
    one, var1 = dn.denoise_var(beauty, m2, aov, p, var_out=True)
    two, var2 = dn.denoise_var(beauty, m2, aov, p, var_out=True)
    dev, var3 = _device_call(dn, beauty, m2, aov, p)
    inp, var4 = _device_call(dn, beauty, m2, aov, p, in_place=True)
    for other, v in ((two, var2), (dev, var3), (inp, var4)):
        assert np.array_equal(bits(one), bits(other)) and np.array_equal(bits(var1), bits(v))


def test_two_streams_through_one_handle_bitwise(dn):
    frames = [smooth(64, 64, seed=21), synth(61, 64, seed=22)]
    ps = [params(64, 64, 5), params(61, 64, 3)]
    serial = [dn.denoise_var(*f, p) for f, p in zip(frames, ps)]
    streams = [Stream(0), Stream(0)]
    bufs = [tuple(DevBuf(x.shape, init=x) for x in f) + (DevBuf(f[0].shape),) for f in frames]
    try:
        for _ in range(3):  # the calls share one workspace: each must wait for the one before
            for (b, q, a, o), p, s in zip(bufs, ps, streams):
                dn.denoise_var_device(p, b.ptr, q.ptr, a.ptr, o.ptr, stream=s.handle)
        for s in streams:
            s.sync()
        for (b, q, a, o), want in zip(bufs, serial):
            assert np.array_equal(bits(o.download()), bits(want))
    finally:
        for s in streams:
            s.destroy()
        for t in bufs:
            for d in t:
                d.free()


def test_two_handles_in_two_threads_bitwise(dn):
    frames = [smooth(64, 64, seed=31), synth(33, 17, seed=32)]
    ps = [params(64, 64, 4), params(33, 17, 2)]
    serial = [dn.denoise_var(*f, p) for f, p in zip(frames, ps)]
    got, errs = [None, None], []

    def work(k):
        try:
            d = rt.Denoiser(0)
            try:
                for _ in range(3):
                    got[k] = d.denoise_var(*frames[k], ps[k])
            finally:
                d.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for g, want in zip(got, serial):
        assert np.array_equal(bits(g), bits(want))


@pytest.mark.parametrize("first", ["plain", "var"])
def test_interleaved_with_the_plain_filter_on_one_handle_bitwise(dn, first):
    """rt_denoise and rt_denoise_var share the handle's workspace (48 or 64 B per pixel for the
    plain filter, 64 for this one): growing it in either order, and reusing it, changes no bit."""
    small, large = synth(3, 5, seed=41), smooth(64, 64, seed=42)
    calls = {"plain1": lambda d: d.denoise(small[0], small[2],
                                           _plain(3, 5, 1)),      # 48 B per pixel
             "plainL": lambda d: d.denoise(large[0], large[2], _plain(64, 64, 5)),
             "var1": lambda d: d.denoise_var(*small, params(3, 5, 1)),
             "varL": lambda d: d.denoise_var(*large, params(64, 64, 5))}
    alone = {}
    for k, f in calls.items():
        h = rt.Denoiser(0)
        try:
            alone[k] = f(h)
        finally:
            h.close()
    order = ["plain1", "var1", "plainL", "varL"] if first == "plain" else \
        ["var1", "plain1", "varL", "plainL"]
    fresh = rt.Denoiser(0)
    try:
        for k in order + order[::-1]:
            assert np.array_equal(bits(calls[k](fresh)), bits(alone[k])), k
    finally:
        fresh.close()
    for k in calls:  # and on the module's long-lived handle
        assert np.array_equal(bits(calls[k](dn)), bits(alone[k])), k


def _plain(H, W, levels):
    p = rt.denoise_default_params(W, H, 4.0, 4.0)
    p.levels = levels
    return p


# ---------------------------------------------------------------- 4. the property
def test_smooths_noise_and_keeps_converged_texture(dn):
    """tests/test_moments_host.py's frame (where the reference alone is held to the same three
    conditions): the variance-guided filter keeps the zero-variance stripes within BOUND of the
    input and at least halves the noisy half's deviation; the plain filter with default params
    moves the stripes by more than 100 x BOUND."""
    beauty, m2, aov, pv, pd = property_frame()
    got, var, _ = check(dn, beauty, m2, aov, pv, "property frame")
    plain = dn.denoise(beauty, aov, pd)
    keep, ratio, moved = property_figures(got, plain, beauty, pv.beauty_samples)
    print(f"right half moved {keep:.3e} (variance-guided) vs {moved:.3e} (plain); left-half "
          f"deviation x{ratio:.3f}")
    assert keep <= BOUND
    assert ratio <= 0.5
    assert moved > 100 * BOUND


# ---------------------------------------------------------------- 5. end to end
def test_moments_aov_denoise_on_one_stream(dn):
    spp = 16
    blob, cam = rt.preset_blob("cornell_box", width=64, spp=spp)
    H, W = cam.image_height, cam.image_width
    assert (H, W, cam.samples_per_pixel, cam.sqrt_spp) == (64, 64, spp, 4)
    opts = rt.make_opts(cam, seed=1)
    _, cam_t = rt.preset_blob("cornell_box", width=64, spp=961)
    ds = rt.DeviceScene(blob)
    s = Stream(0)
    b, q, a, o = DevBuf((H, W, 3)), DevBuf((H, W, 3)), DevBuf((H, W, rt.AOV_CHANNELS)), \
        DevBuf((H, W, 3))
    p = params(H, W, 5, n=cam.sqrt_spp, B=spp, A=spp)
    try:
        ds.render_moments_device(cam, opts, b.ptr, q.ptr, stream=s.handle)
        ds.render_aov_device(cam, opts, a.ptr, stream=s.handle)
        dn.denoise_var_device(p, b.ptr, q.ptr, a.ptr, o.ptr, stream=s.handle)
        s.sync()
        got, beauty, m2, aov = o.download(), b.download(), q.download(), a.download()
        host_beauty, _ = ds.render(cam, opts)
        truth, _ = ds.render(cam_t, rt.make_opts(cam_t, seed=7))
    finally:
        s.destroy()
        for d in (b, q, a, o):
            d.free()
        ds.close()
    assert np.array_equal(bits(beauty), bits(host_beauty))
    ref, _, valid = denoise_var_ref(beauty, m2, aov, p)
    m = mean_error(got, ref, p)
    plain = dn.denoise(beauty, aov, rt.denoise_default_params(W, H, spp))
    truth = truth.astype(np.float64) / cam_t.samples_per_pixel
    noisy = clipped_rmse(beauty.astype(np.float64) / spp, truth)
    den = clipped_rmse(got.astype(np.float64) / spp, truth)
    den_plain = clipped_rmse(plain.astype(np.float64) / spp, truth)
    print(f"cornell_box 64x64x{spp}: vs reference {m:.3e}; clipped RMSE noisy {noisy:.4f}, "
          f"variance-guided {den:.4f}, rt_denoise {den_plain:.4f} (5 levels each), "
          f"invalid {int((~valid).sum())}")
    assert m <= BOUND
    assert den < noisy


# ---------------------------------------------------------------- 6. error paths
def test_error_paths_start_no_kernel(dn):
    H, W = 8, 8
    beauty, m2, aov = synth(H, W, seed=51)
    sentinel = np.full((H, W, 3), 7.25, np.float32)
    vs = np.full((H, W), 7.25, np.float32)
    b, q, a, o, v = (DevBuf(x.shape, init=x) for x in (beauty, m2, aov, sentinel, vs))
    try:
        def code(**kw):
            with pytest.raises(rt.RtError) as e:
                dn.denoise_var_device(params(H, W, **kw), b.ptr, q.ptr, a.ptr, o.ptr, v.ptr,
                                      stats=True)
            return e.value.code

        assert code(levels=0) == rt.RT_ERR_INVALID_ARG
        assert code(flags=0x4) == rt.RT_ERR_INVALID_ARG
        assert code(beauty_rows=1) == rt.RT_ERR_INVALID_ARG
        assert code(_pad0=3) == rt.RT_ERR_INVALID_ARG
        with pytest.raises(rt.RtError) as e:
            dn.denoise_var_device(params(H, W), b.ptr, 0, a.ptr, o.ptr, v.ptr)
        assert e.value.code == rt.RT_ERR_INVALID_ARG
        assert np.array_equal(o.download(), sentinel) and np.array_equal(v.download(), vs)
        p0 = params(H, W)
        p0.height = 0
        st = dn.denoise_var_device(p0, b.ptr, q.ptr, a.ptr, o.ptr, v.ptr, stats=True)
        assert st.samples == 0 and st.launches == 0 and st.out_bytes == 0
        assert np.array_equal(o.download(), sentinel)
        p = params(H, W, 2)
        st = dn.denoise_var_device(p, b.ptr, q.ptr, a.ptr, o.ptr, v.ptr, stats=True)
        assert st.launches == 4 and st.samples == H * W and st.ms_kernel > 0.0
        assert st.out_bytes == H * W * 16
        want, wv = dn.denoise_var(beauty, m2, aov, p, var_out=True)
        assert np.array_equal(bits(o.download()), bits(want))
        assert np.array_equal(bits(v.download()), bits(wv))
    finally:
        for d in (b, q, a, o, v):
            d.free()


# ---------------------------------------------------------------- 7. the host program
def test_cli_denoise_var_flag(dn, tmp_path):
    """rt_render_cli --denoise-var [levels] writes the frame this module computes through the
    Python binding."""
    cli = rt.BUILD / "rt_render_cli"
    blob, cam = rt.preset_blob("cornell_box", width=32, spp=4)
    opts = rt.make_opts(cam, seed=1)
    ds = rt.DeviceScene(blob)
    try:
        beauty, m2 = ds.render_moments(cam, opts)
        aov, _ = ds.render_aov(cam, opts)
    finally:
        ds.close()
    files = {}
    for name, levels, extra in (("default", 5, ["--denoise-var"]), ("two", 2, ["--denoise-var", "2"])):
        p = rt.denoise_var_default_params(32, 32, cam.samples_per_pixel, cam.sqrt_spp)
        p.levels = levels
        frame = dn.denoise_var(beauty, m2, aov, p)
        out = tmp_path / f"{name}.ppm"
        r = subprocess.run([str(cli), "--width", "32", "--spp", "4", *extra, "--out", str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        ref = tmp_path / f"{name}_ref.ppm"
        rt.write_ppm(ref, rt.write_color(frame, cam.samples_per_pixel))
        files[name] = out.read_bytes()
        assert files[name] == ref.read_bytes(), name
    assert files["default"] != files["two"]
