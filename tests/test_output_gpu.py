"""The device output stage (rt_output, rt_output_device) against the host stage it restates,
rt.write_color and rt.auto_expose.

The byte rule. The device evaluates the host's f64 expressions in the host's order, so the two can
differ only through pow, whose last bit is not fixed between the two maths libraries. A last-bit
difference of 256 * x changes its integer part only where 256 * x is within rounding of an integer:
a device byte may differ from rt.write_color's only where the host's 256 * x, recomputed here in
f64, lies within 1e-9 of an integer, then by 1, and in at most 2 bytes of a test input. For the
synthetic inputs below no value lies that close (computed in numpy at ev = none, 1.0, 0.37 and
their own auto-exposure: the closest is 1.06e-5 away in the 67x33 frame and 5.9e-7 in the 301x257
one), so the host itself passes with zero differences and any differing byte is a real failure.

The exposure bound. Host and device add the same N non-negative terms (1/N) lum^2 in different
orders; each sum is within about (N + 2) 2^-53 relative of the exact one, the square root halves
the gap and a few roundings remain: 4 N 2^-53 relative."""
import ctypes as C
import functools

import numpy as np
import pytest

import surely_rt as rt
from hip_buf import DevBuf, Stream

pytestmark = pytest.mark.gpu

W, H, SPP = 67, 33, 16
BIG_W, BIG_H = 301, 257  # 77,357 pixels: 38 reduction blocks, then the second stage
E = 2.718281828459045
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def frame(w=W, h=H):
    rng = np.random.default_rng(20241020)
    sums = (np.exp(rng.uniform(np.log(1e-6), np.log(50.0), w * h * 3)) * SPP).astype(np.float32)
    sums = sums.reshape(h, w, 3)
    sums.setflags(write=False)
    return sums


def host_256x(sums, spp, ev):
    """rth_write_color's 256 * x per value, in f64"""
    with np.errstate(all="ignore"):
        x = sums.astype(np.float64).ravel() * (1.0 / spp)
        if ev is not None:
            x = 1.0 - np.power(E, -ev * x)
        x = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
        return 256.0 * np.clip(x, 0.0, 0.999)


def check_bytes(dev, sums, spp, ev, what):
    """the byte rule of the module docstring, over r g b bytes"""
    ref = rt.write_color(sums, spp, ev).ravel()
    dev = np.asarray(dev).ravel()
    assert dev.shape == ref.shape, what
    differ = np.nonzero(dev != ref)[0]
    print(f"{what}: {differ.size} of {ref.size} bytes differ from the host's")
    assert differ.size <= 2, (what, differ[:8])
    y = host_256x(sums, spp, ev)
    for i in differ:
        assert abs(int(dev[i]) - int(ref[i])) == 1, (what, i, dev[i], ref[i])
        assert abs(y[i] - np.round(y[i])) <= 1e-9, (what, i, y[i])


def check_frame(dev, sums, spp, ev, rgba, what):
    if rgba:
        dev = np.asarray(dev).reshape(-1, 4)
        assert (dev[:, 3] == 255).all(), what
        dev = dev[:, :3]
    check_bytes(dev, sums, spp, ev, what)


class Bytes:
    """n output bytes inside a float DevBuf, `shift` bytes past a 4-byte boundary, with 16 or more
    guard bytes on either side; read() checks every guard byte and returns the n bytes."""

    def __init__(self, n, shift=0):
        self.off, self.n = 16 + shift, n
        total = self.off + n + 16
        self.buf = DevBuf((-(-total // 4) + 2,))
        self.buf.upload(np.full(self.buf.nbytes, GUARD, np.uint8).view(np.float32))
        self.ptr = self.buf.ptr + self.off

    def read(self):
        raw = self.buf.download().view(np.uint8)
        assert (raw[:self.off] == GUARD).all(), "bytes written before the output buffer"
        assert (raw[self.off + self.n:] == GUARD).all(), "bytes written after the output buffer"
        return raw[self.off:self.off + self.n].copy()

    def free(self):
        self.buf.free()


def run_device(out, sums, params, in_shift=0, out_shift=0, **kw):
    """rt_output_device over fresh device buffers -> (bytes, what output_device returned); the
    sums start in_shift floats, the bytes out_shift bytes past the allocation's alignment"""
    n_px = params.width * params.height
    src = DevBuf((n_px * 3 + in_shift,),
                 init=np.concatenate([np.zeros(in_shift, np.float32), sums.ravel()]))
    dst = Bytes(n_px * (4 if params.flags & rt.RT_OUTPUT_RGBA else 3), out_shift)
    try:
        res = out.output_device(params, src.ptr + 4 * in_shift, dst.ptr, **kw)
        return dst.read(), res
    finally:
        src.free()
        dst.free()


@pytest.fixture(scope="module")
def out(gpu_available):
    o = rt.Output()
    yield o
    o.close()


# ------------------------------------------------------------------ 1. the synthetic frame
@pytest.mark.parametrize("ev,rgba", [(None, False), (0.37, False), (None, True), (0.37, True)])
def test_synthetic_frame(out, ev, rgba):
    sums = frame()
    p = rt.output_params(W, H, SPP, exposure=ev, rgba=rgba)
    host_bytes, host_ev = out.output(sums, p)
    assert host_bytes.shape == (H, W, 4 if rgba else 3) and host_ev == ev
    check_frame(host_bytes, sums, SPP, ev, rgba, f"rt_output ev={ev} rgba={rgba}")
    dev_bytes, dev_ev = run_device(out, sums, p, want_exposure=True)
    assert dev_ev == ev
    check_frame(dev_bytes, sums, SPP, ev, rgba, f"rt_output_device ev={ev} rgba={rgba}")


# ------------------------------------------------------------------ 2. special values
@pytest.mark.parametrize("ev", [None, 0.37])
def test_special_values_match_the_host_exactly(out, ev):
    knee = np.float32(0.0031308 * SPP)  # linear_to_gamma's branch point, in the sums' scale
    vals = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, knee,
                     np.nextafter(knee, np.float32(0)), np.nextafter(knee, np.float32(1)),
                     1e30, SPP * 0.999], np.float32)
    sums = np.resize(vals, 5 * 3 * 3).reshape(3, 5, 3)  # every value in more than one channel
    p = rt.output_params(5, 3, SPP, exposure=ev)
    ref = rt.write_color(sums, SPP, ev)
    assert ref[0, 0, 0] == 0 and ref[0, 0, 1] == 255 and ref[0, 0, 2] == 0  # NaN, +inf, -inf
    host_bytes, _ = out.output(sums, p)
    assert np.array_equal(host_bytes, ref)
    dev_bytes, _ = run_device(out, sums, p)
    assert np.array_equal(dev_bytes.reshape(ref.shape), ref)


# ------------------------------------------------------------------ 3. auto-exposure
def auto(out, sums, w, h):
    """both entry points with RT_OUTPUT_AUTO_EXPOSE -> (bytes, ev), asserted bit-equal"""
    p = rt.output_params(w, h, SPP, auto=True)
    host_bytes, host_ev = out.output(sums, p)
    dev_bytes, dev_ev = run_device(out, sums, p, want_exposure=True)
    assert host_ev == dev_ev and np.array_equal(host_bytes.ravel(), dev_bytes)
    return dev_bytes, dev_ev


@pytest.mark.parametrize("w,h", [(W, H), (BIG_W, BIG_H)])
def test_auto_exposure_against_the_host(out, w, h):
    sums = frame(w, h)
    dev_bytes, ev = auto(out, sums, w, h)
    ref_ev = rt.auto_expose(sums, SPP)
    rel = abs(ev - ref_ev) / ref_ev
    print(f"{w}x{h}: device ev {ev!r}, host ev {ref_ev!r}, relative difference {rel:.3e}, "
          f"bound {4 * w * h * 2.0 ** -53:.3e}")
    if (w, h) == (W, H):
        assert abs(ref_ev - 0.0730626) < 1e-6
    assert rel <= 4 * w * h * 2.0 ** -53
    check_bytes(dev_bytes, sums, SPP, ev, f"auto-exposure {w}x{h}")
    # the same input again: the same bits
    again_bytes, again_ev = auto(out, sums, w, h)
    assert again_ev == ev and np.array_equal(again_bytes, dev_bytes)


def test_auto_exposure_special_cases(out):
    dim = (frame() * np.float32(1e-3)).astype(np.float32)  # m < 0.001
    dev_bytes, ev = auto(out, dim, W, H)
    assert ev == 1.0 and rt.auto_expose(dim, SPP) == 1.0
    check_bytes(dev_bytes, dim, SPP, 1.0, "auto-exposure of a dim frame")
    bad = frame().copy()
    bad[H // 2, W // 3] = np.nan  # one NaN pixel: m is NaN
    dev_bytes, ev = auto(out, bad, W, H)
    assert ev == 1.0 and rt.auto_expose(bad, SPP) == 1.0
    assert (dev_bytes.reshape(H, W, 3)[H // 2, W // 3] == 0).all()
    check_bytes(dev_bytes, bad, SPP, 1.0, "auto-exposure with a NaN pixel")


# ------------------------------------------------------------------ 4. footprint and alignment
@pytest.mark.parametrize("rgba", [False, True])
def test_footprint_and_alignment(out, rgba):
    sums = frame()
    p = rt.output_params(W, H, SPP, exposure=0.37, rgba=rgba)
    aligned, _ = run_device(out, sums, p)  # Bytes.read checks the guard bytes on both sides
    check_frame(aligned, sums, SPP, 0.37, rgba, f"aligned rgba={rgba}")
    shifted, _ = run_device(out, sums, p, in_shift=1, out_shift=1)
    assert np.array_equal(shifted, aligned)
    # auto-exposure reads the shifted input too
    pa = rt.output_params(W, H, SPP, auto=True, rgba=rgba)
    a0, ev0 = run_device(out, sums, pa, want_exposure=True)
    a1, ev1 = run_device(out, sums, pa, in_shift=1, out_shift=3, want_exposure=True)
    assert ev0 == ev1 and np.array_equal(a0, a1)


def test_empty_frame_touches_nothing(out):
    p = rt.output_params(W, 0, SPP, auto=True)
    dst = Bytes(W * H * 3)
    src = DevBuf((W * H * 3,), init=frame().ravel())
    try:
        st = out.output_device(p, src.ptr, dst.ptr, stats=True)
        assert st.samples == 0 and st.out_bytes == 0 and st.launches == 0
        assert (dst.read() == GUARD).all()
    finally:
        src.free()
        dst.free()
    empty, _ = out.output(np.zeros((0, W, 3), np.float32), p)
    assert empty.shape == (0, W, 3)


# ------------------------------------------------------------------ 5. stream order, handle reuse
def test_output_follows_a_render_on_its_stream(out):
    blob, cam = rt.preset_blob("cornell_box", width=64, spp=16)
    n_px = cam.image_width * cam.image_height
    ds = rt.DeviceScene(blob, device=0)
    stream = Stream()
    acc = DevBuf((n_px * 3,))
    dst = Bytes(n_px * 3)
    p = rt.output_params(cam.image_width, cam.image_height, cam.samples_per_pixel, auto=True)
    try:
        ds.render_device(cam, rt.make_opts(cam, seed=1, flags=rt.RT_FLAG_OVERWRITE), acc.ptr,
                         stream=stream.handle)
        out.output_device(p, acc.ptr, dst.ptr, stream=stream.handle)  # no synchronisation between
        stream.sync()
        dev_bytes = dst.read()
        sums = acc.download().reshape(cam.image_height, cam.image_width, 3)
        assert np.isfinite(sums).all() and sums.max() > 0
        # the exposure that call applied: the same input gives the same bits
        ev = out.output_device(p, acc.ptr, dst.ptr, stream=stream.handle, want_exposure=True)
        assert np.array_equal(dst.read(), dev_bytes)
        ref_ev = rt.auto_expose(sums, cam.samples_per_pixel)
        assert abs(ev - ref_ev) / ref_ev <= 4 * n_px * 2.0 ** -53
        check_bytes(dev_bytes, sums, cam.samples_per_pixel, ev, "cornell_box 64x64x16 on a stream")
    finally:
        stream.destroy()
        acc.free()
        dst.free()
        ds.close()


def test_one_handle_grows_its_workspace_and_fills_the_stats(gpu_available):
    o = rt.Output()
    try:
        for (w, h), rgba in (((W, H), False), ((BIG_W, BIG_H), True), ((W, H), True)):
            sums = frame(w, h)
            p = rt.output_params(w, h, SPP, auto=True, rgba=rgba)
            dev_bytes, (ev, st) = run_device(o, sums, p, want_exposure=True, stats=True)
            assert abs(ev - rt.auto_expose(sums, SPP)) / ev <= 4 * w * h * 2.0 ** -53
            check_frame(dev_bytes, sums, SPP, ev, rgba, f"one handle, {w}x{h}")
            assert st.samples == w * h and st.out_bytes == w * h * (4 if rgba else 3)
            assert st.launches >= 1 and not any(st.ops) and st.ms_kernel > 0
            host_bytes, host_ev, hst = o.output(sums, p, stats=True)
            assert host_ev == ev and np.array_equal(host_bytes.ravel(), dev_bytes)
            assert hst.samples == w * h and hst.out_bytes == st.out_bytes and not any(hst.ops)
        # without auto-exposure: one launch
        _, st = run_device(o, frame(), rt.output_params(W, H, SPP), stats=True)
        assert st.launches == 1 and st.out_bytes == W * H * 3
    finally:
        o.close()
