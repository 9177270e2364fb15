"""Pixel renders taller than one call's row field (rts::kRowsPerCall = 32760 rows; lane item keys
hold the call's row index in 15 bits): rt_render_device and rt_render_moments_device
(render_device_split, rt_device.hip) and rt_render_aov_device (its own copy of the loop,
rt_aov.hip) render such a row range as consecutive sub-calls into `accum + off` / `m2 + off`,
with `row_begin + k0 * row_step`, and sum the sub-calls' stats. The RNG is keyed by the global
pixel and sample, so the image must not depend on where the split falls.

The frames are strips of the Cornell box 2 pixels or 1 pixel wide with square pixels (aspect
W / H; strip_cases.py), so a 65521-row frame costs 131,042 pixels: a thin column through the
middle of the box (ceiling, light, back wall, floor), no row of it black. Output buffers start
from a sentinel (overwrite) or from random values (accumulate). Heights: 32760 (the last unsplit one), 32761 and 32767 (they pass
check_render_args' 32767-row bound but must still be split), 32768, and 65521 = 2 * 32760 + 1
(three sub-calls, the last of one row).

References, all bit for bit: the same rows rendered by explicit calls of at most 20000 rows each
through row_begin (their boundaries fall elsewhere), and one short call over exactly the rows
that straddle each internal boundary. The 16 rows about the first boundary are also held to the
f64 oracle with the project's 1e-4 bound (test_gpu_parity._check_values).

A strided range: the issue's row_step = 2, n_rows = 32761 fits a 65521-row image only with
row_begin = 0 (rows 0 .. 65520); with row_begin = 1 the last row would be 65521, outside it.
row_begin = 1 is therefore run on a 65523-row image, with the same n_rows and step."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
from strip_cases import cornell_blob, strip_camera

pytestmark = pytest.mark.gpu

SPLIT = 32760  # rts::kRowsPerCall
SHORT = 20000  # rows of an explicit reference call
HEIGHTS = [32760, 32761, 32767, 32768, 65521]
SHAPES = [(2, 1), (1, 2), (2, 2), (1, 1)]  # (W, sqrt_spp)
KINDS = ["beauty", "moments", "aov"]
SEED = 7
TOL = 1e-4
UNWRITTEN = -7.0


@pytest.fixture(scope="module")
def scene(gpu_available):
    blob = cornell_blob()
    ds = rt.DeviceScene(blob)
    yield blob, ds
    ds.close()


def _channels(kind):
    return rt.AOV_CHANNELS if kind == "aov" else 3


class _Frame:
    """The device buffers of one render kind over n_rows rows: accum (and m2 for moments)."""

    def __init__(self, kind, n_rows, W, init=None):
        from hip_buf import DevBuf

        self.kind, self.W, self.ch = kind, W, _channels(kind)
        shape = (n_rows, W, self.ch)
        n = 2 if kind == "moments" else 1
        # without a start value: a sentinel no render writes, so a row left out shows
        self.bufs = [DevBuf(shape, init=np.full(shape, UNWRITTEN, np.float32) if init is None
                            else init[k]) for k in range(n)]

    def call(self, ds, cam, opts, row_off=0, stats=False):
        """One entry-point call whose output starts at row `row_off` of the buffers."""
        off = row_off * self.W * self.ch * 4
        p = [b.ptr + off for b in self.bufs]
        if self.kind == "beauty":
            return ds.render_device(cam, opts, p[0], stats=stats)
        if self.kind == "moments":
            return ds.render_moments_device(cam, opts, p[0], p[1], stats=stats)
        return ds.render_aov_device(cam, opts, p[0], stats=stats)

    def download(self):
        return [b.download() for b in self.bufs]

    def free(self):
        for b in self.bufs:
            b.free()


def _short_calls(fr, ds, cam, n_rows, row_begin=0, row_step=1, flags=rt.RT_FLAG_OVERWRITE):
    """The call's rows by explicit calls of at most SHORT rows each."""
    for k0 in range(0, n_rows, SHORT):
        n = min(SHORT, n_rows - k0)
        fr.call(ds, cam, rt.make_opts(cam, seed=SEED, row_begin=row_begin + k0 * row_step,
                                      row_step=row_step, n_rows=n, flags=flags), row_off=k0)


def _bits_equal(got, want, what):
    for g, w in zip(got, want):
        gu, wu = g.view(np.uint32), w.view(np.uint32)
        if not np.array_equal(gu, wu):
            rows = np.unique(np.argwhere(gu != wu)[:, 0])
            raise AssertionError(f"{what}: {rows.size} rows differ, first {rows[:6].tolist()}")


def _bands(H):
    """Row ranges of up to 24 rows that straddle each internal sub-call boundary of H rows."""
    return [(b - 8, min(b + 16, H)) for b in range(SPLIT, H, SPLIT)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,S", SHAPES)
@pytest.mark.parametrize("H", HEIGHTS)
def test_tall_frame_equals_short_calls(scene, kind, W, S, H):
    """Whole frame against explicit short calls, the straddling bands against one short call
    each, and the summed stats."""
    _, ds = scene
    cam = strip_camera(W, H, S)
    tall_f, ref_f = _Frame(kind, H, W), _Frame(kind, H, W)
    try:
        st = tall_f.call(ds, cam, rt.make_opts(cam, seed=SEED), stats=True)
        tall = tall_f.download()
        _short_calls(ref_f, ds, cam, H)
        _bits_equal(tall, ref_f.download(), f"{kind} {W}x{H} S={S} vs short calls")
        assert all(not (t == UNWRITTEN).any() for t in tall)
        assert tall[0].any()
        # stats: the sub-calls' sums
        assert st.samples == H * W * S * S
        launches = 0
        for k0 in range(0, H, SPLIT):
            n = min(SPLIT, H - k0)
            part = ref_f.call(ds, cam, rt.make_opts(cam, seed=SEED, row_begin=k0, n_rows=n),
                              row_off=k0, stats=True)
            assert part.samples == n * W * S * S
            launches += part.launches
        assert st.launches == launches and launches >= len(range(0, H, SPLIT))
        for lo, hi in _bands(H):
            band_f = _Frame(kind, hi - lo, W)
            try:
                band_f.call(ds, cam, rt.make_opts(cam, seed=SEED, row_begin=lo, n_rows=hi - lo))
                _bits_equal([t[lo:hi] for t in tall], band_f.download(),
                            f"{kind} {W}x{H} S={S} rows [{lo}, {hi})")
            finally:
                band_f.free()
        if H > SPLIT:
            assert _bands(H)[0] == (32752, min(32776, H))
    finally:
        tall_f.free()
        ref_f.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,S", SHAPES[:2])
@pytest.mark.parametrize("H", HEIGHTS)
def test_tall_frame_accumulates_like_short_calls(scene, kind, W, S, H):
    """RT_FLAG_OVERWRITE clear: a tall call into a random non-zero buffer equals the explicit
    short calls into a copy of that buffer."""
    _, ds = scene
    cam = strip_camera(W, H, S)
    rng = np.random.default_rng(H + W)
    n = 2 if kind == "moments" else 1
    base = [rng.random((H, W, _channels(kind)), dtype=np.float32) + 0.5 for _ in range(n)]
    tall_f, ref_f = _Frame(kind, H, W, init=base), _Frame(kind, H, W, init=base)
    try:
        tall_f.call(ds, cam, rt.make_opts(cam, seed=SEED, flags=0))
        _short_calls(ref_f, ds, cam, H, flags=0)
        tall = tall_f.download()
        _bits_equal(tall, ref_f.download(), f"{kind} {W}x{H} S={S} accumulate")
        assert not np.array_equal(tall[0], base[0])
    finally:
        tall_f.free()
        ref_f.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,row_begin", [(65521, 0), (65523, 1)])
def test_tall_strided_range(scene, kind, H, row_begin):
    """row_step = 2, n_rows = 32761 (two sub-calls): the second sub-call starts at
    row_begin + 32760 * 2. Against short strided calls and against the rows of the whole frame."""
    _, ds = scene
    W, S, n_rows = 2, 2, 32761
    cam = strip_camera(W, H, S)
    assert row_begin + (n_rows - 1) * 2 < H
    got_f, ref_f, full_f = _Frame(kind, n_rows, W), _Frame(kind, n_rows, W), _Frame(kind, H, W)
    try:
        st = got_f.call(ds, cam, rt.make_opts(cam, seed=SEED, row_begin=row_begin, row_step=2,
                                              n_rows=n_rows), stats=True)
        assert st.samples == n_rows * W * S * S
        got = got_f.download()
        _short_calls(ref_f, ds, cam, n_rows, row_begin=row_begin, row_step=2)
        _bits_equal(got, ref_f.download(), f"{kind} strided from {row_begin} vs short calls")
        _short_calls(full_f, ds, cam, H)
        _bits_equal(got, [f[row_begin::2][:n_rows] for f in full_f.download()],
                    f"{kind} strided from {row_begin} vs the frame's rows")
    finally:
        for f in (got_f, ref_f, full_f):
            f.free()


@pytest.mark.parametrize("W,S", SHAPES[:2])
def test_rows_about_the_split_against_the_oracle(scene, W, S):
    """The 16 rows [32752, 32768) of the tall GPU frame against the f64 oracle rendering them
    with row_begin = 32752: same NaN / inf masks, per-pixel average within 1e-4."""
    blob, ds = scene
    H, lo, hi = 65521, SPLIT - 8, SPLIT + 8
    cam = strip_camera(W, H, S)
    fr = _Frame("beauty", H, W)
    try:
        fr.call(ds, cam, rt.make_opts(cam, seed=SEED))
        got = fr.download()[0][lo:hi]
    finally:
        fr.free()
    ref, _ = O.render(blob, cam, rt.make_opts(cam, seed=SEED, row_begin=lo, n_rows=hi - lo),
                      precision=64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref))
    assert np.array_equal(np.isneginf(got), np.isneginf(ref))
    fin = np.isfinite(got)
    d = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64)) / (S * S)
    print(f"tall frame vs f64 oracle, {W}x{H} S={S}, rows [{lo}, {hi}): max |d| = {d.max():.3e}")
    assert fin.any() and got[fin].max() > 0.0
    assert d.max() <= TOL


def test_tile_and_adaptive_renders_refuse_tall_ranges(scene):
    """rt_render_tiles_device and rt_render_adaptive_device at 32761 rows: RT_ERR_UNSUPPORTED,
    nothing launched, the output buffers bitwise untouched (and 32760 rows are accepted)."""
    from hip_buf import DevBuf

    _, ds = scene
    lib = rt.device_lib()
    W, S, H = 2, 2, 32761
    cam = strip_camera(W, H, S)
    rng = np.random.default_rng(3)
    base = rng.integers(0, 2**32, (H, W, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    acc, m2 = DevBuf((H, W, 3), init=base), DevBuf((H, W, 3), init=base)  # copied as bytes
    ad = rt.Adaptive()
    try:
        tiles = np.array([0], np.uint32)
        opts = rt.make_opts(cam, seed=SEED, sj_begin=0, sj_count=1)
        st = rt.RtStats()
        rc = lib.rt_render_tiles_device(ds._h, C.byref(cam), C.byref(opts), tiles.ctypes.data, 1,
                                        1, C.c_void_p(acc.ptr), C.c_void_p(m2.ptr), None,
                                        C.byref(st))
        assert rc == rt.RT_ERR_UNSUPPORTED and st.launches == 0 and st.samples == 0
        params = rt.RtAdaptiveParams(passes=1, min_passes=1, threshold=0.0, floor=1e-3)
        tx, ty = rt.tile_grid(W, H)
        rows = np.zeros(tx * ty, np.uint32)
        per = np.zeros(1, np.uint32)
        opts = rt.make_opts(cam, seed=SEED)
        st = rt.RtStats()
        rc = lib.rt_render_adaptive_device(ad._h, ds._h, C.byref(cam), C.byref(opts),
                                           C.byref(params), C.c_void_p(acc.ptr),
                                           C.c_void_p(m2.ptr), None, None, rows.ctypes.data,
                                           per.ctypes.data, None, C.byref(st))
        assert rc == rt.RT_ERR_UNSUPPORTED and st.launches == 0 and st.samples == 0
        assert not rows.any() and not per.any()
        for b in (acc, m2):
            assert np.array_equal(b.download().view(np.uint32), base.view(np.uint32))
        # one row fewer is served by both
        opts = rt.make_opts(cam, seed=SEED, n_rows=H - 1, sj_begin=0, sj_count=1)
        st = ds.render_tiles_device(cam, opts, tiles, 1, acc.ptr, m2.ptr, stats=True)
        assert st.launches >= 1 and st.samples == 8 * W * S
        _, per, st = ad.render_device(ds, cam, rt.make_opts(cam, seed=SEED, n_rows=H - 1), params,
                                      acc.ptr, m2.ptr)
        assert st.launches >= 1 and per[0] == tx * rt.tile_grid(W, H - 1)[1]
    finally:
        ad.close()
        acc.free()
        m2.free()
