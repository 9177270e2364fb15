"""How a frame is put together from several devices' cyclic row shares: rt_multi_* (rt.MultiScene:
device scatter / gather through rt_deinterleave, rt_device.hip) and rt_render_multi
(rt.render_multi: the host de-interleave), at the shapes where that code can go wrong and the
72-row frames of test_gpu_parity cannot show it: shares of unequal size (the arithmetic exists
on the host as (n_rows - k + G - 1) / G and again in the kernel's row0 loop), more devices than
rows, strided row ranges and stratum subsets, the accumulate scatter on ragged shares, rows wide
enough for a second pass of the kernel's x stride loop (3 W > 64 * 256), frames taller than a
grid's 65535 blocks in y (rt_deinterleave loops over rows; each device's share of 35001 rows is
also split into sub-calls of 32760), staging-buffer reuse, two frames on two caller streams, and
a frame followed by the output stage on one stream.

The box's one GPU listed several times gives every listing its own rt_scene, stream and row
buffer, so the shares really run concurrently. The reference in every case is one rt_render of
the same camera and options on a single DeviceScene, compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import surely_rt as rt
from strip_cases import cornell_blob, strip_camera

pytestmark = pytest.mark.gpu

LISTS = [[0], [0, 0], [0, 0, 0], [0] * 5]
RAGGED_H = [1, 2, 3, 4, 7, 61]
OVERWRITE = rt.RT_FLAG_OVERWRITE


@pytest.fixture(scope="module")
def one(gpu_available):
    """The blob and the single-device scene every reference frame comes from."""
    blob = cornell_blob()
    ds = rt.DeviceScene(blob)
    yield blob, ds
    ds.close()


def _base(shape, seed=1):
    return np.random.default_rng(seed).random(shape, dtype=np.float32) + 0.25


def _single(ds, cam, opts):
    """(overwritten frame, frame accumulated into _base) of one device, and the base."""
    shape = (opts.n_rows, cam.image_width, 3)
    full, _ = ds.render(cam, opts)
    acc_opts = rt.RtRenderOpts.from_buffer_copy(opts)
    acc_opts.flags = opts.flags & ~OVERWRITE
    base = _base(shape)
    acc, _ = ds.render(cam, acc_opts, accum=base.copy())
    assert full.any() and not np.array_equal(acc, base)
    return full, acc, base, acc_opts


def _same(got, want, what):
    gu, wu = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(gu, wu):
        rows = np.unique(np.argwhere(gu != wu)[:, 0])
        raise AssertionError(f"{what}: {rows.size} of {got.shape[0]} rows differ, "
                             f"first {rows[:8].tolist()}")


def _n_samples(cam, opts):
    return opts.n_rows * cam.image_width * (opts.sj_count or cam.sqrt_spp) * cam.sqrt_spp


def _check_handle(m, ds, cam, opts, what):
    """One overwritten and one accumulated frame of `m` against the single device; 2 frames."""
    from hip_buf import DevBuf

    full, acc, base, acc_opts = _single(ds, cam, opts)
    out = DevBuf(full.shape, init=np.full(full.shape, -7.0, np.float32))
    try:
        st = m.render_device(cam, opts, out.ptr, stats=True)
        _same(out.download(), full, f"rt_multi {what}")
        assert st.samples == _n_samples(cam, opts) and st.launches == len(m.devices)
        out.upload(base)
        m.render_device(cam, acc_opts, out.ptr)
        _same(out.download(), acc, f"rt_multi accumulate {what}")
    finally:
        out.free()


def _check_host(blob, devs, ds, cam, opts, what):
    full, acc, base, acc_opts = _single(ds, cam, opts)
    got, st = rt.render_multi(blob, cam, opts, devs,
                              accum=np.full(full.shape, -7.0, np.float32))
    _same(got, full, f"rt_render_multi {what}")
    assert st.samples == _n_samples(cam, opts) and st.launches == len(devs)
    got, _ = rt.render_multi(blob, cam, acc_opts, devs, accum=base.copy())
    _same(got, acc, f"rt_render_multi accumulate {what}")


def _sub_ranges(cam):
    """(name, opts) on a 61-row image at sqrt_spp = 2: strided rows, one stratum row, both."""
    return [("rows 5 + 3k", rt.make_opts(cam, seed=4, row_begin=5, row_step=3, n_rows=11)),
            ("stratum row 1", rt.make_opts(cam, seed=4, sj_begin=1, sj_count=1)),
            ("rows 5 + 3k, stratum row 1",
             rt.make_opts(cam, seed=4, row_begin=5, row_step=3, n_rows=11, sj_begin=1, sj_count=1))]


# ---------------------------------------------------------------- rt_multi_*
@pytest.mark.parametrize("devs", LISTS, ids=lambda d: f"G{len(d)}")
def test_multi_ragged_and_tiny_shares(one, devs):
    """W = 9, 4 spp, H in {1, 2, 3, 4, 7, 61}: shares of unequal size and, with 5 listings,
    devices without a row. stats.samples is exact and every call counts as a frame."""
    blob, ds = one
    m = rt.MultiScene(blob, devs)
    try:
        for n, H in enumerate(RAGGED_H):
            cam = strip_camera(9, H, 2)
            _check_handle(m, ds, cam, rt.make_opts(cam, seed=4), f"{devs} H={H}")
            assert m.info()["frames"] == 2 * (n + 1)
        info = m.info()
        assert info["uploads"] == info["devices"] == len(devs)
    finally:
        m.close()


@pytest.mark.parametrize("devs", LISTS, ids=lambda d: f"G{len(d)}")
def test_multi_row_and_stratum_sub_ranges(one, devs):
    """row_begin = 5, row_step = 3, n_rows = 11 of 61 rows; sj_begin = 1, sj_count = 1 of
    sqrt_spp = 2 (stats.samples follows sj_count); and both at once."""
    blob, ds = one
    cam = strip_camera(9, 61, 2)
    m = rt.MultiScene(blob, devs)
    try:
        for name, opts in _sub_ranges(cam):
            _check_handle(m, ds, cam, opts, f"{devs} {name}")
        assert _n_samples(cam, _sub_ranges(cam)[2][1]) == 11 * 9 * 1 * 2
    finally:
        m.close()


def test_multi_wide_rows(one):
    """W = 5500 (16500 floats a row > 64 blocks * 256 threads): the second pass of the kernel's
    x stride loop, gather and scatter, on three ragged shares of 7 rows."""
    blob, ds = one
    cam = strip_camera(5500, 7, 1)
    assert cam.image_width * 3 > 64 * 256
    m = rt.MultiScene(blob, [0, 0, 0])
    try:
        _check_handle(m, ds, cam, rt.make_opts(cam, seed=4), "W=5500 H=7")
    finally:
        m.close()


@pytest.mark.parametrize("devs", LISTS[1:3], ids=lambda d: f"G{len(d)}")
def test_multi_tall_frame(one, devs):
    """W = 1, H = 70001 > 65535: rt_deinterleave's row loop and the capped grid.y, overwrite
    and accumulate; with two listings each share (35001, 35000 rows) is also split into
    sub-calls inside rt_render_device, at a row stride of 2."""
    from hip_buf import hip

    blob, ds = one
    cam = strip_camera(1, 70001, 1)
    limit = C.c_int(0)  # 30: hipDeviceAttributeMaxGridDimY (hip_runtime_api.h, ROCm 7)
    assert hip().hipDeviceGetAttribute(C.byref(limit), 30, 0) == 0
    print(f"hipDeviceAttributeMaxGridDimY = {limit.value}; the frame has {cam.image_height} rows")
    m = rt.MultiScene(blob, devs)
    try:
        _check_handle(m, ds, cam, rt.make_opts(cam, seed=4), f"{devs} H=70001")
    finally:
        m.close()


def test_multi_staging_reuse_on_one_handle(one):
    """61 rows, then 7, then 61 again, then 128: the staging buffer is reallocated only when a
    frame outgrows it (stage_allocs 1, 1, 1, 2) and every frame is right."""
    from hip_buf import DevBuf

    blob, ds = one
    m = rt.MultiScene(blob, [0, 0])
    try:
        for H, allocs in ((61, 1), (7, 1), (61, 1), (128, 2)):
            cam = strip_camera(9, H, 2)
            opts = rt.make_opts(cam, seed=6)
            full, _ = ds.render(cam, opts)
            out = DevBuf(full.shape, init=np.full(full.shape, -7.0, np.float32))
            try:
                m.render_device(cam, opts, out.ptr)
                _same(out.download(), full, f"staging reuse H={H}")
            finally:
                out.free()
            assert m.info()["stage_allocs"] == allocs, H
    finally:
        m.close()


@pytest.mark.parametrize("swapped", [False, True], ids=["a_then_b", "b_then_a"])
def test_multi_two_caller_streams(one, swapped):
    """Frame A (seed 4) on stream s1 into a, frame B (seed 5) on stream s2 into b, no host
    synchronisation between the calls and no stats: the second frame reuses the staging area
    and the devices' row buffers, so it must wait for the first frame's gather (frame_done)."""
    from hip_buf import DevBuf, Stream

    blob, ds = one
    cam = strip_camera(40, 61, 4)
    want = {s: ds.render(cam, rt.make_opts(cam, seed=s))[0] for s in (4, 5)}
    assert not np.array_equal(want[4], want[5])
    m = rt.MultiScene(blob, [0, 0, 0])
    streams = {4: Stream(), 5: Stream()}
    bufs = {s: DevBuf(want[s].shape, init=np.full(want[s].shape, -7.0, np.float32))
            for s in (4, 5)}
    try:
        for s in ((5, 4) if swapped else (4, 5)):
            m.render_device(cam, rt.make_opts(cam, seed=s), bufs[s].ptr, streams[s].handle)
        for st in streams.values():
            st.sync()
        for s in (4, 5):
            _same(bufs[s].download(), want[s], f"two streams, seed {s}")
        assert m.info()["frames"] == 2
    finally:
        for b in bufs.values():
            b.free()
        m.close()
        for st in streams.values():
            st.destroy()


def test_multi_frame_then_output_stage_on_one_stream(one):
    """rt_multi_render followed by rt_output_device on the same stream with no synchronisation
    in between: the bytes are those of the single-device frame."""
    from hip_buf import DevBuf, Stream

    blob, ds = one
    cam = strip_camera(40, 61, 2)
    opts = rt.make_opts(cam, seed=8)
    full, _ = ds.render(cam, opts)
    n_px = cam.image_width * cam.image_height
    p = rt.output_params(cam.image_width, cam.image_height, cam.samples_per_pixel, auto=True)
    out = rt.Output()
    want, _ = out.output(full, p)
    m = rt.MultiScene(blob, [0, 0, 0])
    stream = Stream()
    acc = DevBuf(full.shape, init=np.full(full.shape, -7.0, np.float32))
    dst = DevBuf((-(-n_px * 3 // 4),))
    try:
        m.render_device(cam, opts, acc.ptr, stream.handle)
        out.output_device(p, acc.ptr, dst.ptr, stream=stream.handle)
        stream.sync()
        got = dst.download().view(np.uint8)[:n_px * 3].reshape(want.shape)
        assert np.array_equal(got, want)
        assert len(np.unique(want)) > 8
    finally:
        acc.free()
        dst.free()
        stream.destroy()
        m.close()
        out.close()


def test_multi_argument_checks(one):
    """A row range outside the image, row_step = 0, a null output and no devices are
    RT_ERR_INVALID_ARG and count no frame; n_rows = 0 is RT_OK and touches nothing."""
    from hip_buf import DevBuf

    blob, ds = one
    lib = rt.device_lib()
    cam = strip_camera(9, 61, 2)
    guard = _base((61, 9, 3), seed=9)
    out = DevBuf(guard.shape, init=guard)
    m = rt.MultiScene(blob, [0, 0, 0])
    try:
        def code(opts, ptr):
            with pytest.raises(rt.RtError) as e:
                m.render_device(cam, opts, ptr)
            return e.value.code

        # rows 59, 62: the second lies outside the 61-row image
        assert code(rt.make_opts(cam, row_begin=59, row_step=3, n_rows=2), out.ptr) == \
            rt.RT_ERR_INVALID_ARG
        bad_step = rt.make_opts(cam, n_rows=1)
        bad_step.row_step = 0
        assert code(bad_step, out.ptr) == rt.RT_ERR_INVALID_ARG
        assert code(rt.make_opts(cam), 0) == rt.RT_ERR_INVALID_ARG
        h = C.c_void_p()
        devs = (C.c_int * 1)(0)
        assert lib.rt_multi_create(blob.ref(), devs, 0, C.byref(h)) == rt.RT_ERR_INVALID_ARG
        assert not h.value
        assert m.info()["frames"] == 0
        m.render_device(cam, rt.make_opts(cam, n_rows=0), out.ptr)  # RT_OK
        assert m.info()["frames"] == 0
        assert np.array_equal(out.download(), guard)
        # the refused calls left the handle usable
        full, _ = ds.render(cam, rt.make_opts(cam, seed=4))
        m.render_device(cam, rt.make_opts(cam, seed=4), out.ptr)
        _same(out.download(), full, "after refused calls")
        assert m.info()["frames"] == 1
    finally:
        out.free()
        m.close()


# ---------------------------------------------------------------- rt_render_multi (host path)
@pytest.mark.parametrize("devs", LISTS, ids=lambda d: f"G{len(d)}")
def test_render_multi_ragged_and_sub_ranges(one, devs):
    """The host path over the same ragged heights and sub-ranges, overwrite and accumulate."""
    blob, ds = one
    for H in RAGGED_H:
        cam = strip_camera(9, H, 2)
        _check_host(blob, devs, ds, cam, rt.make_opts(cam, seed=4), f"{devs} H={H}")
    cam = strip_camera(9, 61, 2)
    for name, opts in _sub_ranges(cam):
        _check_host(blob, devs, ds, cam, opts, f"{devs} {name}")


@pytest.mark.parametrize("devs", LISTS[1:3], ids=lambda d: f"G{len(d)}")
def test_render_multi_tall_frame(one, devs):
    """W = 1, H = 70001 through the host de-interleave; shares of 35001 rows are split."""
    blob, ds = one
    cam = strip_camera(1, 70001, 1)
    _check_host(blob, devs, ds, cam, rt.make_opts(cam, seed=4), f"{devs} H=70001")


def test_render_multi_argument_checks(one):
    """The same refusals through rt_render_multi; n_rows = 0 is RT_OK and touches nothing."""
    blob, _ = one
    lib = rt.device_lib()
    cam = strip_camera(9, 61, 2)
    guard = _base((61, 9, 3), seed=9)
    acc = guard.copy()

    def code(opts, devs, accum=acc):
        with pytest.raises(rt.RtError) as e:
            rt.render_multi(blob, cam, opts, devs, accum=accum)
        return e.value.code

    assert code(rt.make_opts(cam, row_begin=59, row_step=3, n_rows=2), [0, 0, 0]) == \
        rt.RT_ERR_INVALID_ARG
    bad_step = rt.make_opts(cam, n_rows=1)
    bad_step.row_step = 0
    assert code(bad_step, [0, 0]) == rt.RT_ERR_INVALID_ARG
    assert code(rt.make_opts(cam), []) == rt.RT_ERR_INVALID_ARG
    opts, devs = rt.make_opts(cam), (C.c_int * 2)(0, 0)
    assert lib.rt_render_multi(blob.ref(), C.byref(cam), C.byref(opts), devs, 2, None,
                               None) == rt.RT_ERR_INVALID_ARG
    none = rt.make_opts(cam, n_rows=0)
    assert lib.rt_render_multi(blob.ref(), C.byref(cam), C.byref(none), devs, 2, acc.ctypes.data,
                               None) == rt.RT_OK
    assert np.array_equal(acc, guard)
