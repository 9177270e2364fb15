"""Re-entrancy of one device scene ("re-entrant per distinct output buffer"; the
reference's render_par_lights takes &HittableList and may run concurrently, render.rs:144-150).

Renders of ONE rt_scene issued on two HIP streams at once, and from two host threads at once,
each into its own buffer, must give their serial images bit for bit (include/rt_mi355x.h: every
render call takes its own slot of pool-queue word, counters and workspace)."""
import threading

import numpy as np
import pytest

import surely_rt as rt

pytestmark = pytest.mark.gpu

CASES = [("cornell_box", dict(width=400, spp=256)),
         ("final_scene", dict(width=200, spp=64, depth=12))]


@pytest.mark.parametrize("name,kw", CASES)
def test_two_streams_render_one_scene_concurrently(gpu_available, name, kw):
    from hip_buf import DevBuf, Stream

    blob, cam = rt.preset_blob(name, **kw)
    ds = rt.DeviceScene(blob)
    seeds = (11, 12)
    serial = [ds.render(cam, rt.make_opts(cam, seed=s))[0] for s in seeds]
    assert not np.array_equal(serial[0], serial[1])
    ones = np.ones(serial[0].shape, np.float32)
    # accumulate mode, serially: ones + the render's sums (rounded once, from f64)
    serial_acc = [ds.render(cam, rt.make_opts(cam, seed=s, flags=0), accum=ones.copy())[0]
                  for s in seeds]
    streams = [Stream(), Stream()]
    bufs = [DevBuf(serial[0].shape), DevBuf(serial[0].shape)]
    try:
        # three rounds back to back, nothing synchronised in between: both streams' renders are
        # in flight together, and each stream reuses its own slot in stream order
        for _ in range(3):
            for s, st, b in zip(seeds, streams, bufs):
                ds.render_device(cam, rt.make_opts(cam, seed=s), b.ptr, st.handle)
        for st in streams:
            st.sync()
        for b, ref in zip(bufs, serial):
            assert np.array_equal(b.download(), ref)
        # accumulate mode on both streams at once: each buffer gets its own render added
        for b in bufs:
            b.upload(ones)
        for s, st, b in zip(seeds, streams, bufs):
            ds.render_device(cam, rt.make_opts(cam, seed=s, flags=0), b.ptr, st.handle)
        # a synchronous render with stats meanwhile (its own slot, third stream = NULL)
        again, stt = ds.render(cam, rt.make_opts(cam, seed=seeds[0]))
        assert np.array_equal(again, serial[0]) and stt.samples == cam.image_width * cam.image_height * cam.samples_per_pixel
        for st in streams:
            st.sync()
        for b, ref in zip(bufs, serial_acc):
            assert np.array_equal(b.download(), ref)
    finally:
        for b in bufs:
            b.free()
        for st in streams:
            st.destroy()
        ds.close()


@pytest.mark.parametrize("name,kw", CASES[:1])
def test_two_host_threads_render_one_scene(gpu_available, name, kw):
    blob, cam = rt.preset_blob(name, **kw)
    ds = rt.DeviceScene(blob)
    seeds = (21, 22)
    serial = {s: ds.render(cam, rt.make_opts(cam, seed=s))[0] for s in seeds}
    got: dict[int, list] = {s: [] for s in seeds}
    errors: list[BaseException] = []

    def work(s):
        try:
            for _ in range(4):
                acc, st = ds.render(cam, rt.make_opts(cam, seed=s))
                got[s].append((acc, st.samples))
        except BaseException as e:  # surfaced in the main thread
            errors.append(e)

    th = [threading.Thread(target=work, args=(s,)) for s in seeds]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    ds.close()
    assert not errors, errors
    for s in seeds:
        assert len(got[s]) == 4
        for acc, n in got[s]:
            assert np.array_equal(acc, serial[s])
            assert n == cam.image_width * cam.image_height * cam.samples_per_pixel


def test_per_thread_default_stream_from_two_threads(gpu_available):
    """hipStreamPerThread has one handle value but is a different stream in each host thread
    (ADVICE r4): a render must not take a slot whose previous render, issued by another thread
    on "the same" handle, may still be running. Each thread issues four renders back to back on
    hipStreamPerThread without synchronising, then checks its buffer."""
    from hip_buf import DevBuf, hip

    blob, cam = rt.preset_blob("cornell_box", width=400, spp=256)
    ds = rt.DeviceScene(blob)
    seeds = (31, 32)
    serial = {s: ds.render(cam, rt.make_opts(cam, seed=s))[0] for s in seeds}
    per_thread = 2  # hipStreamPerThread (hip_runtime_api.h)
    bufs = {s: DevBuf(serial[s].shape) for s in seeds}
    errors: list[BaseException] = []
    got: dict[int, np.ndarray] = {}

    def work(s):
        try:
            for _ in range(4):
                ds.render_device(cam, rt.make_opts(cam, seed=s), bufs[s].ptr, per_thread)
            assert hip().hipStreamSynchronize(per_thread) == 0
            got[s] = bufs[s].download()
        except BaseException as e:  # surfaced in the main thread
            errors.append(e)

    th = [threading.Thread(target=work, args=(s,)) for s in seeds]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    for b in bufs.values():
        b.free()
    ds.close()
    assert not errors, errors
    for s in seeds:
        assert np.array_equal(got[s], serial[s])


# ------------------------------------------------------------------ more streams than slots
# A scene keeps at most rt_scene::kMaxSlots = 8 render slots (acquire_slot, rt_device.hip). Twelve
# renders of one scene on twelve streams, issued back to back from one thread without stats or
# synchronisation: from the ninth on, a call finds no new slot to make and takes a slot an earlier
# render used (after that render's event, which its stream also waits for), with that slot's
# pool-queue word, counters and workspace. Every buffer must still hold its serial image.
N_STREAMS = 12


def _issue_all(jobs, streams):
    """Every job's call once, back to back, then all streams synchronised."""
    for job, st in zip(jobs, streams):
        job(st.handle)
    for st in streams:
        st.sync()


def test_twelve_streams_share_eight_slots(gpu_available):
    from hip_buf import DevBuf, Stream

    blob, cam = rt.preset_blob("cornell_box", width=40, spp=16, aspect=40.0 / 24.0)
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (40, 24, 16)
    ds = rt.DeviceScene(blob)
    seeds = list(range(41, 41 + N_STREAMS))
    serial = [ds.render(cam, rt.make_opts(cam, seed=s))[0] for s in seeds]
    assert len({a.tobytes() for a in serial}) == N_STREAMS
    streams = [Stream() for _ in range(N_STREAMS)]
    bufs = [DevBuf(serial[0].shape) for _ in range(N_STREAMS)]
    jobs = [lambda h, s=s, b=b: ds.render_device(cam, rt.make_opts(cam, seed=s), b.ptr, h)
            for s, b in zip(seeds, bufs)]
    try:
        for rnd in range(2):  # the second round meets slots with a recorded event
            for b in bufs:
                b.upload(np.full(b.shape, -7.0, np.float32))
            _issue_all(jobs, streams)
            for k, (b, ref) in enumerate(zip(bufs, serial)):
                assert np.array_equal(b.download(), ref), f"round {rnd}, stream {k}"
    finally:
        for b in bufs:
            b.free()
        for st in streams:
            st.destroy()
        ds.close()


def test_mixed_shapes_pass_through_shared_slots(gpu_available):
    """64x64 and 8x8 frames alternate over the twelve streams, so a reused slot's workspace is
    in turn larger and smaller than the render needs; one of the renders is a moments render
    (the slot's second workspace) and one a tile-list render (the slot's tile list)."""
    from hip_buf import DevBuf, Stream

    blob, big = rt.preset_blob("cornell_box", width=64, spp=16)
    _, small = rt.preset_blob("cornell_box", width=8, spp=16)
    assert (big.image_height, small.image_height) == (64, 8)
    ds = rt.DeviceScene(blob)
    tiles = np.array([0, 3, 9, 36, 63], np.uint32)  # of the 8 x 8 tile grid of the 64x64 frame
    S = big.sqrt_spp
    MOMENTS, TILES = 4, 6  # two of the 64x64 jobs
    fill = np.float32(0.5)

    def make(k, bufs):
        cam = big if k % 2 == 0 else small
        if k == MOMENTS:
            return lambda h: ds.render_moments_device(cam, rt.make_opts(cam, seed=60 + k),
                                                      bufs[0].ptr, bufs[1].ptr, h)
        if k == TILES:
            opts = rt.make_opts(cam, seed=60 + k, sj_begin=0, sj_count=S)
            return lambda h: ds.render_tiles_device(cam, opts, tiles, 1, bufs[0].ptr,
                                                    bufs[1].ptr, h)
        return lambda h: ds.render_device(cam, rt.make_opts(cam, seed=60 + k), bufs[0].ptr, h)

    def buffers(k):
        cam = big if k % 2 == 0 else small
        shape = (cam.image_height, cam.image_width, 3)
        n = 2 if k in (MOMENTS, TILES) else 1
        return [DevBuf(shape, init=np.full(shape, fill, np.float32)) for _ in range(n)]

    streams = [Stream() for _ in range(N_STREAMS)]
    bufs = [buffers(k) for k in range(N_STREAMS)]
    ref_bufs = [buffers(k) for k in range(N_STREAMS)]
    try:
        serial = []
        for k in range(N_STREAMS):  # one at a time, each synchronised before the next
            make(k, ref_bufs[k])(0)
            serial.append([b.download() for b in ref_bufs[k]])
        # tile row 2 (rows 16-23) holds no listed tile; tile 0 is rows and columns 0-7
        assert (serial[TILES][0][16:24] == fill).all()
        assert not (serial[TILES][0][:8, :8] == fill).any()
        assert serial[MOMENTS][1].any() and not np.array_equal(serial[0][0], serial[2][0])
        jobs = [make(k, bufs[k]) for k in range(N_STREAMS)]
        for rnd in range(2):
            for bb in bufs:
                for b in bb:
                    b.upload(np.full(b.shape, fill, np.float32))
            _issue_all(jobs, streams)
            for k in range(N_STREAMS):
                for b, ref in zip(bufs[k], serial[k]):
                    assert np.array_equal(b.download(), ref), f"round {rnd}, stream {k}"
    finally:
        for bb in bufs + ref_bufs:
            for b in bb:
                b.free()
        for st in streams:
            st.destroy()
        ds.close()
