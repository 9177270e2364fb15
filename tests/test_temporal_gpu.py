"""rt_temporal_* on the GPU against tests/temporal_ref.py (the definition of include/rt_mi355x.h in
f64 numpy) over the synthetic sequences of tests/temporal_cases.py, against closed forms that do
not go through the reference, and end to end on cornell_box.

Error measure: the project's, max |got - ref| / max(1, |ref|) on the mean radiance (sums / B,
denoise_ref.mean_error); for the moments the same on Q * n / B^2 (the mean of the squared row
means: the scale in which the estimator reads them); for hist_len the same with max(1, L).
Fragile pixels (temporal_ref.py) are left out, and their share is bounded by 1 %.

Bound: the ceiling is the project's per-pixel parity bound, 1e-4; the asserted BOUND is 8 x the
largest value measured on an MI355X, rounded up to one significant digit (the rule of
test_denoise_gpu.py). Measured maxima (every test prints its own):
  synthetic cases, 4 variants x 6 sizes   colour 1.27e-07  m2 2.03e-07  hist_len 0
  static camera / saturation              1.69e-07
  half-pixel ramp shift (closed form)     0
  cornell_box orbit against the reference colour 1.97e-07  m2 2.45e-07  hist_len 1.19e-07
  cornell_box, camera still, four renders 2.63e-07
The largest is 2.63e-07; 8 x 2.63e-07 = 2.1e-06, rounded up to one digit: BOUND = 3e-6."""
import ctypes as C
import threading

import numpy as np
import pytest

import surely_rt as rt
import temporal_cases as TC
import temporal_ref as TR
from hip_buf import DevBuf, Stream

pytestmark = pytest.mark.gpu

CEILING = 1e-4
BOUND = 3e-6  # 8 x the measured maximum, one significant digit; see the docstring
assert BOUND <= CEILING
M2_SCALE = TC.SPP * TC.SPP / TC.ROWS


@pytest.fixture(scope="module")
def seqs():
    return TC.sequences()


def run_gpu(s, p, m2, frames=None, t=None):
    """the sequence through one handle (host buffers): a list of (beauty, m2 or None, hist_len)"""
    own = t is None
    t = t or rt.Temporal()
    out = []
    try:
        for k in range(len(s.cams) if frames is None else frames):
            r = t.accumulate(s.cams[k], s.beauty[k], s.aov[k], p, m2=s.m2[k] if m2 else None,
                             hist_len=True)
            out.append((r[0], r[1] if m2 else None, r[-1]))
    finally:
        if own:
            t.close()
    return out


def compare(tag, got, r, b_in, q_in, scale=TC.SPP, m2_scale=M2_SCALE):
    """one frame against the reference's dict r; returns the three error figures"""
    b, q, ln = got
    keep = ~r["fragile"]
    share = r["fragile"].mean()
    assert share <= TR.FRAGILE_SHARE, (tag, share)
    # the pixels that did not use the history: the same set, bitwise copies
    assert np.array_equal((ln <= 1)[keep], r["copied"][keep]), tag
    assert np.array_equal((ln == 0)[keep], (r["hist_len"] == 0)[keep]), tag
    c = keep & r["copied"]
    assert np.array_equal(TR.bits(b)[c], TR.bits(b_in)[c]), tag
    e_b = TR.error(b, r["beauty"], scale, keep)
    e_l = TR.error(ln, r["hist_len"], 1.0, keep)
    e_q = 0.0
    if q is not None:
        assert np.array_equal(TR.bits(q)[c], TR.bits(q_in)[c]), tag
        e_q = TR.error(q, r["m2"], m2_scale, keep)
    print(f"{tag}: colour {e_b:.3g} m2 {e_q:.3g} hist_len {e_l:.3g} fragile {share:.4f} "
          f"L>1 {np.mean(ln > 1):.3f}")
    assert max(e_b, e_q, e_l) <= BOUND, tag
    return e_b, e_q, e_l


# ------------------------------------------------------------------ 1. the synthetic cases
@pytest.mark.parametrize("size", [f"{H}x{W}" for H, W in TC.SIZES])
@pytest.mark.parametrize("variant", list(TC.VARIANTS))
def test_synthetic_case_matches_the_reference(seqs, size, variant):
    s = seqs[size]
    m2, vom, kw = TC.VARIANTS[variant]
    p = s.params(m2=m2, vom=vom, **kw)
    ref = TR.TemporalRef()
    got = run_gpu(s, p, m2)
    used = 0
    for k in range(TC.FRAMES):
        r = ref.accumulate(s.cams[k], s.beauty[k], s.aov[k], p, m2=s.m2[k] if m2 else None)
        compare(f"{size} {variant} frame {k}", got[k], r, s.beauty[k], s.m2[k])
        used += int((got[k][2] > 1).sum())
    assert used >= 0.5 * (TC.FRAMES - 1) * s.H * s.W  # the history is in use


# ------------------------------------------------------------------ 2. static camera
def test_static_camera_running_mean_then_saturation():
    s = TC.Sequence(17, 33, frames=5, seed=7, static=True)
    hit = s.aov[0][..., rt.AOV_HITS] > 0
    worst = 0.0
    for max_history in (64.0, 3.0):
        got = run_gpu(s, s.params(m2=True, max_history=max_history), True)
        want = want_q = None
        for k in range(5):
            L = min(k + 1.0, max_history)
            b, q = s.beauty[k].astype(np.float64), s.m2[k].astype(np.float64)
            want = b if k == 0 else (1 - 1 / L) * want + b / L
            want_q = q if k == 0 else (1 - 1 / L) * want_q + q / L
            if max_history == 64.0:
                assert np.abs(want - np.mean([x.astype(np.float64) for x in s.beauty[:k + 1]],
                                             axis=0)).max() <= 1e-12  # the running mean
            gb, gq, gl = got[k]
            assert np.array_equal(gl[hit], np.full(hit.sum(), np.float32(L)))
            assert np.array_equal(gl[~hit], np.ones((~hit).sum(), np.float32))
            assert np.array_equal(TR.bits(gb)[~hit], TR.bits(s.beauty[k])[~hit])
            worst = max(worst, TR.error(gb, want, TC.SPP, hit), TR.error(gq, want_q, M2_SCALE, hit))
    print(f"static camera: worst error {worst:.3g}")
    assert worst <= BOUND


# ------------------------------------------------------------------ 3. the closed form
def test_half_pixel_shift_of_a_ramp_against_its_closed_form():
    cams, aovs, beauties, expect, full = TC.ramp_shift()
    H, W = full.shape
    p = rt.temporal_default_params(W, H)
    t = rt.Temporal()
    try:
        first = t.accumulate(cams[0], beauties[0], aovs[0], p)
        b, ln = t.accumulate(cams[1], beauties[1], aovs[1], p, hist_len=True)
    finally:
        t.close()
    assert np.array_equal(TR.bits(first), TR.bits(beauties[0]))
    assert np.array_equal(ln[full], np.full(full.sum(), np.float32(2)))
    e = TR.error(b, expect, TC.SPP, full)
    print(f"ramp shift: error {e:.3g}")
    assert e <= BOUND
    gone = np.broadcast_to(np.arange(W) + TC.RAMP_K + 0.5 >= W, (H, W))  # no tap in the frame
    assert np.array_equal(ln[gone], np.ones(gone.sum(), np.float32))
    assert np.array_equal(TR.bits(b)[gone], TR.bits(beauties[1])[gone])


# ------------------------------------------------------------------ 4. history state
def test_history_state_and_info():
    s, small = TC.Sequence(17, 33, frames=3, seed=9), TC.Sequence(3, 5, frames=1)
    p = s.params(m2=True)
    t = rt.Temporal()
    try:
        assert t.info() == dict(frames=0, width=0, height=0, moments=False)

        def call(k, params=p, seq=s, m2=True):
            return t.accumulate(seq.cams[k], seq.beauty[k], seq.aov[k], params,
                                m2=seq.m2[k] if m2 else None, hist_len=True)

        def is_copy(r, k, seq=s, m2=True):
            return (np.array_equal(TR.bits(r[0]), TR.bits(seq.beauty[k])) and
                    (not m2 or np.array_equal(TR.bits(r[1]), TR.bits(seq.m2[k]))) and
                    np.array_equal(r[-1], np.ones_like(r[-1])))

        assert is_copy(call(0), 0)  # the first call
        assert t.info() == dict(frames=1, width=33, height=17, moments=True)
        r = call(1)
        assert (r[-1] > 1).any() and not is_copy(r, 1)
        assert t.info()["frames"] == 2
        # a moments mismatch, both ways; the history stays as it was
        with pytest.raises(rt.RtError) as e:
            call(2, params=s.params(), m2=False)
        assert e.value.code == rt.RT_ERR_INVALID_ARG and t.info()["frames"] == 2
        # height == 0 touches nothing
        empty = s.cams[2].copy()
        empty.image_height = 0
        lib = rt.device_lib()
        assert lib.rt_temporal_accumulate_device(t._h, C.byref(s.params(height=0)), C.byref(empty),
                                                 C.c_void_p(8), None, C.c_void_p(8), C.c_void_p(8),
                                                 None, None, None, None) == rt.RT_OK
        assert t.info() == dict(frames=2, width=33, height=17, moments=True)
        # RESET: a copy, and the history may change its kind
        reset = s.params(flags=rt.RT_TEMPORAL_RESET)
        assert is_copy(call(2, params=reset, m2=False), 2, m2=False)
        assert t.info() == dict(frames=1, width=33, height=17, moments=False)
        with pytest.raises(rt.RtError) as e:
            call(2)
        assert e.value.code == rt.RT_ERR_INVALID_ARG
        assert (call(2, params=s.params(), m2=False)[-1] > 1).any()
        assert t.info()["frames"] == 2
        # a size change: a copy, again of either kind; then back
        assert is_copy(call(0, params=small.params(m2=True), seq=small), 0, seq=small)
        assert t.info() == dict(frames=1, width=5, height=3, moments=True)
        assert is_copy(call(1), 1)
        assert t.info() == dict(frames=1, width=33, height=17, moments=True)
    finally:
        t.close()


# ------------------------------------------------------------------ 5. NaN and inf
def test_non_finite_pixels_pass_through_and_are_no_ones_tap():
    s = TC.Sequence(17, 33, frames=3, seed=11, static=True)
    hit = s.aov[0][..., rt.AOV_HITS] > 0
    ys, xs = np.nonzero(hit)  # four pixels that have a position: the first, the last, two between
    bad = [(int(ys[k]), int(xs[k])) for k in (0, len(ys) // 3, len(ys) // 2, len(ys) - 1)]
    assert len(set(bad)) == 4
    b1, q1 = s.beauty[1].copy(), s.m2[1].copy()
    b1[bad[0]][1], b1[bad[1]][0], q1[bad[2]][2], b1[bad[3]] = np.nan, np.inf, -np.inf, np.nan
    b1[bad[3]][2] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]  # a NaN with a payload
    p = s.params(m2=True)
    t = rt.Temporal()
    try:
        t.accumulate(s.cams[0], s.beauty[0], s.aov[0], p, m2=s.m2[0])
        b, q, ln = t.accumulate(s.cams[1], b1, s.aov[1], p, m2=q1, hist_len=True)
        for y, x in bad:
            assert ln[y, x] == 0
            assert np.array_equal(TR.bits(b[y, x]), TR.bits(b1[y, x]))
            assert np.array_equal(TR.bits(q[y, x]), TR.bits(q1[y, x]))
        mask = np.ones_like(hit)
        for y, x in bad:
            mask[y, x] = False
        assert np.isfinite(b[mask]).all() and np.isfinite(q[mask]).all()
        assert np.array_equal(ln[mask & hit], np.full((mask & hit).sum(), np.float32(2)))
        # the next frame: the camera is still, so each bad pixel would be its own tap
        b, q, ln = t.accumulate(s.cams[2], s.beauty[2], s.aov[2], p, m2=s.m2[2], hist_len=True)
        assert np.isfinite(b).all() and np.isfinite(q).all()
        for y, x in bad:
            assert ln[y, x] == 1
            assert np.array_equal(TR.bits(b[y, x]), TR.bits(s.beauty[2][y, x]))
        assert np.array_equal(ln[mask & hit], np.full((mask & hit).sum(), np.float32(3)))
    finally:
        t.close()


# ------------------------------------------------------------------ 6. in place, streams, threads
def run_device(s, p, m2, stream=0, in_place=True):
    """the sequence through a fresh handle on device buffers: [(beauty, m2, hist_len)] of bits"""
    t = rt.Temporal()
    shape = (s.H, s.W, 3)
    bufs, out = [], []
    try:
        for k in range(len(s.cams)):
            b, a = DevBuf(shape, init=s.beauty[k]), DevBuf((s.H, s.W, rt.AOV_CHANNELS), init=s.aov[k])
            q = DevBuf(shape, init=s.m2[k]) if m2 else None
            ob = b if in_place else DevBuf(shape)
            oq = q if in_place or not m2 else DevBuf(shape)
            ln = DevBuf((s.H, s.W))
            bufs += [x for x in (b, a, q, ob, oq, ln) if x is not None]
            t.accumulate_device(p, s.cams[k], b.ptr, a.ptr, ob.ptr, q.ptr if m2 else 0,
                                oq.ptr if m2 else 0, ln.ptr, stream=stream)
            out.append((ob, oq, ln))
        res = [tuple(None if x is None else TR.bits(x.download()) for x in o) for o in out]
    finally:
        t.close()
        for x in {id(x): x for x in bufs}.values():
            x.free()
    return res


def same(a, b):
    return all(np.array_equal(x, y) if x is not None else y is None
               for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def test_in_place_streams_threads_and_determinism(seqs):
    s, s2 = seqs["61x64"], seqs["17x33"]
    p, p2 = s.params(m2=True, vom=True), s2.params()
    host = [tuple(None if x is None else TR.bits(x) for x in f) for f in run_gpu(s, p, True)]
    host2 = [tuple(None if x is None else TR.bits(x) for x in f) for f in run_gpu(s2, p2, False)]
    assert same(run_device(s, p, True, in_place=True), host)
    assert same(run_device(s, p, True, in_place=False), host)
    assert same(run_device(s2, p2, False, in_place=True), host2)
    st = Stream()
    try:
        assert same(run_device(s, p, True, stream=st.handle), host)
    finally:
        st.destroy()
    # two handles driven from two threads: each gives its serial result, bit for bit
    res, streams = {}, [Stream(), Stream()]

    def work(name, seq, params, m2, stream):
        res[name] = run_device(seq, params, m2, stream=stream.handle)

    th = [threading.Thread(target=work, args=("a", s, p, True, streams[0])),
          threading.Thread(target=work, args=("b", s2, p2, False, streams[1]))]
    try:
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        for x in streams:
            x.destroy()
    assert same(res["a"], host) and same(res["b"], host2)


def test_stats(seqs):
    s = seqs["17x33"]
    t = rt.Temporal()
    try:
        for m2, want in ((False, 12 + 4), (True, 24 + 4)):
            r = t.accumulate(s.cams[0], s.beauty[0], s.aov[0],
                             s.params(m2=m2, flags=rt.RT_TEMPORAL_RESET),
                             m2=s.m2[0] if m2 else None, hist_len=True, stats=True)
            st = r[-1]
            assert (st.samples, st.launches, st.out_bytes) == (17 * 33, 1, 17 * 33 * want)
            assert st.ms_kernel > 0 and st.ms_total >= st.ms_kernel and not any(st.ops)
    finally:
        t.close()


# ------------------------------------------------------------------ 7. end to end
@pytest.fixture(scope="module")
def cornell():
    sc = rt.Scene(1)
    w, l, cam = sc.preset("cornell_box", "", 64, 4, 8, 1.0)
    box = sc.bbox(w)
    pivot = [(box[0] + box[1]) / 2, (box[2] + box[3]) / 2, (box[4] + box[5]) / 2]
    ds = rt.DeviceScene(sc.serialize(w, l))
    yield ds, cam, pivot
    ds.close()


def render_frame(ds, cam, seed, bufs, overwrite=True):
    b, q, a = bufs
    o = rt.make_opts(cam, seed=seed, flags=rt.RT_FLAG_OVERWRITE if overwrite else 0)
    ds.render_moments_device(cam, o, b.ptr, q.ptr)
    ds.render_aov_device(cam, rt.make_opts(cam, seed=seed), a.ptr)


def test_cornell_orbit_end_to_end(cornell):
    ds, cam0, pivot = cornell
    H, W, B, n = cam0.image_height, cam0.image_width, cam0.samples_per_pixel, cam0.sqrt_spp
    assert (H, W, B, n) == (64, 64, 4, 2)
    p = rt.temporal_default_params(W, H)
    p.beauty_rows, p.flags = n, rt.RT_TEMPORAL_VARIANCE_OF_MEAN
    shape = (H, W, 3)
    bufs = (DevBuf(shape), DevBuf(shape), DevBuf((H, W, rt.AOV_CHANNELS)))
    ob, oq, ln = DevBuf(shape), DevBuf(shape), DevBuf((H, W))
    t, ref = rt.Temporal(), TR.TemporalRef()
    worst = 0.0
    try:
        for k in range(4):
            cam = rt.camera_orbit_y(cam0, pivot, 1.0 * k)
            render_frame(ds, cam, 1 + k, bufs)
            t.accumulate_device(p, cam, bufs[0].ptr, bufs[2].ptr, ob.ptr, bufs[1].ptr, oq.ptr,
                                ln.ptr)
            b_in, q_in, a_in = (x.download() for x in bufs)
            r = ref.accumulate(cam, b_in, a_in, p, m2=q_in)
            got = (ob.download(), oq.download(), ln.download())
            worst = max(worst, *compare(f"cornell frame {k}", got, r, b_in, q_in, scale=B,
                                        m2_scale=B * B / n))
            if k:
                assert np.mean(got[2] > 1) >= 0.5  # a turn of 1 degree keeps most of the frame
        print(f"cornell orbit: worst error {worst:.3g}")
        # the camera held still, seeds 1..4: where the history was taken every time, the four
        # renders' mean. Pixels on an edge may miss it (the material id is the first sample's, and
        # depth and normal are per-frame means): they are not compared, and by far most pixels of a
        # Cornell box are inside a wall, so at least 70 % must be.
        acc = (DevBuf(shape), DevBuf(shape), DevBuf((H, W, rt.AOV_CHANNELS)))
        p.flags = rt.RT_TEMPORAL_RESET
        try:
            for k in range(4):
                render_frame(ds, cam0, 1 + k, bufs)
                render_frame(ds, cam0, 1 + k, acc, overwrite=k == 0)
                t.accumulate_device(p, cam0, bufs[0].ptr, bufs[2].ptr, ob.ptr, bufs[1].ptr, oq.ptr,
                                    ln.ptr)
                p.flags = 0
            total, got, L = acc[0].download(), ob.download(), ln.download()
        finally:
            for x in acc:
                x.free()
        full = L == 4
        e = TR.error(got, total.astype(np.float64) / 4, B, full)
        print(f"cornell static: L == 4 at {full.mean():.3f} of the pixels, error {e:.3g}")
        assert full.mean() >= 0.7 and e <= BOUND
    finally:
        t.close()
        for x in bufs + (ob, oq, ln):
            x.free()
