"""The adaptive sampler on the GPU: the tile error and resolve kernels on synthetic moments against
a numpy f64 evaluation of the header's formulas, and the driver against its own algorithm
re-enacted in Python over render_tiles_device and tile_error.

Bounds, derived: a tile error is the f32 rounding (2^-24) of an f64 value whose inputs keep
Q - S^2/n free of cancellation (every channel has Q >= 1.5 S^2/n or Q <= 0.5 S^2/n, the latter
clamped to 0), so the kernel's f64 evaluation and numpy's differ by a few 2^-53: 2^-22 relative
holds with room. With threshold -1 every tile takes all P passes, and each pass adds a
non-negative f64 pass total into the f32 sum with one rounding, against the one rounding of the
one-call frame: (P + 2) 2^-24 relative."""
import ctypes as C

import numpy as np
import pytest

import surely_rt as rt
from adaptive_cases import Case, bits, sentinel
from hip_buf import DevBuf, Stream

pytestmark = pytest.mark.gpu

W, H, S = 20, 12, 4
FLOOR = 1e-2


@pytest.fixture(scope="module")
def ad(gpu_available):
    a = rt.Adaptive()
    yield a
    a.close()


@pytest.fixture(scope="module")
def cases(gpu_available):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
        return made[name]

    yield get
    for c in made.values():
        c.ds.close()


def tile_of():
    y, x = np.mgrid[0:H, 0:W]
    return (y // 8) * 3 + x // 8


def synthetic(rows):
    """S >= 0 and Q with every channel either Q >= 1.6 S^2/n or Q <= 0.4 S^2/n"""
    g = np.random.default_rng(7)
    n = rows[tile_of()].astype(np.float64)[..., None]
    s = g.uniform(0.5, 4.0, (H, W, 3)).astype(np.float32)
    s[g.random((H, W, 3)) < 0.05] = 0.0  # black channels: the floor keeps them finite
    hi = g.random((H, W, 3)) < 0.6
    f = np.where(hi, g.uniform(1.6, 3.0, (H, W, 3)), g.uniform(0.0, 0.4, (H, W, 3)))
    q = (f * s.astype(np.float64) ** 2 / n).astype(np.float32)
    return s, q


def reference(s, q, rows):
    """per-pixel e of the header, f64; NaN where invalid"""
    n = rows[tile_of()].astype(np.float64)[..., None]
    B = n * S
    s, q = s.astype(np.float64), q.astype(np.float64)
    with np.errstate(all="ignore"):
        var = np.maximum(0.0, q - s * s / n) * n / ((n - 1.0) * B * B)
        e = np.sqrt(var.sum(-1)) / ((np.maximum(s, 0.0) / B).sum(-1) + FLOOR)
        ok = np.isfinite(s).all(-1) & np.isfinite(q).all(-1) & np.isfinite(e)
    return np.where(ok, e, np.nan)


def test_tile_error_against_numpy(ad):
    rows = np.array([2, 3, 4, 2, 3, 4], np.uint32)
    s, q = synthetic(rows)
    # invalid pixels: NaN and inf in S and in Q; tile 5 (x 16..19, y 8..11) wholly invalid
    s[0, 0, 1] = np.nan
    s[2, 9, 0] = np.inf
    q[3, 17, 2] = np.nan
    q[9, 1, 0] = np.inf
    q[10, 12, 1] = -np.inf
    s[8:12, 16:20, 0] = np.nan
    n_bad = 5 + 16
    e = reference(s, q, rows)
    assert np.isnan(e).sum() == n_bad
    want = np.array([np.nanmax(np.where(tile_of() == t, e, np.nan)) if t != 5 else 0.0
                     for t in range(6)])
    assert (want[:5] > 0).all()
    b, m = DevBuf((H, W, 3), init=s), DevBuf((H, W, 3), init=q)
    try:
        err, inv = ad.tile_error(W, H, S, FLOOR, b.ptr, m.ptr, rows)
        assert err.dtype == np.float32 and inv == n_bad
        assert err[5] == 0.0
        rel = np.abs(err[:5].astype(np.float64) - want[:5]) / want[:5]
        print("tile errors", err, "max rel", rel.max())
        assert (rel <= 2.0 ** -22).all()
        # a tile that holds one row has no estimate
        rows1 = rows.copy()
        rows1[1] = 1
        err1, inv1 = ad.tile_error(W, H, S, FLOOR, b.ptr, m.ptr, rows1)
        assert np.isposinf(err1[1]) and np.array_equal(np.delete(err1, 1), np.delete(err, 1))
        # its pixels are not examined: the planted inf at (2, 9) lies in tile 1
        assert inv1 == n_bad - 1
    finally:
        b.free()
        m.free()


def test_tile_error_clamps_negative_variances_to_zero(ad):
    rows = np.full(6, 4, np.uint32)
    s = np.full((H, W, 3), 2.0, np.float32)
    q = np.full((H, W, 3), 0.25, np.float32)  # far below S^2/n = 1: every term clamps
    q[5, 3] = 3.0                               # one pixel of tile 0 with a real variance
    b, m = DevBuf((H, W, 3), init=s), DevBuf((H, W, 3), init=q)
    try:
        err, inv = ad.tile_error(W, H, S, FLOOR, b.ptr, m.ptr, rows)
        assert inv == 0 and (err[1:] == 0.0).all()
        e = reference(s, q, rows)[5, 3]
        assert abs(float(err[0]) - e) <= 2.0 ** -22 * e
    finally:
        b.free()
        m.free()


def test_resolve_against_numpy(ad):
    rows = np.array([2, 3, 4, 1, 3, 4], np.uint32)
    g = np.random.default_rng(11)
    a = g.uniform(0.0, 50.0, (H, W, 3)).astype(np.float32)
    a.view(np.uint32)[1, 18, 2] = 0x7FC12345  # a NaN payload in a tile that holds every row
    n = rows[tile_of()].astype(np.float64)
    Bp = n * S
    want = (a.astype(np.float64) * ((S * S) / Bp)[..., None]).astype(np.float32)
    b, o, sm = DevBuf((H, W, 3), init=a), DevBuf((H, W, 3)), DevBuf((H, W))
    try:
        ad.resolve_device(W, H, S, rows, b.ptr, o.ptr, sm.ptr)
        out, smp = o.download(), sm.download()
        fullm = (n == S)
        assert np.array_equal(bits(out)[fullm], bits(a)[fullm])  # bitwise copy, payload included
        assert np.array_equal(bits(out)[~fullm], bits(want)[~fullm])
        assert np.array_equal(smp, Bp.astype(np.float32))
        assert np.array_equal(bits(b.download()), bits(a))
        # in place, and without the sample counts
        ad.resolve_device(W, H, S, rows, b.ptr, b.ptr)
        assert np.array_equal(bits(b.download()), bits(out))
    finally:
        b.free()
        o.free()
        sm.free()


def test_two_streams_through_one_handle_bitwise(gpu_available):
    """One handle's workspace and host copy of rows_held serve calls on two streams, small frame,
    large frame, small frame, ...: each call must wait for the one before it, through a workspace
    growth too. Bitwise against a fresh handle's serial results."""
    g = np.random.default_rng(5)
    sizes = [(20, 12), (72, 40)]  # 6 and 45 tiles
    rows = [g.integers(1, S + 1, int(np.prod(rt.tile_grid(w, h)))).astype(np.uint32)
            for w, h in sizes]
    assert [r.size for r in rows] == [6, 45]
    assert all(len(set(r.tolist())) > 1 for r in rows) and set(rows[1].tolist()) == {1, 2, 3, 4}
    accs = [g.uniform(0.0, 50.0, (h, w, 3)).astype(np.float32) for w, h in sizes]
    bufs = [(DevBuf(a.shape, init=a), DevBuf(a.shape), DevBuf(a.shape[:2])) for a in accs]
    streams = [Stream(0), Stream(0)]
    fresh, one = rt.Adaptive(), rt.Adaptive()
    try:
        serial = []
        for (w, h), r, (b, o, sm) in zip(sizes, rows, bufs):
            fresh.resolve_device(w, h, S, r, b.ptr, o.ptr, sm.ptr)
            serial.append((o.download(), sm.download()))
            o.upload(sentinel(o.shape))
            sm.upload(sentinel(sm.shape))
        assert all(np.isfinite(out).all() and (smp > 0).all() for out, smp in serial)
        for _ in range(3):
            for (w, h), r, (b, o, sm), s in zip(sizes, rows, bufs, streams):
                one.resolve_device(w, h, S, r, b.ptr, o.ptr, sm.ptr, stream=s.handle)
        for s in streams:
            s.sync()
        for (b, o, sm), (out, smp) in zip(bufs, serial):
            assert np.array_equal(bits(o.download()), bits(out))
            assert np.array_equal(bits(sm.download()), bits(smp))
    finally:
        for s in streams:
            s.destroy()
        for t in bufs:
            for d in t:
                d.free()
        fresh.close()
        one.close()


def params(P, min_passes, threshold):
    p = rt.RtAdaptiveParams()
    p.passes, p.min_passes, p.threshold, p.floor = P, min_passes, threshold, FLOOR
    return p


def enact(c, ad, P, min_passes, threshold, acc, m2):
    """The header's algorithm over render_tiles_device and tile_error. threshold None: stop at the
    first error evaluation and return the errors of the active tiles."""
    active = np.arange(c.n_tiles, dtype=np.uint32)
    held = np.zeros(c.n_tiles, np.uint32)
    per = np.zeros(P, np.uint32)
    samples = 0
    for p in range(P):
        if active.size == 0:
            break
        b, step, n = rt.adaptive_schedule(c.S, P, p)
        st = c.ds.render_tiles_device(c.cam, c.opts(overwrite=(p == 0), sj_begin=b, sj_count=n),
                                      active, step, acc.ptr, m2.ptr, stats=True)
        samples += st.samples
        per[p] = active.size
        held[active] += n
        if p + 1 >= min_passes and p + 1 < P:
            err, _ = ad.tile_error(c.W, c.H, c.S, FLOOR, acc.ptr, m2.ptr, held)
            if threshold is None:
                return err[active]
            active = active[err[active] > threshold]
    return held, per, samples


@pytest.mark.parametrize("name,P,min_passes", [("cornell64", 4, 2), ("final16", 2, 1)])
def test_driver_is_its_algorithm_re_enacted(cases, ad, name, P, min_passes):
    c = cases(name)
    acc, m2 = DevBuf(c.shape, init=sentinel(c.shape)), DevBuf(c.shape, init=sentinel(c.shape))
    dacc, dm2 = DevBuf(c.shape, init=sentinel(c.shape)), DevBuf(c.shape, init=sentinel(c.shape))
    try:
        seen = np.sort(enact(c, ad, P, min_passes, None, acc, m2).astype(np.float64))
        thr = float(np.median(seen))
        if not ((seen > thr).any() and (seen <= thr).any()):
            distinct = np.unique(seen)
            assert distinct.size >= 2, seen
            thr = float(distinct[0] + distinct[1]) / 2
        held, per, samples = enact(c, ad, P, min_passes, thr, acc, m2)
        assert held.min() < held.max(), "some tile stops early and some tile continues"
        drows, dper, st = ad.render_device(c.ds, c.cam, c.opts(), params(P, min_passes, thr),
                                           dacc.ptr, dm2.ptr)
        assert np.array_equal(drows, held) and np.array_equal(dper, per)
        assert np.array_equal(bits(dacc.download()), bits(acc.download()))
        assert np.array_equal(bits(dm2.download()), bits(m2.download()))
        px = c.mask(range(c.n_tiles))  # all pixels; per-tile pixel counts below
        per_px = np.array([c.mask([t]).sum() for t in range(c.n_tiles)])
        assert px.all() and st.samples == samples == int((per_px * held).sum()) * c.S
        assert (np.diff(dper.astype(np.int64)) <= 0).all() and dper[0] == c.n_tiles
        assert st.launches >= int((dper > 0).sum()) and st.ms_kernel > 0 and st.ms_total > 0
    finally:
        for b in (acc, m2, dacc, dm2):
            b.free()


def test_threshold_extremes(cases, ad):
    c = cases("cornell64")
    P = 4
    acc, m2, out, smp = DevBuf(c.shape), DevBuf(c.shape), DevBuf(c.shape), DevBuf((c.H, c.W))
    try:
        # +inf: nothing continues past min_passes
        rows, per, st = ad.render_device(c.ds, c.cam, c.opts(), params(P, 2, float("inf")),
                                         acc.ptr, m2.ptr, out.ptr, smp.ptr)
        n01 = rt.adaptive_schedule(c.S, P, 0)[2] + rt.adaptive_schedule(c.S, P, 1)[2]
        assert list(per) == [c.n_tiles, c.n_tiles, 0, 0] and (rows == n01).all()
        assert st.samples == c.H * c.W * n01 * c.S
        assert (smp.download() == n01 * c.S).all()
        want = (acc.download().astype(np.float64) * (c.S * c.S / (n01 * c.S))).astype(np.float32)
        assert np.array_equal(bits(out.download()), bits(want))
        # -1: every pass on every tile
        rows, per, st = ad.render_device(c.ds, c.cam, c.opts(), params(P, 1, -1.0),
                                         acc.ptr, m2.ptr, out.ptr, smp.ptr)
        assert list(per) == [c.n_tiles] * P and (rows == c.S).all()
        assert st.samples == c.W * c.H * c.S * c.S and (smp.download() == c.S * c.S).all()
        a = acc.download()
        assert np.array_equal(bits(out.download()), bits(a))  # every row held: a copy
        full = c.full()[0].astype(np.float64)
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(full) & np.isfinite(a)
            assert np.array_equal(np.isfinite(full), np.isfinite(a))
            d = np.abs(a.astype(np.float64) - full)[fin]
            print("threshold -1: max rel", (d / np.maximum(full[fin], 1e-300)).max())
            assert (d <= (P + 2) * 2.0 ** -24 * full[fin]).all()
        # the host-buffer convenience is the same driver
        hout, hsmp, hrows, hper, hst = ad.render(c.ds, c.cam, c.opts(), params(P, 1, -1.0))
        assert np.array_equal(bits(hout), bits(a)) and (hsmp == c.S * c.S).all()
        assert np.array_equal(hrows, rows) and hst.samples == st.samples
    finally:
        for b in (acc, m2, out, smp):
            b.free()
