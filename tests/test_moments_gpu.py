"""rt_render_moments* on the GPU: the beauty sums stay rt_render_device's bit for bit, and m2 is the
sum over the call's stratum rows of the squared f64 row totals.

The bound on m2 against per-row renders is derived, not measured: a per-row render through
rt_render_device gives (float)R_j, off by at most 2^-24 relative, so its square is off by at most
2^-23; all terms are non-negative; rounding the result to f32 adds 2^-24. REL = 2^-22 sits above
the sum. Against the f64 oracle the bound is the project's per-sample tolerance TOL (1e-4,
tests/test_gpu_parity.py) carried through the square: with m samples per row,
|dQ| <= sum_j (2 |R_j| TOL m + (TOL m)^2) + 2^-22 Q."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
from hip_buf import DevBuf

pytestmark = pytest.mark.gpu

REL = 2.0 ** -22
TOL = 1e-4  # per sample, as tests/test_gpu_parity.py

CASES = {
    "cornell16": ("cornell_box", dict(width=20, spp=16, depth=8, aspect=20 / 12), 0),
    "cornell49": ("cornell_box", dict(width=20, spp=49, depth=8, aspect=20 / 12), 0),
    # the BVH kernels; the interpreter walker gives the scene-specialised kernel's bits without
    # its compilation
    "final16": ("final_scene", dict(width=16, spp=16, depth=8), rt.RT_FLAG_INTERPRETER),
}


class Case:
    def __init__(self, name):
        scene, kw, self.flags = CASES[name]
        self.blob, self.cam = rt.preset_blob(scene, **kw)
        self.ds = rt.DeviceScene(self.blob)
        self.H, self.W, self.S = self.cam.image_height, self.cam.image_width, self.cam.sqrt_spp

    def opts(self, overwrite=True, **kw):
        f = self.flags | (rt.RT_FLAG_OVERWRITE if overwrite else 0)
        return rt.make_opts(self.cam, seed=1, flags=f, **kw)

    def shape(self, o):
        return (o.n_rows, self.W, 3)

    def plain(self, o, init=None):
        """rt_render_device -> accum"""
        b = DevBuf(self.shape(o), init=init)
        try:
            self.ds.render_device(self.cam, o, b.ptr)
            return b.download()
        finally:
            b.free()

    def moments(self, o, init=None, init2=None, stats=False):
        """rt_render_moments_device -> (accum, m2[, stats])"""
        b, q = DevBuf(self.shape(o), init=init), DevBuf(self.shape(o), init=init2)
        try:
            st = self.ds.render_moments_device(self.cam, o, b.ptr, q.ptr, stats=stats)
            return (b.download(), q.download(), st) if stats else (b.download(), q.download())
        finally:
            b.free()
            q.free()

    def rows_ref(self, sj0=0, n_sj=None, **kw):
        """Q from per-row renders of rt_render_device: sum_j (double)(float)R_j ^ 2"""
        Q = None
        for j in range(sj0, sj0 + (self.S if n_sj is None else n_sj)):
            r = self.plain(self.opts(sj_begin=j, sj_count=1, **kw)).astype(np.float64)
            Q = r * r if Q is None else Q + r * r
        return Q


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def close_to(m2, Q_ref, what):
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(Q_ref)
        assert np.array_equal(fin, np.isfinite(m2)), f"{what}: non-finite masks differ"
        rel = np.abs(m2.astype(np.float64)[fin] - Q_ref[fin]) / np.maximum(Q_ref[fin], 1e-300)
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{what}: max |m2 - Q_ref| / Q_ref = {worst:.3e} (bound {REL:.3e})")
    assert worst <= REL, (what, worst)


@pytest.mark.parametrize("name", list(CASES))
def test_accum_bits_m2_against_per_row_renders_and_repeatability(cases, name):
    c = cases(name)
    assert (c.H, c.W) == ((12, 20) if name.startswith("cornell") else (16, 16))
    o = c.opts()
    want = c.plain(o)
    acc, m2, st = c.moments(o, stats=True)
    assert np.array_equal(bits(acc), bits(want))
    assert st.samples == c.H * c.W * c.S * c.S and st.launches == 1 and st.ms_kernel > 0
    acc2, m2b = c.moments(o)
    assert np.array_equal(bits(acc2), bits(want)) and np.array_equal(bits(m2), bits(m2b))
    # the host entry point
    hacc, hm2, hst = c.ds.render_moments(c.cam, o, stats=True)
    assert np.array_equal(bits(hacc), bits(want)) and np.array_equal(bits(hm2), bits(m2))
    assert hst.samples == st.samples
    close_to(m2, c.rows_ref(), name)
    # Q >= S^2 / n up to rounding: the variance estimate is not dominated by cancellation noise
    S, Q = acc.astype(np.float64), m2.astype(np.float64)
    fin = np.isfinite(S) & np.isfinite(Q)
    assert (Q[fin] >= S[fin] ** 2 / c.S * (1 - 4 * REL)).all()


ENVS = [{"RT_SEG_PAIRS": 5, "RT_TAIL_PAIRS": 3},       # row, segment and tail items (42 pairs)
        {"RT_SEG_PAIRS": 0, "RT_TAIL_PAIRS": 0},       # row items only
        {"RT_TAIL_PAIRS": 0},                          # segment items only
        {"RT_TAIL_PAIRS": 1 << 30},                    # tail items only
        # one stratum row per chunk (the whole 20x12x49 frame needs under 1 MB): the carry buffer;
        # then each chunk's 6 pairs as 3 row, 2 segment and 1 tail items
        {"RT_WORKSPACE_MB": 0},
        {"RT_SEG_PAIRS": 2, "RT_TAIL_PAIRS": 1, "RT_WORKSPACE_MB": 0}]


@pytest.mark.parametrize("name", ["cornell49"])
def test_item_kinds_and_chunking_leave_the_bits_unchanged(cases, monkeypatch, name):
    c = cases(name)
    o = c.opts()
    acc, m2 = c.moments(o)
    for env in ENVS:
        for k in ("RT_SEG_PAIRS", "RT_TAIL_PAIRS", "RT_WORKSPACE_MB"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        a, q, st = c.moments(o, stats=True)
        if "RT_WORKSPACE_MB" in env:
            assert st.launches > 1, (env, st.launches)
        assert np.array_equal(bits(a), bits(acc)), env
        assert np.array_equal(bits(q), bits(m2)), env
        # a plain render after a chunked moments render on the same slot is still itself
        assert np.array_equal(bits(c.plain(o)), bits(acc)), env


@pytest.mark.parametrize("name,rows", [("cornell16", {}),
                                       ("cornell16", dict(row_begin=1, row_step=3, n_rows=4))])
def test_accumulating_calls_compose(cases, name, rows):
    c = cases(name)
    assert c.S == 4
    whole_a, whole_q = c.moments(c.opts(**rows))
    lo, hi = dict(sj_begin=0, sj_count=2, **rows), dict(sj_begin=2, sj_count=2, **rows)
    # accum: exactly what two rt_render_device calls give
    want = c.plain(c.opts(overwrite=False, **hi), init=c.plain(c.opts(**lo)))
    a, q = c.moments(c.opts(**lo))
    close_to(q, c.rows_ref(0, 2, **rows), "first half")
    a, q = c.moments(c.opts(overwrite=False, **hi), init=a, init2=q)
    assert np.array_equal(bits(a), bits(want))
    close_to(q, whole_q.astype(np.float64), f"composition {rows}")
    close_to(q, c.rows_ref(**rows), f"composition against the rows {rows}")
    # accumulate mode adds to what the buffers hold
    base = np.full(whole_a.shape, 3.0, np.float32)
    a, q = c.moments(c.opts(overwrite=False, **rows), init=base, init2=base)
    assert np.array_equal(bits(a), bits(c.plain(c.opts(overwrite=False, **rows), init=base)))
    close_to(q, 3.0 + whole_q.astype(np.float64), "accumulate onto 3.0")


@pytest.mark.parametrize("name", ["cornell16", "cornell49"])
def test_m2_against_the_f64_oracle(cases, name):
    c = cases(name)
    _, m2 = c.moments(c.opts())
    m = c.S  # samples per stratum row
    Q = np.zeros((c.H, c.W, 3))
    slack = np.zeros((c.H, c.W, 3))
    for j in range(c.S):
        r, _ = O.render(c.blob, c.cam, rt.make_opts(c.cam, seed=1, sj_begin=j, sj_count=1),
                        precision=64)
        r = r.astype(np.float64)
        Q += r * r
        slack += 2 * np.abs(r) * TOL * m + (TOL * m) ** 2
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(Q)
        assert np.array_equal(fin, np.isfinite(m2))
        d = np.abs(m2.astype(np.float64) - Q)[fin]
        bound = (slack + REL * Q)[fin]
    print(f"{name}: max |m2 - Q_oracle| = {d.max():.3e}, largest share of its bound "
          f"{(d / bound).max():.3e}")
    assert (d <= bound).all()


def test_error_paths_start_no_kernel(cases):
    c = cases("cornell16")
    o = c.opts()
    sentinel = np.full(c.shape(o), 7.25, np.float32)
    b, q = DevBuf(sentinel.shape, init=sentinel), DevBuf(sentinel.shape, init=sentinel)
    try:
        lib = rt.device_lib()
        rc = lib.rt_render_moments_device(c.ds._h, C.byref(c.cam), C.byref(o), C.c_void_p(b.ptr),
                                          None, None, None)
        assert rc == rt.RT_ERR_INVALID_ARG and b"null" in lib.rt_last_error()
        rc = lib.rt_render_moments_device(c.ds._h, C.byref(c.cam), C.byref(o), None,
                                          C.c_void_p(q.ptr), None, None)
        assert rc == rt.RT_ERR_INVALID_ARG
        o0 = c.opts(n_rows=0)
        st = c.ds.render_moments_device(c.cam, o0, b.ptr, q.ptr, stats=True)
        assert st.samples == 0 and st.launches == 0 and st.out_bytes == 0
        bad = c.opts(sj_begin=3, sj_count=5)
        with pytest.raises(rt.RtError) as e:
            c.ds.render_moments_device(c.cam, bad, b.ptr, q.ptr)
        assert e.value.code == rt.RT_ERR_INVALID_ARG
        assert np.array_equal(b.download(), sentinel) and np.array_equal(q.download(), sentinel)
        # the scene still renders
        a, m2 = c.moments(o)
        assert np.array_equal(bits(a), bits(c.plain(o))) and np.isfinite(m2).all()
    finally:
        b.free()
        q.free()
