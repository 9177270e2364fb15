"""rt_render_tiles_device on the GPU against the entry points it restricts: with the full list and
stride 1 it is rt_render_moments_device bit for bit; a partial list touches the listed tiles only; a
single strided row is rt_render_device's; and neither the launch's split into item kinds nor its
chunking changes a bit.

The one bound is derived: with a, b the f32 single-row renders of rows 0 and 2 and x the f32 render
of both, each is one f32 rounding (relative 2^-24) of a non-negative f64 row total (x of their f64
sum), so |x - (a + b)| <= 2^-24 (A + B) + 2^-24 (A + B) (1 + 2^-24) < 2^-22 (a + b)."""
import ctypes as C

import numpy as np
import pytest

import surely_rt as rt
from adaptive_cases import CASES, Case, bits, sentinel
from hip_buf import DevBuf

pytestmark = pytest.mark.gpu

# The full-list test alone also runs the tile-list variants of two more ahead-of-time kernels (the
# interpreter walker: no hiprtc compile), 16 x 16 each: the staged volume kernel and the staged
# textured one.
FULL_LIST_CASES = {
    "smoke16": ("cornell_smoke", dict(width=16, spp=16, depth=8), rt.RT_FLAG_INTERPRETER),
    "perlin16": ("two_perlin_spheres", dict(width=16, spp=16, depth=8, aspect=1.0),
                 rt.RT_FLAG_INTERPRETER),
}


@pytest.fixture(scope="module")
def cases(gpu_available):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, FULL_LIST_CASES.get(name))
        return made[name]

    yield get
    for c in made.values():
        c.ds.close()


@pytest.mark.parametrize("name", list(CASES) + list(FULL_LIST_CASES))
def test_full_list_stride_one_is_the_moments_render(cases, name):
    c = cases(name)
    assert (c.H, c.W) == ((12, 20) if name.startswith("cornell") else (16, 16))
    everything = np.arange(c.n_tiles)
    base = np.full(c.shape, 3.0, np.float32)
    for rng in (dict(sj_begin=0, sj_count=c.S), dict(sj_begin=1, sj_count=2)):
        want_a, want_q = c.full() if rng["sj_count"] == c.S else c.moments(c.opts(**rng))
        a, q, st = c.tiles(everything, c.opts(**rng), stats=True)
        assert np.array_equal(bits(a), bits(want_a)) and np.array_equal(bits(q), bits(want_q)), rng
        assert st.samples == c.H * c.W * rng["sj_count"] * c.S and st.launches == 1
        # adding into a non-zero buffer
        want_a, want_q = c.moments(c.opts(overwrite=False, **rng), init=base, init2=base)
        a, q = c.tiles(everything, c.opts(overwrite=False, **rng), init=base, init2=base)
        assert np.array_equal(bits(a), bits(want_a)) and np.array_equal(bits(q), bits(want_q)), rng


@pytest.mark.parametrize("name,lists", [("cornell16", ([0, 2, 5], [4])),
                                        ("final16", ([0, 3], [2]))])
def test_partial_list_touches_the_listed_tiles_only(cases, name, lists):
    c = cases(name)
    want_a, want_q = c.full()
    for lst in lists:
        a, q, st = c.tiles(lst, c.opts(sj_count=c.S), init=sentinel(c.shape),
                           init2=sentinel(c.shape), stats=True)
        m = c.mask(lst)
        assert 0 < m.sum() < m.size and st.samples == int(m.sum()) * c.S * c.S
        for got, want in ((a, want_a), (q, want_q)):
            assert np.array_equal(bits(got)[m], bits(want)[m]), lst
            assert np.array_equal(bits(got)[~m], bits(sentinel(c.shape))[~m]), lst
        # without the second buffer: the same sums
        a1, _ = c.tiles(lst, c.opts(sj_count=c.S), init=sentinel(c.shape), m2=False)
        assert np.array_equal(bits(a1), bits(a)), lst


@pytest.mark.parametrize("name", ["cornell16", "final16"])
def test_single_rows_are_the_plain_render_of_that_row(cases, name):
    c = cases(name)
    everything = np.arange(c.n_tiles)
    for r in range(c.S):
        a, _ = c.tiles(everything, c.opts(sj_begin=r, sj_count=1), step=c.S, m2=False)
        assert np.array_equal(bits(a), bits(c.row(r))), r


@pytest.mark.parametrize("name", ["cornell16", "final16"])
def test_strided_rows_sum_the_rows_of_the_stride(cases, name):
    c = cases(name)
    assert c.S == 4
    x, _ = c.tiles(np.arange(c.n_tiles), c.opts(sj_begin=0, sj_count=2), step=2)
    x = x.astype(np.float64)
    ab = c.row(0).astype(np.float64) + c.row(2).astype(np.float64)
    wrong = c.row(0).astype(np.float64) + c.row(1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(ab) & np.isfinite(x)
        assert fin.sum() > 0.9 * fin.size
        d = np.abs(x - ab)[fin]
        print(f"{name}: max |x - (a + b)| / (a + b) = {(d / np.maximum(ab[fin], 1e-300)).max():.3e}")
        assert (d <= 2.0 ** -22 * ab[fin]).all()
        # a dropped stride (rows 0 and 1) is told apart
        fin2 = fin & np.isfinite(wrong)
        assert (np.abs(x - wrong)[fin2] > 2.0 ** -22 * wrong[fin2]).any()


def test_chunks_and_item_kinds_leave_the_bits_unchanged(cases, monkeypatch):
    c = cases("cornell64")
    assert c.S == 8
    lst, o, step = [1, 2, 4], c.opts(sj_begin=1, sj_count=4), 2  # rows 1, 3, 5, 7: 12 pairs
    a, q, st = c.tiles(lst, o, step=step, init=sentinel(c.shape), init2=sentinel(c.shape), stats=True)
    assert st.launches == 1
    plain = c.plain(c.opts())
    envs = [{"RT_WORKSPACE_MB": 0},                       # one stratum row per chunk: the compact carry
            {"RT_SEG_PAIRS": 0, "RT_TAIL_PAIRS": 0},      # row items only
            {"RT_SEG_PAIRS": 5, "RT_TAIL_PAIRS": 3},      # row, segment and tail items
            {"RT_TAIL_PAIRS": 0},                         # segment items only
            {"RT_TAIL_PAIRS": 1 << 30},                   # tail items only
            {"RT_SEG_PAIRS": 2, "RT_TAIL_PAIRS": 1, "RT_WORKSPACE_MB": 0}]
    for env in envs:
        for k in ("RT_SEG_PAIRS", "RT_TAIL_PAIRS", "RT_WORKSPACE_MB"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        a2, q2, st2 = c.tiles(lst, o, step=step, init=sentinel(c.shape), init2=sentinel(c.shape),
                              stats=True)
        if "RT_WORKSPACE_MB" in env:
            assert st2.launches > 1, env
        assert np.array_equal(bits(a2), bits(a)) and np.array_equal(bits(q2), bits(q)), env
    for k in ("RT_SEG_PAIRS", "RT_TAIL_PAIRS", "RT_WORKSPACE_MB"):
        monkeypatch.delenv(k, raising=False)
    # and the strided chunks are the rows they name
    m = c.mask(lst)
    want = sum(c.row(r).astype(np.float64) for r in (1, 3, 5, 7))
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(want) & m[..., None]
        assert (np.abs(a.astype(np.float64) - want)[fin] <= 2.0 ** -21 * want[fin]).all()
    assert np.array_equal(bits(c.plain(c.opts())), bits(plain))


def test_rejected_arguments_start_no_kernel(cases):
    c = cases("cornell16")
    s = sentinel(c.shape)
    b, q = DevBuf(c.shape, init=s), DevBuf(c.shape, init=s)
    try:
        o = c.opts(sj_count=c.S)
        for lst in ([2, 1], [0, 0], [1, 3, 3], [c.n_tiles], [0, c.n_tiles]):
            with pytest.raises(rt.RtError) as e:
                c.ds.render_tiles_device(c.cam, o, lst, 1, b.ptr, q.ptr)
            assert e.value.code == rt.RT_ERR_INVALID_ARG, lst
        counting = c.opts(sj_count=c.S)
        counting.flags |= rt.RT_FLAG_COUNT_OPS
        for bad, step in ((counting, 1),
                          (c.opts(sj_begin=1, sj_count=2), 3),   # rows 1, 4: past sqrt_spp = 4
                          (c.opts(sj_count=0), 1), (o, 0)):
            with pytest.raises(rt.RtError) as e:
                c.ds.render_tiles_device(c.cam, bad, [0], step, b.ptr, q.ptr)
            assert e.value.code == rt.RT_ERR_INVALID_ARG
        st = c.ds.render_tiles_device(c.cam, o, [], 1, b.ptr, q.ptr, stats=True)
        assert st.samples == 0 and st.launches == 0
        assert np.array_equal(bits(b.download()), bits(s)) and np.array_equal(bits(q.download()), bits(s))
    finally:
        b.free()
        q.free()


def test_plain_renders_are_unchanged_by_tile_renders(cases):
    c = cases("cornell16")
    before = c.plain(c.opts())
    c.tiles([0, 2, 5], c.opts(sj_count=c.S))
    c.tiles([3], c.opts(sj_begin=1, sj_count=1), step=c.S, m2=False)
    assert np.array_equal(bits(c.plain(c.opts())), bits(before))
    state, msg = c.ds.jit_info()
    assert state == 1, msg
    f = cases("final16")
    before = f.plain(f.opts())
    f.tiles([1, 2], f.opts(sj_count=f.S))
    assert np.array_equal(bits(f.plain(f.opts())), bits(before))
    # the walker of final_scene's tile render may also be the scene-specialised one or the
    # reference-order BVH walk: same bits
    a0, q0 = f.tiles([1, 2], f.opts(sj_count=f.S))
    o = f.opts(sj_count=f.S)
    o.flags |= rt.RT_FLAG_REFERENCE_BVH
    a1, q1 = f.tiles([1, 2], o)
    assert np.array_equal(bits(a1), bits(a0)) and np.array_equal(bits(q1), bits(q0))
