"""Adaptive sampling, the parts that need no device: the pass schedule, the mirror of
rt_adaptive_params, and the argument checks that are made before the handle is read and before any
HIP call (so they answer RT_ERR_INVALID_ARG with no GPU present, given garbage handles)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import surely_rt as rt

HEADER = (Path(__file__).resolve().parent.parent / "include" / "rt_mi355x.h").read_text()
BOGUS = C.c_void_p(0x1000)  # never dereferenced: the checks come first


def test_schedule_partitions_the_rows_evenly():
    for S in range(2, 41):
        for P in range(1, S // 2 + 1):
            seen = []
            for p in range(P):
                b, step, n = rt.adaptive_schedule(S, P, p)
                assert (b, step) == (p, P)
                rows = [b + k * step for k in range(n)]
                assert rows and rows[-1] < S and rows[-1] + step >= S
                seen += rows
                if p == 0:
                    assert n >= 2
            assert sorted(seen) == list(range(S)), (S, P)


def test_schedule_rejects_invalid_pass_counts():
    for S, P, p in [(8, 0, 0), (8, 5, 0), (8, -1, 0), (3, 2, 0), (1, 1, 0), (8, 4, 4), (8, 4, -1),
                    (0, 0, 0)]:
        with pytest.raises(rt.RtError) as e:
            rt.adaptive_schedule(S, P, p)
        assert e.value.code == rt.RT_ERR_INVALID_ARG, (S, P, p)
    lib = rt.device_lib()
    one = C.c_int(0)
    assert lib.rt_adaptive_schedule(8, 2, 0, None, C.byref(one), C.byref(one)) == rt.RT_ERR_INVALID_ARG


def test_params_struct_mirrors_the_header():
    body = re.search(r"typedef struct rt_adaptive_params \{(.*?)\} rt_adaptive_params;", HEADER, re.S)
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = [d.split() for d in text.split(";") if d.strip()]
    sizes = {"int32_t": (4, C.c_int32), "double": (8, C.c_double)}
    off = 0
    assert [f[1] for f in fields] == [n for n, _ in rt.RtAdaptiveParams._fields_]
    for (ty, name), (pname, pty) in zip(fields, rt.RtAdaptiveParams._fields_):
        size, cty = sizes[ty]
        assert pty is cty and off % size == 0, name  # no padding before any field
        assert getattr(rt.RtAdaptiveParams, name).offset == off, name
        off += size
    assert off == 24 == C.sizeof(rt.RtAdaptiveParams)
    assert "24 bytes, no padding" in HEADER


def params(**kw):
    p = rt.RtAdaptiveParams()
    p.passes, p.min_passes, p.threshold, p.floor = 2, 1, 0.05, 1e-2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_tile_error_and_resolve_check_arguments_before_the_handle():
    lib = rt.device_lib()
    rows = np.full(6, 2, np.uint32)
    err = np.zeros(6, np.float32)
    buf = C.c_void_p(0x2000)  # a "device" pointer the checks never reach

    def te(ad=BOGUS, w=20, h=12, s=4, floor=1e-2, a=buf, q=buf, r=rows.ctypes.data, e=err.ctypes.data):
        return lib.rt_adaptive_tile_error(ad, w, h, s, floor, a, q, r, e, None, None)

    for bad in (dict(ad=None), dict(a=None), dict(q=None), dict(r=None), dict(e=None), dict(w=0),
                dict(w=-3), dict(h=-1), dict(s=0), dict(floor=0.0), dict(floor=-1.0),
                dict(floor=float("nan")), dict(floor=float("inf"))):
        assert te(**bad) == rt.RT_ERR_INVALID_ARG, bad
    rows[3] = 5  # more rows than sqrt_spp
    assert te() == rt.RT_ERR_INVALID_ARG
    rows[3] = 2

    def rs(ad=BOGUS, w=20, h=12, s=4, r=rows.ctypes.data, a=buf, o=buf):
        return lib.rt_adaptive_resolve_device(ad, w, h, s, r, a, o, None, None)

    for bad in (dict(ad=None), dict(r=None), dict(a=None), dict(o=None), dict(w=0), dict(h=-1),
                dict(s=0)):
        assert rs(**bad) == rt.RT_ERR_INVALID_ARG, bad
    rows[0] = 0  # a tile that holds nothing cannot be resolved
    assert rs() == rt.RT_ERR_INVALID_ARG
    assert lib.rt_adaptive_create(0, None) == rt.RT_ERR_INVALID_ARG


def test_driver_and_tile_render_check_arguments_before_the_handles():
    lib = rt.device_lib()
    blob, cam = rt.preset_blob("cornell_box", width=20, spp=16, depth=8, aspect=20 / 12)
    buf = C.c_void_p(0x2000)

    def drive(ad=BOGUS, sc=BOGUS, cam_=cam, o=None, p=None, a=buf, q=buf):
        o = rt.make_opts(cam) if o is None else o
        p = params() if p is None else p
        return lib.rt_render_adaptive_device(ad, sc, C.byref(cam_) if cam_ else None, C.byref(o),
                                             C.byref(p), a, q, None, None, None, None, None, None)

    for bad in (dict(ad=None), dict(sc=None), dict(cam_=None), dict(a=None), dict(q=None),
                dict(p=params(threshold=float("nan"))), dict(p=params(floor=0.0)),
                dict(p=params(floor=float("inf"))), dict(p=params(passes=0)),
                dict(p=params(passes=3)),  # sqrt_spp = 4: at most 2
                dict(p=params(min_passes=0)), dict(p=params(min_passes=3)),
                dict(o=rt.make_opts(cam, sj_begin=1)), dict(o=rt.make_opts(cam, sj_count=2)),
                dict(o=rt.make_opts(cam, flags=0)),
                dict(o=rt.make_opts(cam, flags=rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_COUNT_OPS))):
        assert drive(**bad) == rt.RT_ERR_INVALID_ARG, bad
    narrow = cam.copy()
    narrow.image_width = 0
    assert drive(cam_=narrow) == rt.RT_ERR_INVALID_ARG
    assert lib.rt_render_adaptive_device(BOGUS, BOGUS, C.byref(cam), C.byref(rt.make_opts(cam)),
                                         None, buf, buf, None, None, None, None, None,
                                         None) == rt.RT_ERR_INVALID_ARG

    # rt_render_tiles_device: the list and the flags are judged on the host
    def tiles(lst, o=None, step=1, sc=BOGUS):
        o = rt.make_opts(cam, sj_count=4) if o is None else o
        t = np.asarray(lst, np.uint32)
        return lib.rt_render_tiles_device(sc, C.byref(cam), C.byref(o), t.ctypes.data, t.size, step,
                                          buf, buf, None, None)

    for lst in ([2, 1], [0, 0], [1, 3, 3], [6], [0, 1, 2, 3, 4, 5, 6], [0xffffffff]):
        assert tiles(lst) == rt.RT_ERR_INVALID_ARG, lst
    assert tiles([0], step=0) == rt.RT_ERR_INVALID_ARG
    assert tiles([0], o=rt.make_opts(cam)) == rt.RT_ERR_INVALID_ARG  # sj_count 0 is not "all" here
    assert tiles([0], o=rt.make_opts(cam, sj_count=4, flags=rt.RT_FLAG_OVERWRITE |
                                     rt.RT_FLAG_COUNT_OPS)) == rt.RT_ERR_INVALID_ARG
    assert tiles([0], sc=None) == rt.RT_ERR_INVALID_ARG
    # nothing to do: RT_OK before the scene is read
    assert tiles([]) == rt.RT_OK
    assert tiles([], o=rt.make_opts(cam, n_rows=0, sj_count=4)) == rt.RT_OK


def test_plain_kernel_source_names_no_tile_list():
    """The generated walker that plain renders compile carries nothing of the variant."""
    blob, _ = rt.preset_blob("cornell_box", width=20, spp=16, depth=8, aspect=20 / 12)
    state, src = rt.jit_check(blob)
    assert state == 1 and "trace_body" not in src and "tile" not in src.lower()
