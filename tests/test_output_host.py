"""The device output stage, the parts that need no device: the mirror of rt_output_params and the
argument checks that are made before the handle is read and before any HIP call (so they answer
RT_ERR_INVALID_ARG with no GPU present, given a garbage handle and garbage buffer pointers)."""
import ctypes as C
import re
from pathlib import Path

import surely_rt as rt

HEADER = (Path(__file__).resolve().parent.parent / "include" / "rt_mi355x.h").read_text()
BOGUS = C.c_void_p(0x1000)  # never dereferenced: the checks come first
BUF = C.c_void_p(0x2000)  # a "buffer" the checks never reach
INF, NAN = float("inf"), float("nan")


def test_params_struct_mirrors_the_header():
    body = re.search(r"typedef struct rt_output_params \{(.*?)\} rt_output_params;", HEADER, re.S)
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    sizes = {"int32_t": (4, C.c_int32), "uint32_t": (4, C.c_uint32), "double": (8, C.c_double)}
    fields = []  # (type, name), a declaration may name several fields
    for decl in (d.strip() for d in text.split(";")):
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(ty, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in rt.RtOutputParams._fields_]
    off = 0
    for (ty, name), (_, pty) in zip(fields, rt.RtOutputParams._fields_):
        size, cty = sizes[ty]
        assert pty is cty and off % size == 0, name  # no padding before any field
        assert getattr(rt.RtOutputParams, name).offset == off, name
        off += size
    assert off == 32 == C.sizeof(rt.RtOutputParams)
    assert "32 bytes, no padding" in HEADER


def test_flag_constants_match_the_header():
    defs = dict(re.findall(r"#define (RT_OUTPUT_\w+)\s+(0x[0-9a-fA-F]+)u", HEADER))
    assert len(defs) == 3
    for name, value in defs.items():
        assert getattr(rt, name) == int(value, 16), name


def test_output_params_sets_the_flags():
    p = rt.output_params(7, 5, 16)
    assert (p.width, p.height, p.flags, p._pad0, p.samples_per_pixel) == (7, 5, 0, 0, 16.0)
    p = rt.output_params(7, 5, 16, exposure=0.37, rgba=True)
    assert p.flags == rt.RT_OUTPUT_EXPOSURE | rt.RT_OUTPUT_RGBA and p.exposure == 0.37
    p = rt.output_params(7, 5, 16, exposure=0.37, auto=True)
    assert p.flags == rt.RT_OUTPUT_AUTO_EXPOSE and p.exposure == 0.0


def _calls():
    lib = rt.device_lib()

    def device(o, p, s, b):
        return lib.rt_output_device(o, C.byref(p) if p is not None else None, s, b, None, None,
                                    None)

    def host(o, p, s, b):
        return lib.rt_output(o, C.byref(p) if p is not None else None, s, b, None, None)

    return {"rt_output_device": device, "rt_output": host}


def _params(**kw):
    p = rt.output_params(20, 12, 16)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_arguments_are_checked_before_the_handle():
    exp = rt.RT_OUTPUT_EXPOSURE
    bad_params = [dict(width=0), dict(width=-3), dict(height=-1),
                  dict(width=65536, height=32768),  # width * height = 2^31
                  dict(width=2 ** 31 - 1, height=2 ** 31 - 1),
                  dict(samples_per_pixel=0.0), dict(samples_per_pixel=-4.0),
                  dict(samples_per_pixel=NAN), dict(samples_per_pixel=INF),
                  dict(flags=exp, exposure=NAN), dict(flags=exp, exposure=INF),
                  dict(flags=exp, exposure=-INF),
                  dict(flags=exp | rt.RT_OUTPUT_RGBA, exposure=NAN),
                  dict(flags=0x8), dict(flags=0x80000000), dict(flags=exp | 0x10),
                  dict(_pad0=1), dict(_pad0=-1)]
    for name, call in _calls().items():
        assert call(BOGUS, None, BUF, BUF) == rt.RT_ERR_INVALID_ARG, name
        assert call(BOGUS, _params(), None, BUF) == rt.RT_ERR_INVALID_ARG, name
        assert call(BOGUS, _params(), BUF, None) == rt.RT_ERR_INVALID_ARG, name
        assert call(None, _params(), BUF, BUF) == rt.RT_ERR_INVALID_ARG, name
        for bad in bad_params:
            assert call(BOGUS, _params(**bad), BUF, BUF) == rt.RT_ERR_INVALID_ARG, (name, bad)
    assert rt.device_lib().rt_output_create(0, None) == rt.RT_ERR_INVALID_ARG


def test_an_empty_frame_is_ok_and_reads_nothing():
    auto = rt.RT_OUTPUT_AUTO_EXPOSE
    for name, call in _calls().items():
        assert call(BOGUS, _params(height=0), BUF, BUF) == rt.RT_OK, name
        # a non-finite exposure is ignored where no flag, or auto-exposure, says so
        assert call(BOGUS, _params(height=0, exposure=NAN), BUF, BUF) == rt.RT_OK, name
        assert call(BOGUS, _params(height=0, flags=auto | rt.RT_OUTPUT_EXPOSURE, exposure=NAN),
                    BUF, BUF) == rt.RT_OK, name
        # the largest frame the checks let through
        assert call(BOGUS, _params(width=2 ** 31 - 1, height=0), BUF, BUF) == rt.RT_OK, name


def test_abi_version_is_unchanged():
    assert rt.device_lib().rt_abi_version() == 3
    assert re.search(r"#define RT_ABI_VERSION 3\b", HEADER)
