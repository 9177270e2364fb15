"""First-hit AOV pass, host side (no GPU): the Python constants mirror the header's RT_AOV_*
defines, and both entry points reject null arguments before any device call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import surely_rt as rt

REPO = Path(__file__).resolve().parent.parent


def _header_defines():
    text = (REPO / "include" / "rt_mi355x.h").read_text()
    return {k: int(v) for k, v in re.findall(r"^#define (RT_AOV_\w+) (\d+)\s*$", text, re.M)}


def test_python_constants_mirror_the_header():
    d = _header_defines()
    assert set(d) == {"RT_AOV_CHANNELS", "RT_AOV_HITS", "RT_AOV_T", "RT_AOV_NORMAL",
                      "RT_AOV_ALBEDO", "RT_AOV_EMISSION", "RT_AOV_MATID"}
    assert rt.AOV_CHANNELS == d["RT_AOV_CHANNELS"] == 12
    assert rt.AOV_HITS == d["RT_AOV_HITS"]
    assert rt.AOV_T == d["RT_AOV_T"]
    assert rt.AOV_NORMAL == d["RT_AOV_NORMAL"]
    assert rt.AOV_ALBEDO == d["RT_AOV_ALBEDO"]
    assert rt.AOV_EMISSION == d["RT_AOV_EMISSION"]
    assert rt.AOV_MATID == d["RT_AOV_MATID"]


def test_channel_names_and_planes():
    assert len(rt.AOV_NAMES) == 12 == rt.AOV_CHANNELS
    assert len(set(rt.AOV_NAMES)) == 12
    assert rt.AOV_NAMES[rt.AOV_HITS] == "hits" and rt.AOV_NAMES[rt.AOV_T] == "t"
    assert rt.AOV_NAMES[rt.AOV_NORMAL:rt.AOV_NORMAL + 3] == ("nx", "ny", "nz")
    assert rt.AOV_NAMES[rt.AOV_ALBEDO] == "albedo_r" and rt.AOV_NAMES[rt.AOV_EMISSION + 2] == "emission_b"
    assert rt.AOV_NAMES[rt.AOV_MATID] == "matid"
    a = np.arange(2 * 3 * 12, dtype=np.float32).reshape(2, 3, 12)
    p = rt.aov_planes(a)
    assert sorted(p) == ["albedo", "emission", "hits", "matid", "normal", "t"]
    assert p["hits"].shape == (2, 3) and p["normal"].shape == (2, 3, 3)
    assert p["albedo"][1, 2, 0] == a[1, 2, 5] and p["emission"][0, 1, 2] == a[0, 1, 10]
    assert p["matid"][1, 0] == a[1, 0, 11] and p["t"][0, 0] == a[0, 0, 1]
    assert np.shares_memory(p["normal"], a)  # views


def test_null_arguments_are_rejected_without_a_device():
    lib = rt.device_lib()
    _, cam = rt.preset_blob("cornell_box", width=8, spp=1)
    opts = rt.make_opts(cam)
    buf = np.zeros((cam.image_height, 8, rt.AOV_CHANNELS), np.float32)
    fake = C.c_void_p(16)  # a non-null scene handle that must never be dereferenced
    cases = [(None, C.byref(cam), C.byref(opts), buf.ctypes.data),
             (fake, None, C.byref(opts), buf.ctypes.data),
             (fake, C.byref(cam), None, buf.ctypes.data),
             (fake, C.byref(cam), C.byref(opts), None)]
    for sc, c, o, b in cases:
        assert lib.rt_render_aov(sc, c, o, b, None) == rt.RT_ERR_INVALID_ARG
        assert b"null" in lib.rt_last_error()
        assert lib.rt_render_aov_device(sc, c, o, b, None, None) == rt.RT_ERR_INVALID_ARG
    assert not buf.any()
