"""Host-only: the device probes (csrc/probe/rt_probe.hip and rt_probe_scene.hip,
build/librtprobe.so) build, load without a GPU and export every function tests/probe_lib.py
binds; the wrapper's record sizes are the ones the kernels index with (a mismatch would read or
write past a buffer); the scene probe refuses on the host what its kernels must never see."""
import ctypes as C
import re
import subprocess

import probe_lib as P

import numpy as np
import pytest

import surely_rt as rt

SRC = (P.REPO / "surely-raytracing_amd" / "csrc" / "probe" / "rt_probe.hip").read_text()
SCENE_SRC = (P.REPO / "surely-raytracing_amd" / "csrc" / "probe" / "rt_probe_scene.hip").read_text()


def test_probe_library_builds_loads_and_exports_every_bound_symbol():
    subprocess.run(["make", "-C", str(P.REPO), "probe"], check=True)
    assert P.PROBE_SO.exists()
    lib = P.lib()
    raw = C.CDLL(str(P.PROBE_SO))
    assert len(P.PROBES) >= 32 and len(P.SCENE_PROBES) >= 5
    assert len(P.symbols()) == len(P.PROBES) + len(P.SCENE_PROBES) + 1
    for sym in P.symbols():
        assert getattr(raw, sym) is not None and getattr(lib, sym).restype is C.c_int, sym


def test_wrapper_record_sizes_are_the_kernels():
    decl = {n: (int(i), int(o)) for n, i, o in re.findall(r"^PROBE(?:_DECL)?\((\w+), (\d+), (\d+)\)", SRC, re.M)}
    assert decl == P.PROBES
    decl = {n: (int(i), int(o)) for n, i, o in re.findall(r"^SCENE_PROBE\((\w+), (\d+), (\d+)\)", SCENE_SRC, re.M)}
    assert decl == P.SCENE_PROBES
    # ... and each is tied to its kernel's own IN / OUT by a static_assert, and has its entry point
    assert "static_assert(K_##name::IN == NIN && K_##name::OUT == NOUT" in SCENE_SRC
    for name in P.SCENE_PROBES:
        assert re.search(rf"^RTP_API int rtp_{name}\(const rt_scene_blob\* blob,", SCENE_SRC, re.M), name


def test_probe_is_part_of_all_and_of_no_product_rule():
    """`make all` (the driver's build) builds the probe from the product's own header; no rule of
    the product libraries names it."""
    mk = (P.REPO / "Makefile").read_text()
    assert "probe" in re.search(r"^all: (.*)$", mk, re.M).group(1).split()
    rule = re.search(r"^\$\(BUILD\)/librtprobe\.so: (.*)\n\t.*\n\t(.*)$", mk, re.M)
    assert "$(HIPFLAGS)" in rule.group(2) and "-D" not in rule.group(2)  # the product's flags
    named = [ln for ln in mk.splitlines() if "rtprobe" in ln or "rt_probe" in ln]
    assert all(ln.startswith(("#", "probe:", "$(BUILD)/librtprobe.so:")) for ln in named), named
    assert '#include "../rt_kernel.h"' in SRC and '#include "../rt_kernel.h"' in SCENE_SRC
    # both probe files, the product's flattener and nothing else of the product
    srcs = [d for d in rule.group(1).split() if d.endswith((".hip", ".cpp"))]
    assert srcs == ["$(CSRC)/probe/rt_probe.hip", "$(CSRC)/probe/rt_probe_scene.hip",
                    "$(CSRC)/rt_flatten.cpp", "$(CSRC)/rt_obvh.cpp"], srcs
    assert "$(filter %.hip %.cpp,$^)" in rule.group(2)


def _blob(bvh=False, nested=False):
    sc = rt.Scene(3)
    m = sc.lambertian((0.5, 0.5, 0.5))
    objs = [sc.sphere((0, 0, 0), 1.0, m), sc.quad((3, -1, -1), (0, 2, 0), (0, 0, 2), m),
            sc.translate(sc.rotate_y(sc.sphere((0, 0, 0), 0.5, m), 30.0), (0, 3, 0)),
            sc.constant_medium(sc.sphere((5, 0, 0), 1.0, m), 0.5, (1, 1, 1))]
    if nested:
        inner = sc.constant_medium(sc.sphere((9, 0, 0), 1.0, m), 0.5, (1, 1, 1))
        objs.append(sc.constant_medium(sc.hittable_list(inner), 0.5, (1, 1, 1)))
    world = sc.hittable_list(*objs)
    if bvh:
        world = sc.hittable_list(sc.create_bvh(world))
    return sc.serialize(world, None)


def test_scene_records_and_host_refusals():
    """No GPU: the record list of a small scene, and every refusal, which is decided on the host
    before any HIP call (so it can be checked here)."""
    blob = _blob()
    recs = P.scene_records(blob)
    types = recs[:, 1].tolist()
    assert types.count(P.RTL_SPHERE) == 3 and types.count(P.RTL_QUAD) == 1
    assert types.count(P.RTL_TRANSLATE) == 1 and types.count(P.RTL_ROTATE_Y) == 1
    vol = recs[recs[:, 1] == P.RTL_VOLUME]
    assert len(vol) == 1 and vol[0, 2] & P.RTL_VOLF_SPHERE and vol[0, 4] == -1
    tr = int(recs[recs[:, 1] == P.RTL_TRANSLATE][0, 0])
    ry = recs[recs[:, 1] == P.RTL_ROTATE_Y][0]
    assert ry[4] == tr  # the rotation sits inside the translation's frame
    assert (recs[:, 0] % 4 == 0).all() and (np.diff(recs[:, 0]) > 0).all()

    def refused(fn, *a):
        with pytest.raises(P.ProbeRefused) as e:
            fn(*a)
        return e.value.code

    ray = [0.0] * 13
    assert refused(P.scene_run, "world_hit", _blob(bvh=True), ray) == P.ERR_BVH
    assert refused(P.scene_records, _blob(bvh=True)) == P.ERR_BVH
    assert refused(P.scene_run, "world_hit", _blob(nested=True), ray) == P.ERR_NESTED
    quad = int(recs[recs[:, 1] == P.RTL_QUAD][0, 0])
    for frame in (quad, tr + 4, -2, 1 << 20, 0.5):  # not a transform record
        assert refused(P.scene_run, "frame", blob, [frame] + [0.0] * 12) == P.ERR_RECORD
    for node in (quad, tr, int(vol[0, 0]) + 4, -1, 1 << 20):  # not a VOLUME record
        assert refused(P.volume_bounds, blob, node, [0.0] * 7) == P.ERR_RECORD
    for tex in (-1, 0.5, 1 << 20, blob.header()["n_textures"]):
        assert refused(P.scene_run, "tex_value", blob, [tex] + [0.0] * 5) == P.ERR_RECORD
    # one bad record among good ones refuses the whole call
    assert refused(P.scene_run, "frame", blob, [[-1.0] + [0.0] * 12, [quad] + [0.0] * 12]) == P.ERR_RECORD
