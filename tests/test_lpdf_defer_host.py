"""The deferred light-list PDF on the host (rt_jit.cpp kLpdfDefer): which scenes the generator lets
the path kernel defer (every light entry a leaf whose constants are also a world-frame record of
the unrolled walk), that each of them compiles for gfx950, and that the cornell_box kernel keeps
its registers and LDS (six waves per SIMD, six workgroups per CU)."""
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest

import lpdf_scenes as S
import surely_rt as rt
import test_gpu_parity as P

REPO = Path(__file__).resolve().parent.parent


def _walker(blob):
    state, src = rt.jit_check(blob)
    assert state == 1, src
    return src


def test_cornell_box_defers_with_both_entries_matched():
    blob, _ = rt.preset_blob("cornell_box", width=32, spp=4)
    src = _walker(blob)
    assert S.defers(src)
    world = src[:src.index("void frame_in")]
    # the light quad's and the sphere's own tests hand out what the entries' weights need
    assert len(re.findall(r"aquad_test<COUNT, 1>\([^;]*, C, lt, lin\);", world)) == 1
    assert len(re.findall(r"sphere_test_v<COUNT>\([^;]*, C, la, lhb, ldisc\);", world)) == 1
    assert re.search(r"lpv0 = \(\(0\.001 <= lt\) & \(lt <= kInf\) & lin\) \? quad_light_w\(d, lt, ", world)
    assert "lpv1 = (!(ldisc < 0.0) & ((lc1 < 0.0) | (ldisc > lc1 * lc1))) ? q_sphere : (wt)0;" in world
    # HittableList::pdf_value's fold in the list's order, then 1/len, as lights_pdf's
    fold = world[world.index("lsum = lpv0;"):]
    assert fold.index("lsum = lsum + lpv1;") < fold.index("lsum = lsum * (wt)(0x1p-1);")


def test_mixed_pdf_one_quad_list_defers():
    blob, _ = rt.preset_blob("cornell_box", variant="mixed_pdf", width=32, spp=4)
    src = _walker(blob)
    assert S.defers(src) and "lpv0 = " in src and "lpv1" not in src


@pytest.mark.parametrize("depth,sphere_light", [(10, False), (10, True)])
def test_zero_pdf_scene_with_every_entry_in_the_world_defers(depth, sphere_light):
    blob, _ = S.zero_pdf_matched(depth, sphere_light)
    assert S.defers(_walker(blob))


@pytest.mark.parametrize("kind", ["checker", "volume"])
def test_matched_rooms_defer(kind):
    blob, _ = S.room(kind)
    assert S.defers(_walker(blob))


def _not_in_world():
    return P._zero_pdf_scene()[0]


@pytest.mark.parametrize("name,make", [
    ("light_not_in_world", _not_in_world),
    ("nested_light_list", S.nested_light_list),
    ("world_quad_inside_translate", lambda: S.room("translate")[0]),
    ("general_light_quad", lambda: S.room("general")[0]),
    ("moving_sphere_light", lambda: S.room("moving")[0]),
    ("two_sphere_lights", lambda: S.room("spheres2")[0]),
    ("cornell_smoke", lambda: rt.preset_blob("cornell_smoke", width=32, spp=4)[0]),
    ("final_scene", lambda: rt.preset_blob("final_scene", width=32, spp=4)[0]),
])
def test_scenes_that_keep_the_immediate_path(name, make):
    src = _walker(make())
    assert not S.defers(src)
    # today's source: no by-products, no second world signature
    assert "lpv0" not in src and "wt& lsum" not in src and "q_sphere" not in src
    assert "RT_LPDF_NOW" not in src


def test_switch_compiles(monkeypatch):
    """-DRT_LPDF_NOW (the A/B handle) forces kLpdfDefer false in the same generated source."""
    monkeypatch.setenv("RT_JIT_OPTS", "-DRT_LPDF_NOW")
    blob, _ = rt.preset_blob("cornell_box", width=32, spp=4)
    src = _walker(blob)
    assert "#ifdef RT_LPDF_NOW\n  static constexpr bool kLpdfDefer = false;" in src


CHILD = r"""
import json, os, sys, tempfile
repo = sys.argv[1]
sys.path.insert(0, os.path.join(repo, "tools"))
sys.path.insert(0, os.path.join(repo, "surely-raytracing_amd"))
os.environ["RT_JIT_CACHE"] = "0"       # compile, do not load the cached object
os.environ.pop("RT_JIT_OPTS", None)
os.environ.pop("RT_JIT_SRC_DIR", None)
import torch  # the benchmark's compiler (tools/jit_cache_fill.py)
import jit_meta
import surely_rt as rt
with tempfile.TemporaryDirectory() as tmp:
    dump = os.path.join(tmp, "cornell_box.co")
    os.environ["RT_JIT_DUMP"] = dump
    blob, _ = rt.preset_blob("cornell_box", width=32, spp=4)
    state, _ = rt.jit_check(blob)
    out = dict(state=state, **(jit_meta.meta(dump) if state == 1 else {}))
    out["stage_bytes"] = rt.lds_check(blob, n_rays=0)["stage_bytes"]
print("META " + json.dumps(out))
"""


def test_cornell_box_keeps_its_occupancy():
    """Read as test_jit_resources.py does. 80 VGPRs keep six waves per SIMD (512 / 6 = 85, in
    granules of 8); six workgroups per CU leave 27,306 B of the 160 KiB LDS to each, static plus
    the staged scene."""
    out = subprocess.run([sys.executable, "-c", CHILD, str(REPO)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("META ")]
    assert line, out.stdout[-2000:]
    m = json.loads(line[-1][5:])
    print(m)
    assert m["state"] == 1
    assert m["vgpr_count"] <= 80, m
    assert m["stage_bytes"] == 3776, m
    assert m["group_segment_fixed_size"] + m["stage_bytes"] <= 27306, m
