"""Kernel resources of the scene-specialised kernels after the f32 weight mirrors and the parked
generator state (rt_kernel.h trace_body): the cornell_box kernel and its tile-list variant, built
for gfx950 without a GPU by the benchmark's compiler, spill nothing and use no scratch at six waves
per SIMD (before: 4 spilled dwords, 20 B); cornell_smoke and final_scene stay at 0 / 0.

Reader and child process as tests/test_jit_resources.py (tools/jit_meta.py on the code object hiprtc
produced with the code-object cache off). The tile-list variant is the second translation unit
rt_scene_jit_check compiles under RT_JIT_CHECK_TILES=1, so the dump then holds that one."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
# (scene, tile-list variant): (vgpr_spill_count, private_segment_fixed_size)
PINNED = {
    ("cornell_box", False): (0, 0),
    ("cornell_box", True): (0, 0),
    ("cornell_smoke", False): (0, 0),
    ("final_scene", False): (0, 0),
}
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
out = {}
with tempfile.TemporaryDirectory() as tmp:
    for arg in sys.argv[2:]:
        name, tiles = arg.split(":")
        dump = os.path.join(tmp, arg.replace(":", "_") + ".co")
        os.environ["RT_JIT_DUMP"] = dump
        if tiles == "1":
            os.environ["RT_JIT_CHECK_TILES"] = "1"
        else:
            os.environ.pop("RT_JIT_CHECK_TILES", None)
        blob, _ = rt.preset_blob(name, width=32, spp=4)
        state, _ = rt.jit_check(blob)
        out[arg] = dict(state=state, **(jit_meta.meta(dump) if state == 1 else {}))
print("META " + json.dumps(out))
"""


def _key(scene, tiles):
    return f"{scene}:{int(tiles)}"


@pytest.fixture(scope="module")
def metas():
    out = subprocess.run([sys.executable, "-c", CHILD, str(REPO), *[_key(*k) for k in PINNED]],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("META ")]
    assert line, out.stdout[-2000:]
    return json.loads(line[-1][5:])


@pytest.mark.parametrize("scene,tiles", sorted(PINNED))
def test_spills_and_scratch_are_pinned(metas, scene, tiles):
    m = metas[_key(scene, tiles)]
    print(scene, "tile-list" if tiles else "plain", m)
    assert m["state"] == 1, "the scene-specialised kernel was not generated or did not compile"
    spills, scratch = PINNED[(scene, tiles)]
    assert spills <= 2 and scratch <= 12  # never above what the mirrors alone reach
    assert m["vgpr_spill_count"] == spills, m
    assert m["private_segment_fixed_size"] == scratch, m
    assert m.get("agpr_count", 0) == 0, m
    if scene == "cornell_box":  # six waves per SIMD: 512 / 6 registers, in allocation granules of 8
        assert m["vgpr_count"] <= 80, m
