"""Kernel resources of the scene-specialised kernels of the three benchmark scenes: they compile
for gfx950 without a GPU, and spill no more VGPRs and use no more scratch than the parent of the
turnover-gate change did.

The parent's values were read from a parent build with this same procedure (tools/jit_meta.py's
reader on the code object that the benchmark's compiler, the hiprtc PyTorch bundles, produced with
the code-object cache off): cornell_box 80 VGPRs, 4 spilled, 20 B scratch; cornell_smoke 92, 0, 0;
final_scene 162, 0, 0."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
PARENT = {  # scene: (vgpr_spill_count, private_segment_fixed_size)
    "cornell_box": (4, 20),
    "cornell_smoke": (0, 0),
    "final_scene": (0, 0),
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
    for name in sys.argv[2:]:
        dump = os.path.join(tmp, name + ".co")
        os.environ["RT_JIT_DUMP"] = dump
        blob, _ = rt.preset_blob(name, width=32, spp=4)
        state, _ = rt.jit_check(blob)
        out[name] = dict(state=state, **(jit_meta.meta(dump) if state == 1 else {}))
print("META " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def metas():
    out = subprocess.run([sys.executable, "-c", CHILD, str(REPO), *PARENT], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("META ")]
    assert line, out.stdout[-2000:]
    return json.loads(line[-1][5:])


@pytest.mark.parametrize("scene", sorted(PARENT))
def test_spills_and_scratch_do_not_exceed_the_parents(metas, scene):
    m = metas[scene]
    print(scene, m)
    assert m["state"] == 1, "the scene-specialised kernel was not generated or did not compile"
    spills, scratch = PARENT[scene]
    assert m["vgpr_spill_count"] <= spills, m
    assert m["private_segment_fixed_size"] <= scratch, m
    assert m.get("agpr_count", 0) == 0, m
