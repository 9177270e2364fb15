"""bench.py's command line: a plain run reports the headline only, --full adds the roofline and
the CPU baseline, --dump-outputs writes the frame of the last timed step."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps")
FULL_ONLY = ("roofline", "cpu_baseline", "speedup_vs_cpu")
TINY = ["--gpus", "1", "--width", "64", "--spp", "16", "--depth", "8"]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("rt_bench_cli", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_and_dump_outputs_are_off_by_default(bench):
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 2)
    a = bench.parse(["--full", "--dump-outputs", "d", "--no-cpu-baseline", "--no-count"])
    assert a.full and a.dump_outputs == "d" and a.no_cpu_baseline and a.no_count
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_the_frame_or_a_fixed_sample(bench, tmp_path, monkeypatch):
    import torch

    frame = torch.arange(5 * 7 * 3, dtype=torch.float32).reshape(5, 7, 3)
    bench.dump_outputs(tmp_path / "a" / "b", frame)
    got = np.load(tmp_path / "a" / "b" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame.numpy())
    # above the size limit: the same seeded sample of pixels every time, in image order
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 12)
    bench.dump_outputs(tmp_path / "s1", frame)
    bench.dump_outputs(tmp_path / "s2", frame)
    s1, s2 = np.load(tmp_path / "s1" / "frame.npy"), np.load(tmp_path / "s2" / "frame.npy")
    assert s1.shape == (10, 3) and s1.nbytes <= 10 * 12 and np.array_equal(s1, s2)
    first = s1[:, 0]
    assert np.all(np.diff(first) > 0) and np.all(first % 3 == 0)
    assert np.array_equal(s1, frame.numpy().reshape(-1, 3)[(first // 3).astype(int)])


def _line(capsys):
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return lines[0]


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_frame(bench, gpu_available, tmp_path,
                                                                 capsys):
    """A plain run: --steps timed steps, the headline fields, none of the --full blocks; the
    dumped frame is the product's render of the same scene, camera and seed, bit for bit, and
    the same from run to run."""
    import surely_rt as rt

    bench.main(TINY + ["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "r1")])
    res = _line(capsys)
    assert all(k in res for k in HEADLINE) and not any(k in res for k in FULL_ONLY)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0
    samples = 64 * 64 * res["config"]["spp_effective"]
    assert res["value"] == pytest.approx(samples / (res["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    bench.main(TINY + ["--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "r2")])
    assert _line(capsys)["steps"] == 1
    f1, f2 = np.load(tmp_path / "r1" / "frame.npy"), np.load(tmp_path / "r2" / "frame.npy")
    assert f1.dtype == np.float32 and f1.shape == (64, 64, 3) and np.array_equal(f1, f2)
    blob, cam = rt.preset_blob("cornell_box", width=64, spp=16, depth=8)
    ds = rt.DeviceScene(blob, device=0)
    ref, _ = ds.render(cam, rt.make_opts(cam, seed=1, flags=rt.RT_FLAG_OVERWRITE))
    ds.close()
    assert np.array_equal(f1, ref) and float(f1.max()) > 0.0


@pytest.mark.gpu
def test_full_run_adds_the_roofline_and_the_cpu_baseline(bench, gpu_available, capsys):
    bench.main(TINY + ["--steps", "1", "--warmup", "1", "--full", "--cpu-seconds", "0.2"])
    res = _line(capsys)
    assert all(k in res for k in HEADLINE + FULL_ONLY)
    assert res["roofline"]["kernel"] == "rt_trace" and res["roofline"]["achieved"] > 0
    assert res["cpu_baseline"]["value"] > 0
