"""The split stream key of rt_rng.h (rng_key_pixel / rng_key_sample / rng_key_next / rng_key_mix)
gives the state of rng_seed for every (seed, pixel, sample): the stand-alone host program
build/rng_key_check (csrc/host/rng_key_check.cpp, built by the Makefile) compares them over more
than 1e6 triples, with runs of consecutive samples across the 32-bit wrap-around and the keys that
hash to the all-zero state rng_seed replaces."""
import re
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_split_stream_key_equals_rng_seed():
    exe = REPO / "build" / "rng_key_check"
    assert exe.exists(), "build/rng_key_check is missing: run make (or __graft_entry__.build())"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"rng_key_check ok: (\d+) triples", out.stdout)
    assert m and int(m.group(1)) >= 1_000_000, out.stdout
