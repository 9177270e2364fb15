"""Host-only: the device-primitive probe (csrc/probe/rt_probe.hip, build/librtprobe.so) builds,
loads without a GPU and exports every function tests/probe_lib.py binds; the wrapper's record
sizes are the ones the kernels index with (a mismatch would read or write past a buffer)."""
import ctypes as C
import re
import subprocess

import probe_lib as P

SRC = (P.REPO / "surely-raytracing_amd" / "csrc" / "probe" / "rt_probe.hip").read_text()


def test_probe_library_builds_loads_and_exports_every_bound_symbol():
    subprocess.run(["make", "-C", str(P.REPO), "probe"], check=True)
    assert P.PROBE_SO.exists()
    lib = P.lib()
    raw = C.CDLL(str(P.PROBE_SO))
    assert len(P.symbols()) == len(P.PROBES) >= 30
    for sym in P.symbols():
        assert getattr(raw, sym) is not None and getattr(lib, sym).restype is C.c_int, sym


def test_wrapper_record_sizes_are_the_kernels():
    decl = {n: (int(i), int(o)) for n, i, o in re.findall(r"^PROBE(?:_DECL)?\((\w+), (\d+), (\d+)\)", SRC, re.M)}
    assert decl == P.PROBES


def test_probe_is_part_of_all_and_of_no_product_rule():
    """`make all` (the driver's build) builds the probe from the product's own header; no rule of
    the product libraries names it."""
    mk = (P.REPO / "Makefile").read_text()
    assert "probe" in re.search(r"^all: (.*)$", mk, re.M).group(1).split()
    rule = re.search(r"^\$\(BUILD\)/librtprobe\.so: (.*)\n\t.*\n\t(.*)$", mk, re.M)
    assert "$(HIPFLAGS)" in rule.group(2) and "-D" not in rule.group(2)  # the product's flags
    named = [ln for ln in mk.splitlines() if "rtprobe" in ln or "rt_probe" in ln]
    assert all(ln.startswith(("#", "probe:", "$(BUILD)/librtprobe.so:")) for ln in named), named
    assert '#include "../rt_kernel.h"' in SRC
