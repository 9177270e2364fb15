"""The device's polynomial transcendentals (rt_kernel.h sincos2pi, log_u01), host-only: the
coefficients are read from the kernel source and evaluated step by step in f64 with the same
fused operations (an fma is exact-product-plus-add, rounded once; tests/fmath_emul.py), then
compared with the exact values (mpmath, 200 bits). Both must stay within an ulp, like the libm
results the oracle uses (vec3.rs:244 / object.rs:127 phi = 2 pi r1; constant_medium.rs:75 log of a
draw). tests/test_device_primitives_gpu.py holds the device to the same emulator bit for bit."""
import math
import random

import mpmath as mp
import pytest

import fmath_emul as E

mp.mp.prec = 200
_fn, _hexes = E.fn_body, E.hexes


def ulps(v, exact):
    e = math.frexp(float(exact))[1]
    return float(abs(mp.mpf(v) - exact) / mp.mpf(2) ** (e - 53))


def test_sincos2pi_within_an_ulp():
    S, C = E.sincos_coefficients()
    assert len(S) == 6 and len(C) == 6
    rng = random.Random(5)
    worst = 0.0
    for i in range(1500):
        u = rng.getrandbits(32) * 2.0 ** -32  # a draw: k * 2^-32
        _, th, s, c = E.sincos2pi_core(u)
        if th != 0.0:
            worst = max(worst, ulps(s, mp.sin(mp.mpf(th))))
        worst = max(worst, ulps(c, mp.cos(mp.mpf(th))))
    assert worst < 1.0, worst


def test_sincos2pi_absolute_error_no_worse_than_the_reference_expression():
    """Against sin / cos of the exact 2 pi u (not of the rounded angle th): the whole function,
    quadrant logic included, errs no more than the reference's f64 libm expression does on the
    same draws (the rounding of 2 pi u alone costs that expression several units)."""
    rng = random.Random(5)
    us = [k * 2.0 ** -32 for k in E.sincos_boundary_ks() + [rng.getrandbits(32) for _ in range(4000)]]
    ds, dc, ls, lc = E.sincos_abs_errors(us, [E.sincos2pi(u) for u in us])
    print(f"sincos2pi emulator |err| / 2^-53: sin {ds:.3f} cos {dc:.3f}; libm expression: "
          f"sin {ls:.3f} cos {lc:.3f}")
    assert ds <= ls and dc <= lc, (ds, dc, ls, lc)


def test_log_u01_within_an_ulp_and_log0():
    body = _fn("log_u01")
    R, ln2_lo, ln2_hi = E.log_coefficients()
    assert len(R) == 7
    assert 0.0 < ln2_lo < 2.0 ** -25 and ln2_hi + ln2_lo == math.log(2.0)
    assert "x == 0.0 ? -kInf" in body  # log(0) = -inf: the reference's infinite free path

    flog = E.log_u01
    rng = random.Random(7)
    ks = [1, 2, 3, 2 ** 31, 2 ** 32 - 1, 0x5A827999] + [rng.getrandbits(32) for _ in range(1500)]
    worst = max(ulps(flog(k * 2.0 ** -32), mp.log(mp.mpf(k) * mp.mpf(2) ** -32))
                for k in ks if k)
    assert worst < 1.0, worst


@pytest.mark.parametrize("name", ["sincos2pi", "log_u01"])
def test_polynomials_use_sgpr_constant_fmas(name):
    """The Horner steps go through fma_k (v_fma_f64 with the constant in an SGPR pair), not a
    plain fma the compiler would turn into v_fmac_f64 plus two constant moves per step."""
    body = _fn(name)
    assert body.count("fma_k<") >= 5
