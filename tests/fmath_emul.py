"""Step-by-step f64 emulators of the device's polynomial transcendentals (rt_kernel.h sincos2pi,
log_u01), shared by the host test (tests/test_device_math.py) and the device test
(tests/test_device_primitives_gpu.py). TEST INFRASTRUCTURE ONLY.

The coefficients are read from the kernel source. The device build has contraction off, so every
step of the kernel is an explicit fma, product, sum or floor, each rounded once; the emulators
perform the same steps in the same order (a Python float operation is one IEEE f64 operation; an
fma is formed exactly in rational arithmetic and rounded once)."""
import math
import re
from fractions import Fraction
from pathlib import Path

import mpmath as mp

SRC = (Path(__file__).resolve().parent.parent / "surely-raytracing_amd" / "csrc" /
       "rt_kernel.h").read_text()


def fn_body(name):
    i = SRC.index(f"void {name}(" if name == "sincos2pi" else f"double {name}(")
    return SRC[i:SRC.index("\n}\n", i)]


def hexes(body, var):
    """The Horner coefficients of `var`, outermost first: the initial literal, then the fma_k
    constants in order."""
    first = re.search(rf"double {var} = (-?0x[0-9a-fp.+-]+);", body).group(1)
    rest = re.findall(rf"{var} = fma_k<__builtin_bit_cast\(uint64_t, \(?(?:double\)\()?"
                      rf"(-?0x[0-9a-fp.+-]+)\)?\)?>\({var}, \w+\);", body)
    return [float.fromhex(first)] + [float.fromhex(h) for h in rest]


def fma(a, b, c):
    """a * b + c rounded once (finite operands)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


_SINCOS = None


def sincos_coefficients():
    global _SINCOS
    if _SINCOS is None:
        body = fn_body("sincos2pi")
        _SINCOS = (hexes(body, "s"), hexes(body, "c"))
    return _SINCOS


def sincos2pi_core(u):
    """The reduction and the two polynomials: (k, th, s, c) with s ~ sin(th), c ~ cos(th),
    th = (4u - k) pi/2 the rounded quarter-turn angle."""
    S, C = sincos_coefficients()
    t = 4.0 * u
    k = math.floor(t + 0.5)
    th = (t - k) * (0.5 * math.pi)
    x2 = th * th
    s = S[0]
    for c in S[1:]:
        s = fma(s, x2, c)
    s = fma(th * x2, s, th)
    c = C[0]
    for cc in C[1:]:
        c = fma(c, x2, cc)
    c = fma(fma(c, x2, -0.5), x2, 1.0)
    return k, th, s, c


def sincos2pi(u):
    """(sin, cos) as the kernel returns them: the quadrant's selection and sign-bit flips."""
    k, _, s, c = sincos2pi_core(u)
    q = int(k) & 3
    sw = (q & 1) != 0
    so, co = (c, s) if sw else (s, c)
    if q & 2:
        so = -so
    if (q + 1) & 2:
        co = -co
    return so, co


_LOG = None


def log_coefficients():
    """(R, ln2_lo, ln2_hi)"""
    global _LOG
    if _LOG is None:
        body = fn_body("log_u01")
        lo = float.fromhex(re.search(r"dk \* (0x[0-9a-fp.+-]+)\);  // ln2_lo", body).group(1))
        hi = float.fromhex(re.search(r"dk \* (0x[0-9a-fp.+-]+) - ", body).group(1))
        _LOG = (hexes(body, "r"), lo, hi)
    return _LOG


def log_u01(x):
    """log of a draw x > 0; div_nr is taken as the correctly rounded quotient (the device's is
    within an ulp of it, so this emulator is not bit-exact)."""
    R, ln2_lo, ln2_hi = log_coefficients()
    m, e = math.frexp(x)
    if m < 0.7071067811865476:
        m, e = m * 2.0, e - 1
    f = m - 1.0
    hfsq = 0.5 * f * f
    s = float(Fraction(f) / Fraction(2.0 + f))
    z = s * s
    r = R[0]
    for c in R[1:]:
        r = fma(r, z, c)
    dk = float(e)
    t = fma(s, hfsq + r * z, dk * ln2_lo)
    return dk * ln2_hi - ((hfsq - t) - f)


def sincos_boundary_ks():
    """k of the draws u = k 2^-32 around every quarter and eighth turn, plus the ends."""
    ks = {0, 1, 2 ** 32 - 1}
    for q in range(4):
        for d in range(-2, 3):
            ks.add(q * 2 ** 30 + d)
            ks.add(q * 2 ** 30 + 2 ** 29 + d)
    return sorted(k for k in ks if 0 <= k < 2 ** 32)


def sincos_abs_errors(us, got):
    """Worst |sin - sin(2 pi u)| and |cos - cos(2 pi u)| in units of 2^-53 (half an ulp of values
    in [1/2, 1)) of `got` = [(sin, cos)] and of the reference's own expression, sin(2 pi u) and
    cos(2 pi u) in f64 libm (vec3.rs:244), against the exact values: (dev_s, dev_c, libm_s, libm_c).
    Relative ulps mean nothing where the exact value is near 0, so the error is absolute."""
    w = [mp.mpf(0)] * 4
    with mp.workprec(200):
        return _sincos_abs_errors(us, got, w)


def _sincos_abs_errors(us, got, w):
    for u, (s, c) in zip(us, got):
        x = 2 * mp.pi * mp.mpf(u)
        es, ec = mp.sin(x), mp.cos(x)
        phi = 2. * math.pi * u
        for n, (v, e) in enumerate([(s, es), (c, ec), (math.sin(phi), es), (math.cos(phi), ec)]):
            w[n] = max(w[n], abs(mp.mpf(v) - e))
    return tuple(float(x * mp.mpf(2) ** 53) for x in w)
