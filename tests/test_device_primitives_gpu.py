"""The device's math and hit-test primitives (rt_kernel.h, rt_rng.h), one by one on the GPU.

Every other GPU test goes through a whole render; these run each small inline function by itself
through the probe library (csrc/probe/rt_probe.hip, tests/probe_lib.py: kernels that call the
product's functions and nothing else) and compare it with a high-precision reference: exact
rational arithmetic (fractions), mpmath at 200 bits, the f64 oracle's hooks, or plain Python /
numpy f64 in the reference's operation order.

Bounds
  * Where the header promises "within an ulp" the result may be at most one ulp from the
    correctly rounded exact value; promised special values and decisions are exact.
  * The vector-operation rule, where the project promises no ulp bound: over the input set the
    device's worst error against the exact result may be at most twice the worst error of the
    reference's own f64 evaluation (the oracle hook where one exists, else Python floats in the
    reference's operation order). The two differ only by fused versus unfused rounding and by
    reciprocals / roots within an ulp instead of correctly rounded; each can at most double one
    operation's rounding error. Vector errors are norm-wise: max_i |got_i - exact_i| / max_i
    |exact_i|. Every such test prints both numbers.
  * Guard band of the random hit tests: rays whose exact roots, discriminant, plane quotient or
    planar coordinates lie within a relative 1e-9 of a decision boundary are left out (at most
    1 % of a set); on the rest the f64 oracle and the device must both take the exact decision.
  * f32 weights (perlin_turb, quad_light_w, sphere_light_w): twice the worst error of a plain
    numpy float32 restatement of the reference formulas on the same inputs.

Measured on an MI355X (the same table stands in DESIGN.md §2):
  distance from the correctly rounded value, ulp: rcp_nr 0, rcp_w 0, div_nr 0, sqrt_nr 0,
    rsq_nr 1, rcp_wt 1 (f32), rsq_wt 1 (f32); pow5_cr equal bit for bit; log_u01 0.718 ulp
  sincos2pi: equal to the emulator bit for bit; |err| / 2^-53 against sin / cos(2 pi u)
    1.087 / 1.136, the f64 libm expression 6.160 / 5.635
  device worst / reference worst (vector-operation rule, bound: a factor 2)
    random_cosine_direction 2.31e-16 / 6.95e-16    random_unit_vector 2.73e-16 / 2.21e-16
    sphere_test_v t         8.53e-13 / 9.96e-13    quad_test t        2.57e-15 / 2.39e-15
    aquad_test<0,1,2> t     1.72e-16, 2.12e-16, 1.85e-16: the oracle's values exactly, with
                            r = rcp_nr(d) and with r = rcp_nr1(d), which is what the callers pass
    rotate_y_in             1.57e-16 / 1.88e-16    rotate_y_out       1.81e-16 / 1.68e-16
    reflect                 3.59e-16 / 4.92e-16    refract            3.94e-16 / 6.04e-16
    refract, critical angle 1.44e-08 / 1.44e-08    unit_vector        3.01e-16 / 2.56e-16
    onb_local               3.24e-16 / 3.57e-16    sphere_uv_f        1.89e-16 / 1.82e-16
  device worst / float32 restatement worst (bound: a factor 2)
    perlin_turb, the oracle test's points 1.18e-07 / 5.40e-05, lattice edges 8.61e-08 / 6.73e-08
    quad_light_w 4.71e-07 / 4.58e-07    sphere_light_w 1.59e-07 / 1.76e-06, near 1: 4.03e-08
  guard band: 0.00 % of the rays left out in every set (sphere 2048, quads 1024 / 2048)."""
import math
import re
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np
import pytest

import fmath_emul as E
import oracle_lib as O
import probe_lib as P
import surely_rt as rt

pytestmark = pytest.mark.gpu

mp.mp.prec = 200
M = mp.mpf
INF = math.inf
NAN = math.nan
SENT = -7.25  # t_out's sentinel: a miss must leave it alone


# ---------------------------------------------------------------- helpers
def _ord(x):
    """Monotone integer image of f64 values: adjacent doubles differ by 1 (+0 and -0 coincide)."""
    b = np.ascontiguousarray(x, np.float64).view(np.int64)
    return np.where(b < 0, -(b & np.int64(0x7FFFFFFFFFFFFFFF)), b)


def _ord32(x):
    b = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _ord1(x):
    return int(_ord([x])[0])


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _rn(x, bits=53):
    """An mpmath value rounded to nearest-even at `bits` significant bits, as a float."""
    with mp.workprec(bits):
        return float(+x)


def _ulps(v, exact):
    """|v - exact| in ulps of exact's binade."""
    e = math.frexp(float(exact))[1]
    return float(abs(M(v) - exact) / M(2) ** (e - 53))


def _vec_err(got, exact):
    """Worst norm-wise relative error of the rows of `got` against the exact rows."""
    w = M(0)
    for g, ex in zip(np.asarray(got, np.float64).reshape(len(exact), -1).tolist(), exact):
        scale = max(abs(M(e)) for e in ex)
        err = max(abs(M(gi) - M(ei)) for gi, ei in zip(g, ex))
        if scale == 0:
            assert err == 0
            continue
        w = max(w, err / scale)
    return float(w)


def _rule(name, dev, ref, factor=2.0):
    print(f"{name}: device worst {dev:.3e}, reference worst {ref:.3e}")
    assert dev <= factor * ref, (name, dev, ref)


def _within_one_ulp(name, got, want, ordf=_ord):
    d = np.abs(ordf(got) - ordf(want))
    print(f"{name}: {len(d)} inputs, worst distance from the correctly rounded value {d.max()} ulp")
    assert np.isfinite(got).all() and d.max() <= 1, (name, int(d.argmax()), d.max())


def _scaled(rng, both_signs, emax=200, f32=False):
    """m 2^e for e in [-emax, emax], m in {1, 2 - ulp, seeded random}."""
    e = np.arange(-emax, emax + 1)
    n = len(e)
    if f32:
        ms = [np.ones(n), np.full(n, 2.0 - 2.0 ** -23),
              (1.0 + rng.random(n)).astype(np.float32).astype(np.float64)]
    else:
        ms = [np.ones(n), np.full(n, 2.0 - 2.0 ** -52), 1.0 + rng.random(n)]
    x = np.concatenate([np.ldexp(np.minimum(m, 2.0 - 2.0 ** -23) if f32 else m, e) for m in ms])
    return np.concatenate([x, -x]) if both_signs else x


def _fr(v):
    return [Fr(x) for x in v]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _near(x, b, rel=1e-9):
    """The exact value x (a Fraction or an mpf) within a relative `rel` of the boundary b."""
    if math.isinf(b):
        return False
    if isinstance(x, Fr):
        return abs(x - Fr(b)) <= Fr(rel) * max(abs(x), abs(Fr(b)))
    return abs(x - M(b)) <= rel * max(abs(x), abs(M(b)))


# ---------------------------------------------------------------- reciprocals and roots
def test_rcp_div_rsq_sqrt_within_an_ulp(gpu_available):
    rng = np.random.default_rng(101)
    x = _scaled(rng, True)
    for name in ("rcp_nr", "rcp_w"):
        got = P.run(name, x)[:, 0]
        _within_one_ulp(name, got, np.array([float(1 / Fr(v)) for v in x.tolist()]))
    a = rng.permutation(_scaled(rng, True))
    got = P.run("div_nr", np.stack([a, x], 1))[:, 0]
    _within_one_ulp("div_nr", got, np.array([float(Fr(p) / Fr(q)) for p, q in zip(a.tolist(), x.tolist())]))
    xp = _scaled(rng, False)
    got = P.run("rsq_nr", xp)[:, 0]
    _within_one_ulp("rsq_nr", got, np.array([_rn(1 / mp.sqrt(M(v))) for v in xp.tolist()]))
    k = rng.integers(1, 2 ** 32, 512).astype(np.float64)
    draws = np.concatenate([k * 2.0 ** -32, 1.0 - k * 2.0 ** -32, [2.0 ** -32, 1.0 - 2.0 ** -32]])
    j = rng.integers(1, 2 ** 26, 256).astype(np.float64)
    squares = np.ldexp(j * j, 2 * rng.integers(-60, 60, 256))
    xs = np.concatenate([xp, draws, squares])
    got = P.run("sqrt_nr", xs)[:, 0]
    _within_one_ulp("sqrt_nr", got, np.array([_rn(mp.sqrt(M(v))) for v in xs.tolist()]))


def test_rcp_wt_rsq_wt_within_an_f32_ulp(gpu_available):
    rng = np.random.default_rng(102)
    x = _scaled(rng, True, emax=120, f32=True)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    got = P.run("rcp_wt", x)[:, 0]
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
    _within_one_ulp("rcp_wt", got, np.array([_rn(1 / M(v), 24) for v in x.tolist()]), _ord32)
    xp = _scaled(rng, False, emax=120, f32=True)
    got = P.run("rsq_wt", xp)[:, 0]
    _within_one_ulp("rsq_wt", got, np.array([_rn(1 / mp.sqrt(M(v)), 24) for v in xp.tolist()]), _ord32)


def test_reciprocal_and_root_special_values(gpu_available):
    sp = np.array([0.0, -0.0, INF, -INF, NAN])
    for name in ("rcp_w", "rcp_wt"):
        g = P.run(name, sp)[:, 0]
        assert g[0] == INF and g[1] == -INF, (name, g)
        assert g[2] == 0.0 and not np.signbit(g[2]) and g[3] == 0.0 and np.signbit(g[3]), (name, g)
        assert np.isnan(g[4]), (name, g)
    g = P.run("sqrt_nr", np.array([0.0, -0.0, INF, -1.0, -2.0 ** -40, -2.0 ** 90, -INF, NAN]))[:, 0]
    assert g[0] == 0.0 and not np.signbit(g[0]) and g[1] == 0.0 and np.signbit(g[1]), g
    assert g[2] == INF and np.isnan(g[3:]).all(), g


# ---------------------------------------------------------------- sincos2pi, log_u01, pow5_cr
def test_sincos2pi_is_the_emulator_bit_for_bit_and_no_worse_than_libm(gpu_available):
    rng = np.random.default_rng(103)
    ks = E.sincos_boundary_ks() + rng.integers(0, 2 ** 32, 4096).tolist()
    us = [k * 2.0 ** -32 for k in ks]
    got = P.run("sincos2pi", us)
    emu = np.array([E.sincos2pi(u) for u in us])
    diff = np.nonzero((_bits(got) != _bits(emu)).any(axis=1))[0]
    assert len(diff) == 0, [(ks[i], got[i].tolist(), emu[i].tolist()) for i in diff[:5]]
    # quarter turns: exactly 0 and +-1 (the sign of a zero is free)
    q = P.run("sincos2pi", [0.0, 0.25, 0.5, 0.75])
    assert np.array_equal(np.abs(q), np.abs(np.array([[0., 1.], [1., 0.], [0., -1.], [-1., 0.]])))
    assert q[0, 1] == 1 and q[1, 0] == 1 and q[2, 1] == -1 and q[3, 0] == -1
    ds, dc, ls, lc = E.sincos_abs_errors(us, got.tolist())
    print(f"sincos2pi |err| / 2^-53 against sin/cos(2 pi u): device sin {ds:.3f} cos {dc:.3f}; "
          f"f64 libm expression sin {ls:.3f} cos {lc:.3f}")
    assert ds <= ls and dc <= lc, (ds, dc, ls, lc)


def test_log_u01_within_an_ulp_and_log0(gpu_available):
    rng = np.random.default_rng(104)
    ks = {1, 2, 3, 2 ** 31, 2 ** 32 - 1, 0x5A827999}
    for j in range(32):
        ks |= {2 ** j - 1, 2 ** j, 2 ** j + 1}
    sw = int(M(2) ** 32 / mp.sqrt(2))  # floor(2^32 / sqrt 2): the `low` branch switches here
    ks |= {sw + d for d in range(-2, 3)}
    ks = sorted(k for k in ks if 0 < k < 2 ** 32) + rng.integers(1, 2 ** 32, 4096).tolist()
    got = P.run("log_u01", [k * 2.0 ** -32 for k in ks])[:, 0]
    errs = [_ulps(g, mp.log(M(k) * M(2) ** -32)) for k, g in zip(ks, got.tolist())]
    w = int(np.argmax(errs))
    print(f"log_u01: {len(ks)} draws, worst error {errs[w]:.3f} ulp at k = {ks[w]}")
    assert errs[w] <= 1.0, (ks[w], errs[w])
    z = P.run("log_u01", [0.0])[0, 0]
    assert z == -INF


def test_pow5_cr_is_correctly_rounded(gpu_available):
    rng = np.random.default_rng(105)
    x = np.concatenate([[0.0, 1.0], 2.0 ** -np.arange(1, 41), rng.random(4096)])
    got = P.run("pow5_cr", x)[:, 0]
    want = np.array([float(Fr(v) ** 5) for v in x.tolist()])
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:5]]


def test_f2i_sat_f2u_sat_are_rusts_as(gpu_available):
    imin, imax, umax = -2.0 ** 31, 2.0 ** 31 - 1, 2.0 ** 32 - 1
    ti = [(NAN, 0), (INF, imax), (-INF, imin), (1e10, imax), (-1e10, imin), (2.0 ** 31, imax),
          (-2.0 ** 31 - 0.5, imin), (-2.0 ** 31, imin), (2147483647.5, 2147483647), (0.999, 0),
          (-0.999, 0), (0.0, 0), (-0.0, 0), (5.9, 5), (-5.9, -5), (-2147483647.5, -2147483647)]
    tu = [(NAN, 0), (INF, umax), (-INF, 0), (1e10, umax), (-1e10, 0), (2.0 ** 32, umax),
          (4294967295.5, 4294967295), (-0.999, 0), (0.999, 0), (-1.0, 0), (-2.0 ** 31, 0),
          (-1e-300, 0), (2.0 ** 31, 2.0 ** 31), (5.9, 5), (0.0, 0), (-0.0, 0)]
    gi = P.run("f2i_sat", [a for a, _ in ti])[:, 0]
    gu = P.run("f2u_sat", [a for a, _ in tu])[:, 0]
    assert gi.tolist() == [float(b) for _, b in ti], list(zip(ti, gi.tolist()))
    assert gu.tolist() == [float(b) for _, b in tu], list(zip(tu, gu.tolist()))


# ---------------------------------------------------------------- RNG
_M32 = 0xFFFFFFFF


def _rng_py(seed, pixel, sample, n):
    """rt_rng.h in Python integers: (first n outputs, state after them, seeded state)."""
    lo, hi = seed & _M32, (seed >> 32) & _M32
    k0 = (((lo ^ 0x85EBCA6B) * 0x9E3779B9) + 1013904223) & _M32
    k1 = (((hi ^ 0xC2B2AE35) * 0x9E3779B9) + (k0 ^ 0x27D4EB2F)) & _M32
    v0, v1 = (pixel * 1664525 + k0) & _M32, (sample * 1664525 + k1) & _M32
    for _ in range(2):
        v0 = (v0 + v1 * 1664525) & _M32
        v1 = (v1 + v0 * 1664525) & _M32
        v0 ^= v0 >> 16
        v1 ^= v1 >> 16
    if v0 | v1 == 0:
        v0 = 0x9E3779B9
    first = (v0, v1)
    rotl = lambda x, k: ((x << k) | (x >> (32 - k))) & _M32  # noqa: E731
    out = []
    for _ in range(n):
        out.append((v0 * 0x9E3779BB) & _M32)
        s1 = v1 ^ v0
        v0, v1 = rotl(v0, 26) ^ s1 ^ ((s1 << 9) & _M32), rotl(s1, 13)
    return out, (v0, v1), first


def _keys64():
    seeds = [1, 0xFFFFFFFF00000001, (5 << 32) | 3, 0x8000000080000000]
    pixels = [0, 2 ** 32 - 1, 123, 2 ** 31 + 7]
    samples = [0, 2 ** 30, 45, 2 ** 32 - 1]
    return [(s, p, m) for s in seeds for p in pixels for m in samples]


def _key_rec(seed, pixel, sample):
    return [float(seed & _M32), float(seed >> 32), float(pixel), float(sample)]


def test_rng_stream_and_split_key(gpu_available):
    keys = _keys64()
    got = P.run("rng_stream", [_key_rec(*k) for k in keys])
    for (seed, pixel, sample), g in zip(keys, got):
        want = O.rng_u32(seed, pixel, sample, 16).astype(np.float64)
        assert np.array_equal(g[6:], want), (seed, pixel, sample)
        py, _, first = _rng_py(seed, pixel, sample, 16)
        assert want.tolist() == [float(v) for v in py]  # the restatement the later tests step
        assert g[0:2].tolist() == [float(first[0]), float(first[1])]
        assert np.array_equal(g[2:4], g[0:2]), "rng_key_mix(rng_key_pixel, rng_key_sample)"
        assert np.array_equal(g[4:6], g[0:2]), "rng_key_next"


def test_rnd_rnd_pm1_rnd_index_are_the_exact_integer_formulas(gpu_available):
    recs, want = [], []
    for seed, pixel, sample in _keys64():
        u = [int(v) for v in O.rng_u32(seed, pixel, sample, 3)]
        for n in (1, 2, 3, 7, 2 ** 31, 2 ** 32 - 1):
            recs.append(_key_rec(seed, pixel, sample) + [float(n)])
            want.append([u[0] * 2.0 ** -32, float(Fr(u[1], 2 ** 31) - 1), float((u[2] * n) >> 32)])
    got = P.run("rng_draws", recs)
    assert np.array_equal(got, np.array(want))
    assert (got[:, 0] >= 0).all() and (got[:, 0] < 1).all() and (got[:, 1] >= -1).all()
    assert (got[:, 1] < 1).all()


def _sample_keys(n, seed):
    return [(seed, 977 * k + 5, 3 * k + 1) for k in range(n)]


def test_random_cosine_direction(gpu_available):
    keys = _sample_keys(2048, 0xA5A5A5A500000011)
    got = P.run("random_cosine_direction", [_key_rec(*k) for k in keys])
    exact, ref = [], []
    for (seed, pixel, sample), g in zip(keys, got):
        r1, r2 = O.rng_draws(seed, pixel, sample, 2).tolist()
        _, state, _ = _rng_py(seed, pixel, sample, 2)
        assert g[3:5].tolist() == [float(state[0]), float(state[1])]  # two draws consumed
        ph = 2 * mp.pi * M(r1)
        exact.append((mp.cos(ph) * mp.sqrt(M(r2)), mp.sin(ph) * mp.sqrt(M(r2)), mp.sqrt(1 - M(r2))))
        phi = 2. * math.pi * r1  # vec3.rs:240-250
        ref.append((math.cos(phi) * math.sqrt(r2), math.sin(phi) * math.sqrt(r2), math.sqrt(1. - r2)))
    _rule("random_cosine_direction", _vec_err(got[:, :3], exact), _vec_err(ref, exact))


def test_random_unit_vector(gpu_available):
    keys = _sample_keys(2048, 0x0123456789ABCDEF)
    got = P.run("random_unit_vector", [_key_rec(*k) for k in keys])
    exact, ref, loops = [], [], 0
    for (seed, pixel, sample), g in zip(keys, got):
        d = O.rng_draws(seed, pixel, sample, 96).tolist()
        n = 0
        while True:  # vec3.rs:231-238 on the same draws
            x, y, z = (-1. + 2. * d[n + c] for c in range(3))  # utils.rs:9-11
            n += 3
            if x * x + y * y + z * z < 1.:
                break
        loops += n // 3 - 1
        _, state, _ = _rng_py(seed, pixel, sample, n)
        assert g[3:5].tolist() == [float(state[0]), float(state[1])], (seed, pixel, sample, n)
        ln = mp.sqrt(M(x) ** 2 + M(y) ** 2 + M(z) ** 2)
        exact.append((M(x) / ln, M(y) / ln, M(z) / ln))
        lf = math.sqrt(x * x + y * y + z * z)  # vec3.rs:179-181
        ref.append((x / lf, y / lf, z / lf))
    assert loops > 400  # the rejection branch ran (about 48 % of the candidates are rejected)
    _rule("random_unit_vector", _vec_err(got[:, :3], exact), _vec_err(ref, exact))


# ---------------------------------------------------------------- sphere_test_v
def _one_sphere_blob(center, radius):
    sc = rt.Scene(1)
    return sc.serialize(sc.hittable_list(sc.sphere(center, radius, sc.lambertian((1, 1, 1)))), None)


def _oracle_t(blob, o, d, tmin, tmax):
    h = O.world_hit(blob, list(o) + list(d) + [0.0], tmin, tmax)
    return None if h is None else float(h[0])


def _sphere_rec(c, r, o, d, tmin, tmax):
    return list(c) + [r] + list(o) + list(d) + [tmin, tmax, SENT]


def test_sphere_test_v_known_answers(gpu_available):
    c, r = (0.0, 0.0, 0.0), 1.0
    blob = _one_sphere_blob(c, r)
    cases = [  # o, d, tmin, tmax, expected t (None: miss)
        ((0, 0, -5), (0, 0, 1), 1e-4, INF, 4.0),     # outside
        ((0, 0, 0), (0, 0, 2), 1e-4, INF, 0.5),      # inside, non-unit direction
        ((0, 0, -5), (0, 0, 1), 1e-4, 4.0, None),    # a root exactly at tmax: strict interval
        ((0, 0, -5), (0, 0, 1), 1e-4, 6.0, 4.0),
        ((0, 0, -5), (0, 0, 1), 4.0, INF, 6.0),      # near root exactly at tmin: the far root
        ((0, 0, -5), (0, 0, 1), 4.0, 6.0, None),     # ... which sits exactly at tmax
        ((0, 0, -1), (0, 0, 1), 1e-4, INF, 2.0),     # origin on the surface: the far root
        ((1, 0, -5), (0, 0, 1), 1e-4, INF, 5.0),     # tangent, disc == 0: a hit
        ((2, 0, -5), (0, 0, 1), 1e-4, INF, None),    # disc < 0
        ((0, 0, 5), (0, 0, 1), 1e-4, INF, None),     # both roots behind
    ]
    got = P.run("sphere_test_v", [_sphere_rec(c, r, o, d, a, b) for o, d, a, b, _ in cases])
    for (o, d, a, b, want), g in zip(cases, got):
        assert _oracle_t(blob, o, d, a, b) == want, (o, d, a, b)
        assert g[0] == (want is not None) and g[1] == (SENT if want is None else want), (o, d, a, b, g)
        oc = np.array(o, float)
        aa, hb = float(np.dot(d, d)), float(np.dot(oc, d))
        assert g[2:5].tolist() == [aa, hb, hb * hb - aa * (float(np.dot(oc, oc)) - 1.0)], g


def _sphere_exact(c, r, o, d, tmin, tmax):
    """Sphere::hit (object.rs:145-166) in exact arithmetic on the f64 inputs: (t or None, guard)."""
    c, o, d = _fr(c), _fr(o), _fr(d)
    oc = [p - q for p, q in zip(o, c)]
    a, hb = _dot(d, d), _dot(oc, d)
    cc = _dot(oc, oc) - Fr(r) ** 2
    disc = hb * hb - a * cc
    guard = abs(disc) <= Fr(1, 10 ** 9) * max(hb * hb, abs(a * cc))
    if disc < 0:
        return None, guard
    sq = mp.sqrt(M(disc.numerator) / M(disc.denominator))
    am, hm = M(a.numerator) / M(a.denominator), M(hb.numerator) / M(hb.denominator)
    roots = [(-hm - sq) / am, (sq - hm) / am]
    guard = guard or any(_near(t, b) for t in roots for b in (tmin, tmax))
    for t in roots:
        if tmin < t < tmax:
            return t, guard
    return None, guard


def _sphere_rays(rng, n):
    c = (0.3, -0.2, 0.5)
    out = []
    for k in range(n):
        r = (0.02, 1.0, 1000.0)[k % 3]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if r == 1000.0:
            dist = rng.uniform(0.0, 1000.0)  # inside: origins up to 1e3 away
        elif rng.random() < 0.1:
            dist = rng.uniform(0.0, 0.9) * r
        else:
            # log-uniform in [1.5 r, 1e3 r] and at most 1e3: farther out, disc / half_b^2 ~ (r / dist)^2
            # falls below the guard band's 1e-9 and every ray of the small sphere would be left out
            far = min(1e3, 1e3 * r)
            dist = r * 1.5 * (far / (1.5 * r)) ** rng.random()
        o = np.array(c) + dist * u
        b = rng.normal(size=3)
        b *= rng.random() ** (1 / 3) / np.linalg.norm(b)
        d = (np.array(c) + 1.3 * r * b - o)
        d *= rng.uniform(0.5, 2.0) / max(np.linalg.norm(d), 1e-3)
        tmax = INF
        if rng.random() < 0.3:  # a finite tmax around the roots
            tmax = float(rng.uniform(0.7, 1.3) * max(np.linalg.norm(np.array(c) - o) / np.linalg.norm(d), 1e-3))
        out.append((c, r, tuple(o.tolist()), tuple(d.tolist()), 1e-4, tmax))
    return out


def test_sphere_test_v_random_rays(gpu_available):
    rays = _sphere_rays(np.random.default_rng(106), 2048)
    blobs = {r: _one_sphere_blob((0.3, -0.2, 0.5), r) for r in (0.02, 1.0, 1000.0)}
    got = P.run("sphere_test_v", [_sphere_rec(*ray) for ray in rays])
    left_out, hits, dev_w, ora_w = 0, 0, M(0), M(0)
    for (c, r, o, d, tmin, tmax), g in zip(rays, got):
        t, guard = _sphere_exact(c, r, o, d, tmin, tmax)
        if guard:
            left_out += 1
            continue
        ot = _oracle_t(blobs[r], o, d, tmin, tmax)
        assert (ot is not None) == (t is not None), ("oracle", r, o, d, tmin, tmax)
        assert bool(g[0]) == (t is not None), ("device", r, o, d, tmin, tmax, g.tolist())
        if t is None:
            assert g[1] == SENT
            continue
        hits += 1
        dev_w = max(dev_w, abs(M(float(g[1])) - t) / t)
        ora_w = max(ora_w, abs(M(ot) - t) / t)
    share = left_out / len(rays)
    print(f"sphere_test_v: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %")
    assert share <= 0.01 and 0.3 * len(rays) < hits < 0.9 * len(rays)
    _rule("sphere_test_v t", float(dev_w), float(ora_w))


# ---------------------------------------------------------------- quads
RT_OBJ_LIST, RT_OBJ_QUAD = 1, 4
_LIT = r"\(?(-?0x[0-9a-fp.+-]+)\)?"


def _quad_case(q, u, v, light=False):
    """One-quad scene -> (blob, K or None, record constants). The axis-aligned record's constants
    are the generated walker's AQuad{...} literals (rt.jit_check, as tests/test_quad_bounds.py);
    the general payload is n, D, q, area as the host builder serialised them (include/rt_mi355x.h
    RT_OBJ_QUAD) with A = v x w and B = w x u, one cross product each as rt_flatten.cpp forms them
    (the generated source reads that payload from the node table, so it holds no literal of it;
    for a light quad it does carry n and area, which are compared)."""
    sc = rt.Scene(2)
    m = sc.diffuse_light((4, 4, 4)) if light else sc.lambertian((0.5, 0.5, 0.5))
    world = sc.hittable_list(sc.quad(q, u, v, m))
    blob = sc.serialize(world, sc.hittable_list(sc.quad(q, u, v, m)) if light else None)
    state, src = rt.jit_check(blob)
    assert state == 1
    s = blob.slots
    p = blob.header()["world_off"]
    assert int(s[p]) == RT_OBJ_LIST and int(s[p + 1]) == 1 and int(s[p + 8]) == RT_OBJ_QUAD
    f = [float(np.uint64(s[p + 10 + k]).view(np.float64)) for k in range(17)]
    qq, uu, vv, n, w, D, area = f[0:3], f[3:6], f[6:9], f[9:12], f[12:15], f[15], f[16]
    A = [vv[1] * w[2] - vv[2] * w[1], vv[2] * w[0] - vv[0] * w[2], vv[0] * w[1] - vv[1] * w[0]]
    B = [w[1] * uu[2] - w[2] * uu[1], w[2] * uu[0] - w[0] * uu[2], w[0] * uu[1] - w[1] * uu[0]]
    gen = [0.0, 0.0] + n + [D] + qq + [area] + A + [0.0] + B + [0.0]
    lits = re.findall(r"aquad_test<COUNT, (\d)>\(AQuad\{(\d+)u, " + ", ".join([_LIT] * 5) + r"\}, o, d", src)
    lw = re.search(r"quad_light_w\(dir, t, mk\(" + ", ".join([_LIT] * 3) + r"\), " + _LIT + r"\)", src)
    if light:
        assert [float.fromhex(x) for x in lw.groups()] == n + [area]
    if not lits:
        assert "quad_test<COUNT>(N + " in src
        return blob, None, gen
    assert len(lits) == 1
    K, h0, *vals = lits[0]
    return blob, int(K), ([float(h0)] + [float.fromhex(x) for x in vals], gen)


def _aquad_rec(K, consts, o, d, tmin, tmax):
    return [float(K)] + list(consts) + list(o) + list(d) + [tmin, tmax, SENT]


def _gquad_rec(gen, o, d, tmin, tmax):
    return list(gen) + list(o) + list(d) + [tmin, tmax, SENT, 0.0]


def _axes(K):
    return (1 if K == 0 else 0), (1 if K == 2 else 2)


def _point(K, yk, ya, yb):
    p = [0.0, 0.0, 0.0]
    lo, hi = _axes(K)
    p[K], p[lo], p[hi] = yk, ya, yb
    return tuple(p)


AXIS_QUADS = {0: ((3, -1, -1), (0, 2, 0), (0, 0, 2)), 1: ((-1, 3, -1), (2, 0, 0), (0, 0, 2)),
              2: ((-1, -1, 3), (2, 0, 0), (0, 2, 0))}
GENERAL_QUAD = ((0.5, -1.25, 2.0), (1.5, 0.5, 0.25), (-0.5, 2.0, 1.0))


# aquad_test_nr1 forms r with rcp_nr1 (one Newton step), as every caller of aquad_test does;
# aquad_test with the two-step rcp_nr (whose cases keep the ids [0], [1], [2])
AQUAD_FORMS = pytest.mark.parametrize("K,form", [
    pytest.param(K, form, id=f"{K}{tag}") for form, tag in (("aquad_test", ""), ("aquad_test_nr1", "-nr1"))
    for K in (0, 1, 2)])


@AQUAD_FORMS
def test_aquad_test_exact_cases(gpu_available, K, form):
    blob, k, (consts, gen) = _quad_case(*AXIS_QUADS[K])
    assert k == K
    _, qk, lo0, lo1, hi0, hi1 = consts
    assert qk == 3.0 and lo0 == -1.0 and hi0 == -1.0
    up, dn = (lambda x: math.nextafter(x, INF)), (lambda x: math.nextafter(x, -INF))
    dirk = _point(K, 1.0, 0.0, 0.0)
    cases = [  # o, d, tmin, tmax, expected t or None
        (_point(K, 0, 0, 0), dirk, 1e-4, INF, 3.0),
        (_point(K, 0, 0, 0), dirk, 3.0, INF, 3.0),        # t == tmin: inclusive
        (_point(K, 0, 0, 0), dirk, 1e-4, 3.0, 3.0),       # t == tmax: inclusive
        (_point(K, 0, 0, 0), dirk, 3.0, 3.0, 3.0),
        (_point(K, 0, 0, 0), dirk, up(3.0), INF, None),
        (_point(K, 0, 0, 0), dirk, 1e-4, dn(3.0), None),
        (_point(K, 0, lo0, 0), dirk, 1e-4, INF, 3.0),      # the hit point exactly on each bound
        (_point(K, 0, lo1, 0), dirk, 1e-4, INF, 3.0),
        (_point(K, 0, 0, hi0), dirk, 1e-4, INF, 3.0),
        (_point(K, 0, 0, hi1), dirk, 1e-4, INF, 3.0),
        (_point(K, 0, lo0, hi1), dirk, 1e-4, INF, 3.0),
        (_point(K, 0, dn(lo0), 0), dirk, 1e-4, INF, None),  # its neighbour outside
        (_point(K, 0, up(lo1), 0), dirk, 1e-4, INF, None),
        (_point(K, 0, 0, dn(hi0)), dirk, 1e-4, INF, None),
        (_point(K, 0, 0, up(hi1)), dirk, 1e-4, INF, None),
        (_point(K, 3, 0, 0), _point(K, 0.0, 1, 0), 1e-4, INF, None),   # d_k = 0, origin in the plane
        (_point(K, 0, 0, 0), _point(K, 0.0, 1, 0), 1e-4, INF, None),   # d_k = 0, parallel
        (_point(K, 0, 0, 0), _point(K, dn(1e-8), 0, 0), 1e-4, INF, None),  # |n.d| < 1e-8
        (_point(K, 0, 0, 0), _point(K, -dn(1e-8), 0, 0), -INF, INF, None),
        (_point(K, 0, 0, 0), _point(K, 1e-8, 0, 0), 1e-4, INF, float(Fr(3) / Fr(1e-8))),  # passes
        (_point(K, 6, 0, 0), _point(K, -1e-8, 0, 0), 1e-4, INF, float(Fr(3) / Fr(1e-8))),
    ]
    # (A NaN planar coordinate, which the accept comparisons let through, needs a non-finite ray:
    # there the reference's n . o or n . d is NaN as well and the test misses. Not a case here.)
    got = P.run(form, [_aquad_rec(K, consts, o, d, a, b) for o, d, a, b, _ in cases])
    gq = P.run("quad_test", [_gquad_rec(gen, o, d, a, b) for o, d, a, b, _ in cases])
    for (o, d, a, b, want), g, gg in zip(cases, got, gq):
        ot = _oracle_t(blob, o, d, a, b)
        assert ot == want, ("oracle", o, d, a, b, ot)  # 3 / 1e-8: the oracle's IEEE quotient
        hit = want is not None
        assert bool(g[0]) == hit and bool(gg[0]) == hit, (o, d, a, b, g.tolist(), gg.tolist())
        if not hit:
            assert g[1] == SENT and gg[1] == SENT, "a miss leaves t_out untouched"
        elif want == 3.0:
            assert g[1] == 3.0 and gg[1] == 3.0 and g[2] == 3.0
        else:
            assert abs(_ord1(g[1]) - _ord1(want)) <= 1 and abs(_ord1(gg[1]) - _ord1(want)) <= 1
            assert g[2] == g[1]
    # the general form's own planar edges on this dyadic quad: a = (y + 1) / 2 exactly
    lo_ax, hi_ax = _axes(K)
    edge = [(_point(K, 0, -1.0, 1.0), 3.0), (_point(K, 0, 1.0, -1.0), 3.0),
            (_point(K, 0, 1.0 + 2.0 ** -51, 0), None), (_point(K, 0, 0, -1.0 - 2.0 ** -52), None)]
    ge = P.run("quad_test", [_gquad_rec(gen, o, dirk, 1e-4, INF) for o, _ in edge])
    for (o, want), g in zip(edge, ge):
        assert _oracle_t(blob, o, dirk, 1e-4, INF) == want
        assert g.tolist() == ([1.0, 3.0] if want else [0.0, SENT]), (o, g)


def _aquad_exact(K, consts, o, d, tmin, tmax):
    """The axis-aligned test in exact arithmetic: (hit, t, plane & inr, t's quotient, guard)."""
    _, qk, lo0, lo1, hi0, hi1 = consts
    o, d = _fr(o), _fr(d)
    lo_ax, hi_ax = _axes(K)
    plane = not abs(d[K]) < Fr(1e-8)
    guard = _near(abs(d[K]), 1e-8)
    if d[K] == 0:
        return False, None, False, guard
    t = (Fr(qk) - o[K]) / d[K]
    ya, yb = o[lo_ax] + t * d[lo_ax], o[hi_ax] + t * d[hi_ax]
    inr = Fr(lo0) <= ya <= Fr(lo1) and Fr(hi0) <= yb <= Fr(hi1)
    for y, (b0, b1) in ((ya, (lo0, lo1)), (yb, (hi0, hi1))):
        ext = Fr(1, 10 ** 9) * max(abs(y), abs(Fr(b0)), abs(Fr(b1)))
        guard = guard or abs(y - Fr(b0)) <= ext or abs(y - Fr(b1)) <= ext
    guard = guard or _near(t, tmin) or _near(t, tmax)
    return plane and tmin <= t <= tmax and inr, t, plane and inr, guard


def _gquad_exact(gen, o, d, tmin, tmax):
    """Quad::hit (object.rs:453-476) in exact arithmetic on the record's constants."""
    n, D, q, A, B = _fr(gen[2:5]), Fr(gen[5]), _fr(gen[6:9]), _fr(gen[10:13]), _fr(gen[14:17])
    o, d = _fr(o), _fr(d)
    den = _dot(n, d)
    guard = _near(abs(den), 1e-8)
    if den == 0:
        return False, None, guard
    t = (D - _dot(n, o)) / den
    pq = [oo + t * dd - qq for oo, dd, qq in zip(o, d, q)]
    a, b = _dot(pq, A), _dot(pq, B)
    eps = Fr(1, 10 ** 9)
    guard = guard or any(abs(x) <= eps or abs(x - 1) <= eps for x in (a, b))
    guard = guard or _near(t, tmin) or _near(t, tmax)
    hit = not abs(den) < Fr(1e-8) and tmin <= t <= tmax and 0 <= a <= 1 and 0 <= b <= 1
    return hit, t, guard


def _quad_rays(rng, q, u, v, n):
    q, u, v = (np.array(x, float) for x in (q, u, v))
    nrm = np.cross(u, v)
    nrm /= np.linalg.norm(nrm)
    out = []
    for _ in range(n):
        a, b = rng.uniform(-0.25, 1.25, 2)  # the target: inside about half of the time
        target = q + a * u + b * v
        o = target + nrm * rng.uniform(0.5, 30.0) * rng.choice([-1.0, 1.0]) + rng.normal(size=3) * 3.0
        d = (target - o) * rng.uniform(0.05, 3.0)
        if rng.random() < 0.1:
            d = -d  # the plane lies behind
        tmax = INF if rng.random() < 0.6 else float(np.linalg.norm(target - o) / np.linalg.norm(d)
                                                      * rng.uniform(0.6, 1.4))
        out.append((tuple(o.tolist()), tuple(d.tolist()), 1e-4, tmax))
    return out


@AQUAD_FORMS
def test_aquad_test_random_rays(gpu_available, K, form):
    blob, k, (consts, _) = _quad_case(*AXIS_QUADS[K])
    rays = _quad_rays(np.random.default_rng(110 + K), *AXIS_QUADS[K], 1024)
    got = P.run(form, [_aquad_rec(K, consts, *ray) for ray in rays])
    left_out, hits, dev_w, ora_w = 0, 0, Fr(0), Fr(0)
    for (o, d, tmin, tmax), g in zip(rays, got):
        hit, t, pinr, guard = _aquad_exact(K, consts, o, d, tmin, tmax)
        if guard:
            left_out += 1
            continue
        ot = _oracle_t(blob, o, d, tmin, tmax)
        assert (ot is not None) == hit, ("oracle", o, d, tmin, tmax)
        assert bool(g[0]) == hit and bool(g[3]) == pinr, ("device", o, d, tmin, tmax, g.tolist())
        # the plane quotient is handed out whatever the interval says: div_nr(fl(q_k - o_k), d_k)
        want_tp = float(Fr(consts[1] - o[K]) / Fr(d[K]))
        assert abs(_ord1(g[2]) - _ord1(want_tp)) <= 1, (o, d, g.tolist(), want_tp)
        if not hit:
            assert g[1] == SENT
            continue
        assert g[1] == g[2]
        hits += 1
        dev_w = max(dev_w, abs(Fr(float(g[1])) - t) / t)
        ora_w = max(ora_w, abs(Fr(ot) - t) / t)
    share = left_out / len(rays)
    print(f"{form}<{K}>: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %")
    assert share <= 0.01 and 0.2 * len(rays) < hits < 0.8 * len(rays)
    _rule(f"{form}<{K}> t", float(dev_w), float(ora_w))


def test_quad_test_random_rays(gpu_available):
    blob, k, gen = _quad_case(*GENERAL_QUAD, light=True)
    assert k is None
    rays = _quad_rays(np.random.default_rng(113), *GENERAL_QUAD, 2048)
    got = P.run("quad_test", [_gquad_rec(gen, *ray) for ray in rays])
    left_out, hits, dev_w, ora_w = 0, 0, Fr(0), Fr(0)
    for (o, d, tmin, tmax), g in zip(rays, got):
        hit, t, guard = _gquad_exact(gen, o, d, tmin, tmax)
        if guard:
            left_out += 1
            continue
        ot = _oracle_t(blob, o, d, tmin, tmax)
        assert (ot is not None) == hit, ("oracle", o, d, tmin, tmax)
        assert bool(g[0]) == hit, ("device", o, d, tmin, tmax, g.tolist())
        if not hit:
            assert g[1] == SENT
            continue
        hits += 1
        dev_w = max(dev_w, abs(Fr(float(g[1])) - t) / t)
        ora_w = max(ora_w, abs(Fr(ot) - t) / t)
    share = left_out / len(rays)
    print(f"quad_test: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %")
    assert share <= 0.01 and 0.2 * len(rays) < hits < 0.8 * len(rays)
    _rule("quad_test t", float(dev_w), float(ora_w))


# ---------------------------------------------------------------- aabb_hit, aabb_hit_bf
def _aabb_ref(mn, mx, o, inv, tmin, tmax):
    """Aabb::hit object.rs:340-370 (subtractions, products and comparisons only)."""
    for a in range(3):
        t0 = (mn[a] - o[a]) * inv[a]
        t1 = (mx[a] - o[a]) * inv[a]
        if inv[a] < 0.:
            t0, t1 = t1, t0
        if t0 > tmin:
            tmin = t0
        if t1 < tmax:
            tmax = t1
        if tmax <= tmin:
            return False
    return True


def test_aabb_hit_both_forms(gpu_available):
    rng = np.random.default_rng(120)
    recs = []
    with np.errstate(divide="ignore"):
        for k in range(4096):
            c = rng.uniform(-50, 50, 3)
            h = rng.uniform(0.01, 20, 3) * (rng.random(3) < 0.9)  # some flat boxes: mn == mx
            o = rng.uniform(-100, 100, 3)
            d = (c + rng.uniform(-1.5, 1.5, 3) * h) - o
            d *= rng.uniform(0.1, 2.0)
            ax = rng.integers(0, 3)
            if k % 16 == 0:
                d[ax] = rng.choice([0.0, -0.0])  # inv = +-inf
            if k % 64 == 0:
                o[ax] = (c - h)[ax]  # ... with the origin on the slab plane: a NaN bound
            tmin, tmax = (1e-4, INF) if k % 3 else (float(rng.uniform(0, 2)), float(rng.uniform(0, 3)))
            recs.append(np.concatenate([c - h, c + h, o, 1.0 / d, [tmin, tmax]]))
        box = ([-1., -2., -3.], [1., 2., 3.])
        for inv_x in (INF, -INF):
            for ox in (-1.0, 1.0, 0.0, 0.5, -1.5, 1.5):  # on the slab planes, inside, outside
                for oy, iy in ((0.0, 0.5), (-10.0, 0.25), (10.0, 0.25), (-10.0, -0.25)):
                    for tmin, tmax in ((1e-4, INF), (-INF, INF), (0.0, 100.0)):
                        recs.append(box[0] + box[1] + [ox, oy, 0.5, inv_x, iy, INF, tmin, tmax])
        for tmin, tmax in ((-INF, INF), (1.0, 1.0), (2.0, 1.0), (0.0, 1e300), (1e-4, INF)):
            recs.append(box[0] + box[1] + [0.0, 0.0, -10.0, INF, -INF, 1.0, tmin, tmax])  # through
            recs.append(box[0] + box[0] + [-5.0, -2.0, -3.0, 0.25, INF, INF, tmin, tmax])  # mn == mx
            recs.append([0.] * 6 + [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0, tmin, tmax])
            recs.append(box[0] + box[1] + [-2.0, 0.0, 0.0, 1.0, INF, INF, tmin, tmax])
    recs = np.array([np.asarray(r, np.float64) for r in recs])
    with np.errstate(invalid="ignore"):
        want = np.array([_aabb_ref(r[0:3], r[3:6], r[6:9], r[9:12], r[12], r[13]) for r in recs.tolist()])
    got = P.run("aabb_hit", recs)
    print(f"aabb_hit: {len(recs)} boxes and rays, {int(want.sum())} hits")
    assert 0.25 * len(recs) < want.sum() < 0.75 * len(recs)
    for col, name in ((0, "aabb_hit"), (1, "aabb_hit_bf")):
        bad = np.nonzero(got[:, col].astype(bool) != want)[0]
        assert len(bad) == 0, (name, recs[bad[0]].tolist())


# ---------------------------------------------------------------- transforms and vector helpers
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _mp3(v):
    return [M(x) for x in v]


def test_rotate_y_in_and_out(gpu_available):
    rng = np.random.default_rng(130)
    ang = np.radians(np.concatenate([rng.uniform(-180, 180, 508), [15.0, -18.0, 90.0, 0.0]]))
    s, c = np.sin(ang), np.cos(ang)
    a = rng.uniform(-600, 600, (512, 3))
    b = _unit(rng, 512) * rng.uniform(0.5, 2.0, (512, 1))
    recs = np.concatenate([s[:, None], c[:, None], a, b], 1)
    for name, sg in (("rotate_y_in", -1.0), ("rotate_y_out", 1.0)):
        got = P.run(name, recs)
        exact, ref = [], []
        for r in recs.tolist():
            sn, cs = r[0], r[1]
            for v in (r[2:5], r[5:8]):  # transform.rs:89-105 (in), 115-127 (out)
                x, y, z = _mp3(v)
                exact.append((M(cs) * x + sg * M(sn) * z, y, -sg * M(sn) * x + M(cs) * z))
                if sg < 0:
                    ref.append((cs * v[0] - sn * v[2], v[1], sn * v[0] + cs * v[2]))
                else:
                    ref.append((cs * v[0] + sn * v[2], v[1], -sn * v[0] + cs * v[2]))
        _rule(name, _vec_err(got.reshape(-1, 3), exact), _vec_err(ref, exact))


def _refract_ref(uv, n, e):  # vec3.rs:223-229
    ct = min(-uv[0] * n[0] + -uv[1] * n[1] + -uv[2] * n[2], 1.)
    perp = [e * (uv[k] + ct * n[k]) for k in range(3)]
    par = math.sqrt(abs(1.0 - (perp[0] * perp[0] + perp[1] * perp[1] + perp[2] * perp[2])))
    return [perp[k] + par * -1. * n[k] for k in range(3)]


def _refract_exact(uv, n, e):
    uv, n, e = _mp3(uv), _mp3(n), M(e)
    ct = min(-_dot(uv, n), M(1))
    perp = [e * (uv[k] + ct * n[k]) for k in range(3)]
    par = mp.sqrt(abs(1 - _dot(perp, perp)))
    return [perp[k] - par * n[k] for k in range(3)]


def test_reflect_refract_unit_vector_onb_local(gpu_available):
    rng = np.random.default_rng(131)
    n = _unit(rng, 512)
    v = _unit(rng, 512) * rng.uniform(0.5, 2.0, (512, 1))
    got = P.run("reflect", np.concatenate([v, n], 1))
    exact = [[a - 2 * _dot(_mp3(vv), _mp3(nn)) * b for a, b in zip(_mp3(vv), _mp3(nn))]
             for vv, nn in zip(v.tolist(), n.tolist())]
    ref = [[vv[k] - 2. * (vv[0] * nn[0] + vv[1] * nn[1] + vv[2] * nn[2]) * nn[k] for k in range(3)]
           for vv, nn in zip(v.tolist(), n.tolist())]  # vec3.rs:219-221
    _rule("reflect", _vec_err(got, exact), _vec_err(ref, exact))

    # refract: unit uv entering against n, both sides of total internal reflection
    uv = _unit(rng, 512)
    uv = np.where((np.sum(uv * n, 1) > 0)[:, None], -uv, uv)
    e = np.where(rng.random(512) < 0.5, 1.0 / 1.5, 1.5) * rng.uniform(0.9, 1.1, 512)
    recs = np.concatenate([uv, n, e[:, None]], 1)
    sin2 = 1 - np.sum(uv * n, 1) ** 2
    tir = e * e * sin2 > 1
    assert 50 < tir.sum() < 400
    got = P.run("refract", recs)
    exact = [_refract_exact(r[0:3], r[3:6], r[6]) for r in recs.tolist()]
    ref = [_refract_ref(r[0:3], r[3:6], r[6]) for r in recs.tolist()]
    _rule("refract", _vec_err(got, exact), _vec_err(ref, exact))
    # |perp|^2 within an ulp of 1: sin(theta) = 1 / e against n = +y
    crit = []
    for ee in np.linspace(1.05, 2.45, 96).tolist():
        sn = 1.0 / ee
        crit.append([sn, -math.sqrt(1.0 - sn * sn), 0.0, 0.0, 1.0, 0.0, ee])
    assert all(abs((Fr(r[6]) * Fr(r[0])) ** 2 - 1) <= Fr(1001, 1000) * Fr(2) ** -52 for r in crit)
    got = P.run("refract", crit)
    exact = [_refract_exact(r[0:3], r[3:6], r[6]) for r in crit]
    ref = [_refract_ref(r[0:3], r[3:6], r[6]) for r in crit]
    _rule("refract at the critical angle", _vec_err(got, exact), _vec_err(ref, exact))

    w = rng.normal(size=(512, 3)) * np.exp(rng.uniform(-8, 8, (512, 1)))
    got = P.run("unit_vector", w)
    exact, ref = [], []
    for r in w.tolist():
        ln = mp.sqrt(_dot(_mp3(r), _mp3(r)))
        exact.append([x / ln for x in _mp3(r)])
        lf = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])  # vec3.rs:179-181
        ref.append([x / lf for x in r])
    _rule("unit_vector", _vec_err(got, exact), _vec_err(ref, exact))

    bu, bv, bw = _unit(rng, 512), _unit(rng, 512), _unit(rng, 512)
    a = _unit(rng, 512)
    recs = np.concatenate([bu, bv, bw, a], 1)
    got = P.run("onb_local", recs)
    exact, ref = [], []
    for r in recs.tolist():
        u_, v_, w_, a_ = r[0:3], r[3:6], r[6:9], r[9:12]
        exact.append([M(a_[0]) * M(u_[k]) + M(a_[1]) * M(v_[k]) + M(a_[2]) * M(w_[k]) for k in range(3)])
        ref.append([a_[0] * u_[k] + a_[1] * v_[k] + a_[2] * w_[k] for k in range(3)])  # onb.rs:24-26
    _rule("onb_local", _vec_err(got, exact), _vec_err(ref, exact))


# ---------------------------------------------------------------- sphere_uv_f
def test_sphere_uv_f(gpu_available):
    pts = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], float)
    uv = P.run("sphere_uv_f", pts)
    exp = [(math.atan2(-z, x) + math.pi) / (2 * math.pi) for x, y, z in pts]
    np.testing.assert_allclose(uv[:, 0], exp, atol=1e-15, rtol=0)
    np.testing.assert_allclose(uv[:, 1], [0.5, 1.0, 0.5, 0.5, 0.0, 0.5], atol=1e-15, rtol=0)
    rng = np.random.default_rng(140)
    p = _unit(rng, 2300)
    p = p[np.abs(p[:, 1]) <= 1 - 2.0 ** -20][:2048]
    assert len(p) == 2048
    got = P.run("sphere_uv_f", p)
    ora = O.sphere_uv(p)
    dev_w = ora_w = M(0)
    for (x, y, z), g, r in zip(p.tolist(), got.tolist(), ora.tolist()):
        eu = (mp.atan2(-M(z), M(x)) + mp.pi) / (2 * mp.pi)
        ev = mp.acos(-M(y)) / mp.pi
        dev_w = max(dev_w, abs(M(g[0]) - eu), abs(M(g[1]) - ev))
        ora_w = max(ora_w, abs(M(r[0]) - eu), abs(M(r[1]) - ev))
    _rule("sphere_uv_f (absolute)", float(dev_w), float(ora_w))


# ---------------------------------------------------------------- perlin_turb
def _turb_f32(ranvec, perms, pts):
    """perlin.rs:30-96 in numpy float32, operation by operation (vectorised over the points)."""
    f = np.float32
    rv = ranvec.astype(f)
    p = pts.astype(f)
    accum = np.zeros(len(p), f)
    weight = f(1)
    for _ in range(7):
        fl = np.floor(p)
        u, v, w = (p - fl).T
        ijk = np.clip(fl.astype(np.float64), -2147483648.0, 2147483647.0).astype(np.int64)
        uu, vv, ww = (x * x * (f(3) - f(2) * x) for x in (u, v, w))
        acc = np.zeros(len(p), f)
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    c = rv[perms[0][(ijk[:, 0] + i) & 255] ^ perms[1][(ijk[:, 1] + j) & 255]
                           ^ perms[2][(ijk[:, 2] + k) & 255]]
                    d = (c[:, 0] * (u - f(i)) + c[:, 1] * (v - f(j))) + c[:, 2] * (w - f(k))
                    acc = acc + ((f(i) * uu + (f(1) - f(i)) * (f(1) - uu))
                                 * (f(j) * vv + (f(1) - f(j)) * (f(1) - vv))
                                 * (f(k) * ww + (f(1) - f(k)) * (f(1) - ww)) * d)
        accum = accum + weight * acc
        weight = weight * f(0.5)
        p = p * f(2)
    return np.abs(accum)


def test_perlin_turb(gpu_available):
    rng = np.random.default_rng(11)  # the tables and points of test_perlin_turb_matches_the_...
    ranvec = rng.normal(size=(256, 3))
    ranvec /= np.linalg.norm(ranvec, axis=1, keepdims=True)
    perms = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.int32)
    kat = np.concatenate([rng.uniform(-300, 300, size=(200, 3)), rng.uniform(-2, 2, size=(56, 3))])
    table = np.zeros(P.PERLIN_BYTES, np.uint8)  # rt_layout.h: 256 x float4, then perm_x / y / z
    rv4 = np.zeros((256, 4), np.float32)
    rv4[:, :3] = ranvec
    table[:4096] = rv4.view(np.uint8).reshape(-1)
    table[4096:] = perms.astype(np.uint8).reshape(-1)

    r2 = np.random.default_rng(150)
    q = lambda a: np.round(a * 2.0 ** 12) / 2.0 ** 12  # noqa: E731  (f32-exact coordinates)
    ints = r2.integers(-260, 260, (64, 3)).astype(np.float64)
    edges = np.concatenate([
        ints, ints + 0.5,
        q(r2.uniform(-1, 0, (64, 3))),                       # cell index -1
        q(r2.uniform(255, 256, (32, 3))), q(r2.uniform(-256, -255, (32, 3))),  # the index wrap
        np.where(r2.random((64, 3)) < 0.5, q(r2.uniform(-1, 0, (64, 3))), q(r2.uniform(255, 256, (64, 3)))),
        [[-0.0, -0.0, -0.0], [0.0, -0.0, 0.25], [-0.0, 255.5, -255.5], [-1.0, 255.0, -256.0],
         [254.99951171875, -0.000244140625, 127.5]],
    ])
    assert np.array_equal(edges, edges.astype(np.float32).astype(np.float64))
    for name, pts in (("perlin_turb, the oracle test's points", kat), ("perlin_turb, lattice edges", edges)):
        pts = np.ascontiguousarray(pts)
        ref = np.zeros(len(pts))
        O.lib(64).oracle_perlin_turb(ranvec.ctypes.data, perms.ctypes.data, pts.ctypes.data, len(pts),
                                     ref.ctypes.data)
        got = P.perlin_turb(table, pts)
        f32 = _turb_f32(ranvec, perms, pts).astype(np.float64)
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
        _rule(name + " (absolute)", float(np.abs(got - ref).max()), float(np.abs(f32 - ref).max()))
    z = P.perlin_turb(table, ints)
    assert np.array_equal(z, np.zeros(len(ints)))  # every offset is zero on the lattice


# ---------------------------------------------------------------- light weights
def test_quad_light_w(gpu_available):
    rng = np.random.default_rng(160)
    n = _unit(rng, 3000)
    d = _unit(rng, 3000)
    keep = np.abs(np.sum(n * d, 1)) >= 0.2  # a light seen at a grazing angle cancels in d . n alike
    n, d = n[keep][:2048], d[keep][:2048] * np.exp(rng.uniform(-3, 3, (2048, 1)))
    t = np.exp(rng.uniform(-2, 6, 2048))
    area = np.exp(rng.uniform(-3, 9, 2048))
    recs = np.concatenate([d, t[:, None], n, area[:, None]], 1)
    got = P.run("quad_light_w", recs)[:, 0]
    # object.rs:492-501 in f64 and in float32
    len2 = np.sum(d * d, 1)
    want = (t * t * len2) / (np.abs(np.sum(d * n, 1) / np.sqrt(len2)) * area)
    f = np.float32
    d32, n32, t32, a32 = d.astype(f), n.astype(f), t.astype(f), area.astype(f)
    l32 = (d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]
    dn32 = (d32[:, 0] * n32[:, 0] + d32[:, 1] * n32[:, 1]) + d32[:, 2] * n32[:, 2]
    w32 = (t32 * t32 * l32) / (np.abs(dn32 / np.sqrt(l32)) * a32)
    _rule("quad_light_w (relative)", float(np.abs(got / want - 1).max()),
          float(np.abs(w32.astype(np.float64) / want - 1).max()))


def test_sphere_light_w(gpu_available):
    rng = np.random.default_rng(161)
    cm = np.concatenate([rng.uniform(0.0, 0.99, 1024), 1.0 - np.exp(rng.uniform(-16, -4, 1024))])
    near = 1.0 - 2.0 ** -np.arange(10, 31).astype(np.float64)  # small distant lights
    got = P.run("sphere_light_w", np.concatenate([cm, near, [1.0]]))[:, 0]
    ref = lambda c: 1. / (2. * math.pi * (1. - c))  # noqa: E731  object.rs:190-202
    f = np.float32
    w32 = (f(1) / ((f(2) * f(math.pi)) * (f(1) - cm[:1024].astype(f)))).astype(np.float64)
    bound = float(np.abs(w32 / ref(cm[:1024]) - 1).max())
    dev = float(np.abs(got[:len(cm)] / ref(cm) - 1).max())
    _rule("sphere_light_w (relative)", dev, bound)
    g = got[len(cm):-1]
    assert np.isfinite(g).all() and g[-1] > 0
    dev_near = float(np.abs(g / ref(near) - 1).max())
    _rule("sphere_light_w near cos_max = 1 (relative)", dev_near, bound)
    assert got[-1] == INF
