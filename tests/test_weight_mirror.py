"""Host-only: the f32 mirrors of the weight constants in the flattened tables (rt_layout.h
RTL_MATF_SOLID_W, rt_flatten.cpp). Every mirror word is the bits of np.float32(field) -- the host's
round-to-nearest-even cast with subnormals kept, which tests/test_weight_mirror_gpu.py shows to be
the device's to_w3 -- the solid-weight flag is set exactly on the materials whose texture is SOLID,
and everything else in the two tables is what a flatten without mirrors writes: this file restates
that layout from the serialised scene (include/rt_mi355x.h) and compares whole records."""
import numpy as np
import pytest

import surely_rt as rt
import weight_mirror_lib as W

PRESETS = ["cornell_box", "cornell_smoke", "final_scene", "quads", "simple_light", "two_spheres",
           "two_perlin_spheres", "random_balls", "three_spheres", "earth"]


def _f64(slots, i):
    return slots[i:i + 1].view(np.float64)[0]


def _put_d(rec, k, d):  # payload double k of a record: words 4 + 2k, 5 + 2k
    rec[4 + 2 * k:6 + 2 * k] = np.array([d], np.float64).view(np.uint32)


def _needs_uv(texs, t, depth=0):
    if depth > 64:
        return False
    kind = int(texs[t, 0])
    if kind == W.IMAGE:
        return int(texs[t, 1]) > 0 and int(texs[t, 2]) > 0
    if kind == W.CHECKER:
        return _needs_uv(texs, int(texs[t, 1]), depth + 1) or _needs_uv(texs, int(texs[t, 2]), depth + 1)
    return False


def _expected(blob):
    """The two tables without mirrors, the mirror words (None where there is none) and the flag,
    from the blob alone."""
    s = blob.slots
    n_tex, tex_off, n_mat, mat_off = (int(s[k]) for k in (3, 4, 5, 6))
    texs = np.zeros((n_tex, W.TEX_WORDS), np.uint32)
    tex_mirror = {}
    for t in range(n_tex):
        b = tex_off + t * W.TEX_SLOTS
        kind = int(s[b])
        texs[t, 0] = kind
        if kind == W.SOLID:
            col = [_f64(s, b + 1 + k) for k in range(3)]
            for k in range(3):
                _put_d(texs[t], k, col[k])
            tex_mirror[t] = col
        elif kind == W.CHECKER:
            _put_d(texs[t], 0, _f64(s, b + 1))
            texs[t, 1], texs[t, 2] = int(s[b + 2]), int(s[b + 3])
        elif kind == W.IMAGE:
            texs[t, 1], texs[t, 2], texs[t, 3] = int(s[b + 1]), int(s[b + 2]), int(s[b + 3])
        else:
            assert kind == W.NOISE
            _put_d(texs[t], 0, _f64(s, b + 1))
            texs[t, 1] = int(s[b + 2])
    mats = np.zeros((n_mat, W.MAT_WORDS), np.uint32)
    mat_mirror, solid = {}, {}
    for m in range(n_mat):
        b = mat_off + m * W.MAT_SLOTS
        kind = int(s[b])
        if kind in (W.LAMBERTIAN, W.DIFFUSE_LIGHT, W.ISOTROPIC):
            t = int(s[b + 1])
            mats[m, 0] = kind | (W.MATF_NEEDS_UV if _needs_uv(texs, t) else 0)
            mats[m, 1] = t
            solid[m] = int(texs[t, 0]) == W.SOLID
            mat_mirror[m] = tex_mirror[t] if solid[m] else None
        elif kind == W.METAL:
            mats[m, 0] = kind
            for k in range(4):
                _put_d(mats[m], k, _f64(s, b + 1 + k))
            solid[m], mat_mirror[m] = False, [_f64(s, b + 1 + k) for k in range(3)]
        else:
            assert kind == W.DIELECTRIC
            mats[m, 0] = kind
            ir = _f64(s, b + 1)
            _put_d(mats[m], 3, ir)
            for k in range(3):
                _put_d(mats[m], k, _f64(s, b + 2 + k))
            with np.errstate(all="ignore"):
                inv = np.float64(1.0) / ir
                rf, rb = (1.0 - inv) / (1.0 + inv), (1.0 - ir) / (1.0 + ir)
            _put_d(mats[m], 4, inv), _put_d(mats[m], 5, rf * rf), _put_d(mats[m], 6, rb * rb)
            solid[m], mat_mirror[m] = False, [_f64(s, b + 2 + k) for k in range(3)]
    return mats, texs, mat_mirror, tex_mirror, solid


def _check(blob):
    mats, texs = W.flat_tables(blob)
    e_mats, e_texs, mat_mirror, tex_mirror, solid = _expected(blob)
    assert mats.shape == e_mats.shape and texs.shape == e_texs.shape
    seen = set()
    for t in range(len(texs)):
        rec = texs[t].copy()
        if t in tex_mirror:
            assert rec[1:4].tolist() == W.f32_bits(tex_mirror[t]).tolist(), (t, tex_mirror[t])
            rec[1:4] = 0
        assert np.array_equal(rec, e_texs[t]), ("texture", t)
    for m in range(len(mats)):
        rec = mats[m].copy()
        assert bool(rec[0] & W.MATF_SOLID_W) == solid[m], ("flag", m)
        rec[0] &= ~np.uint32(W.MATF_SOLID_W)
        words = [2, 3, W.MAT_WZ]
        if mat_mirror[m] is None:  # checker / noise / image: no mirror, the words stay zero
            assert rec[words].tolist() == [0, 0, 0], m
            seen.add("textured")
        else:
            assert rec[words].tolist() == W.f32_bits(mat_mirror[m]).tolist(), (m, mat_mirror[m])
            rec[words] = 0
            seen.add(int(rec[0]) & 0xff)
        assert np.array_equal(rec, e_mats[m]), ("material", m)
    return seen


@pytest.mark.parametrize("name", PRESETS)
def test_preset_mirrors_are_the_f32_of_their_fields(name):
    blob, _ = rt.preset_blob(name, width=32, spp=4)
    _check(blob)


def test_every_material_kind_and_the_edge_values():
    """Each kind over solid, checker and noise textures; the colours run through the edge values:
    f32 subnormals, overflow to inf, NaN, -0.0 and the ties of round-to-nearest-even."""
    blob = W.every_kind_scene()
    seen = _check(blob)
    assert seen == {"textured", W.LAMBERTIAN, W.METAL, W.DIELECTRIC, W.DIFFUSE_LIGHT, W.ISOTROPIC}
    mats, texs = W.flat_tables(blob)
    kinds = {(int(r[0]) & 0xff, bool(r[0] & W.MATF_SOLID_W)) for r in mats}
    for k in (W.LAMBERTIAN, W.DIFFUSE_LIGHT, W.ISOTROPIC):
        assert (k, True) in kinds and (k, False) in kinds
    mirrored = np.concatenate([texs[texs[:, 0] == W.SOLID][:, 1:4].ravel(),
                               mats[:, [2, 3, W.MAT_WZ]].ravel()]).astype(np.uint32)
    f = mirrored.view(np.float32)
    assert np.isnan(f).any() and np.isposinf(f).any() and (mirrored == 0x80000000).any()
    assert ((mirrored & 0x7f800000) == 0).any() and (mirrored & 0x7fffffff != 0).any()  # subnormal
    sub = mirrored[((mirrored & 0x7f800000) == 0) & ((mirrored & 0x7fffffff) != 0)]
    assert sub.size > 0


def test_edge_values_round_as_documented():
    """The host cast the flattener uses, on the edge list: what each class of value becomes."""
    b = W.f32_bits(W.EDGE)
    e = dict(zip(W.EDGE.tolist(), b.tolist()))
    assert e[1e-40] == 71362 and e[2.0 ** -149] == 1            # subnormals kept
    assert e[2.0 ** -150] == 0 and e[2.0 ** -151] == 0          # tie to even (0), below: 0
    assert e[float(np.nextafter(2.0 ** -150, 1.0))] == 1        # just above the tie: up
    assert e[1.0 + 2.0 ** -24] == 0x3f800000                    # tie to even
    assert e[float(np.nextafter(1.0 + 2.0 ** -24, 2.0))] == 0x3f800001
    assert e[1.0 + 3 * 2.0 ** -24] == 0x3f800002                # tie to even, upwards
    assert e[W.F32_OVF] == 0x7f800000        # the first double that overflows
    assert e[float(np.nextafter(W.F32_OVF, 0.0))] == 0x7f7fffff
    assert b[1] == 0x80000000                                   # EDGE[1] is -0.0
    assert (b[-1] & 0x7f800000) == 0x7f800000 and (b[-1] & 0x007fffff) != 0  # NaN stays NaN
