"""rt_temporal_* restated in f64 numpy from the definition in include/rt_mi355x.h: the only
reference of the temporal tests. The guides are formed in f32 as the device forms them (they are
stored and compared, so they must be the same numbers); everything after them is f64.

Besides the outputs every call returns a *fragile* mask: the pixels at which a rounding difference
between f32 and f64 could flip a decision, so that kernel and reference may legitimately differ by
more than rounding. A pixel is fragile when, for one of its in-frame taps, an enabled tap test
(normal, depth) has its two sides within 1e-5 relative of each other; when Wsum is within 1e-5 of
min_weight; when s is within 1e-5 of 0 relative to the pixel's own ray parameter z; or when it
takes an accepted tap of weight > 1e-6 from a pixel that was fragile in the previous call. The
tests leave fragile pixels out and bound their share (<= 1 %). Test infrastructure."""
import numpy as np

import surely_rt as rt

EPS = 1e-5
TAP_EPS = 1e-6
FRAGILE_SHARE = 0.01


def camera_matrix(cam):
    """(center, M) with M = [pixel00_loc - center | pixel_delta_u | pixel_delta_v] as columns."""
    c = np.array(cam.center[:], np.float64)
    m = np.stack([np.array(cam.pixel00_loc[:], np.float64) - c,
                  np.array(cam.pixel_delta_u[:], np.float64),
                  np.array(cam.pixel_delta_v[:], np.float64)], axis=1)
    return c, m


def adjugate_inverse(m):
    """adjugate over determinant, f64"""
    c = np.empty((3, 3))
    for r in range(3):
        for k in range(3):
            r1, r2, k1, k2 = (r + 1) % 3, (r + 2) % 3, (k + 1) % 3, (k + 2) % 3
            c[r, k] = m[r1, k1] * m[r2, k2] - m[r1, k2] * m[r2, k1]  # cofactor (cyclic: signed)
    det = float(m[0] @ c[0])
    assert np.isfinite(det) and det != 0.0
    return c.T / det


def project(cam, xyz):
    """(s, x', y') of world points (..., 3) in `cam`"""
    c, m = camera_matrix(cam)
    v = (np.asarray(xyz, np.float64) - c) @ adjugate_inverse(m).T
    with np.errstate(all="ignore"):
        return v[..., 0], v[..., 1] / v[..., 0], v[..., 2] / v[..., 0]


def guides(aov, H, W):
    """(n (H, W, 3), z, id, hits) as f32 arrays, formed in f32 as the device forms them"""
    g = np.asarray(aov, np.float32).reshape(H, W, rt.AOV_CHANNELS)
    hits = g[..., rt.AOV_HITS]
    hit = hits > 0
    with np.errstate(all="ignore"):
        d = np.where(hit, hits, np.float32(1))
        n = np.where(hit[..., None], g[..., rt.AOV_NORMAL:rt.AOV_NORMAL + 3] / d[..., None],
                     np.float32(0)).astype(np.float32)
        z = np.where(hit, g[..., rt.AOV_T] / d, np.float32(0)).astype(np.float32)
    return n, z, g[..., rt.AOV_MATID].copy(), hits


def _close(a, b):
    return np.abs(a - b) <= EPS * np.maximum(np.abs(a), np.abs(b))


class TemporalRef:
    """One rt_temporal handle. accumulate() returns a dict: beauty, m2 (None without m2: what
    out_m2 receives, VARIANCE_OF_MEAN applied), hist_len, copied (bool: the outputs are bitwise
    copies of the inputs: L <= 1 without a usable history), fragile (bool)."""

    def __init__(self):
        self.h = None
        self.frames = 0

    def info(self):
        if self.h is None:
            return dict(frames=0, width=0, height=0, moments=False)
        H, W = self.h["L"].shape
        return dict(frames=self.frames, width=W, height=H, moments=self.h["moments"])

    def accumulate(self, cam, beauty, aov, p, m2=None):
        H, W = p.height, p.width
        assert (cam.image_height, cam.image_width) == (H, W)
        S = np.asarray(beauty, np.float32).reshape(H, W, 3).astype(np.float64)
        Q = None if m2 is None else np.asarray(m2, np.float32).reshape(H, W, 3).astype(np.float64)
        n32, z32, mid, hits = guides(aov, H, W)
        n, z = n32.astype(np.float64), z32.astype(np.float64)
        valid = np.isfinite(S).all(-1)
        if Q is not None:
            valid &= np.isfinite(Q).all(-1)
        max_history, min_weight = float(p.max_history), float(p.min_weight)
        depth_tol, normal_tol = float(p.depth_tol), float(p.normal_tol)
        h = self.h
        if p.flags & rt.RT_TEMPORAL_RESET or (h is not None and h["L"].shape != (H, W)):
            h = None
        if h is not None:
            assert h["moments"] == (Q is not None), "RT_ERR_INVALID_ARG: moments mismatch"
        out_S, out_Q = S.copy(), None if Q is None else Q.copy()
        L = np.where(valid, 1.0, 0.0)
        usable = np.zeros((H, W), bool)
        fragile = np.zeros((H, W), bool)
        center, M = camera_matrix(cam)
        if h is not None:
            jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                                 indexing="ij")
            D = (np.array(cam.pixel00_loc[:]) + ii[..., None] * np.array(cam.pixel_delta_u[:]) +
                 jj[..., None] * np.array(cam.pixel_delta_v[:]) - center)
            X = center + z[..., None] * D
            with np.errstate(all="ignore"):
                v = (X - h["center"]) @ h["minv"].T
                s, xp, yp = v[..., 0], v[..., 1] / v[..., 0], v[..., 2] / v[..., 0]
                cand = (valid & (hits > 0) & np.isfinite(s) & np.isfinite(xp) & np.isfinite(yp) &
                        (s > 0))
                fragile |= valid & (hits > 0) & (np.abs(s) <= EPS * np.abs(z))
                xs, ys = np.where(cand, xp, 0.0), np.where(cand, yp, 0.0)
                i0, j0 = np.floor(xs), np.floor(ys)
                fx, fy = xs - i0, ys - j0
                ws = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
                Wsum = np.zeros((H, W))
                aS, aQ, aL = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W))
                for t, w in enumerate(ws):
                    w = w.astype(np.float32).astype(np.float64)
                    qi, qj = i0 + (t & 1), j0 + (t >> 1)
                    inside = cand & (qi >= 0) & (qi < W) & (qj >= 0) & (qj < H)
                    ci = np.clip(qi, 0, W - 1).astype(np.int64)
                    cj = np.clip(qj, 0, H - 1).astype(np.int64)
                    ok = inside & (h["L"][cj, ci] >= 1) & (h["z"][cj, ci] > 0) & \
                        (h["id"][cj, ci] == mid)
                    if normal_tol > 0:
                        dn = ((h["n"][cj, ci] - n) ** 2).sum(-1)
                        ok &= dn <= normal_tol * normal_tol
                        fragile |= inside & _close(dn, np.float64(normal_tol * normal_tol))
                    if depth_tol > 0:
                        dz = np.abs(h["z"][cj, ci] - s)
                        ok &= dz <= depth_tol * s
                        fragile |= inside & _close(dz, depth_tol * s)
                    fragile |= ok & (w > TAP_EPS) & h["fragile"][cj, ci]
                    wk = np.where(ok, w, 0.0)
                    Wsum += wk
                    # a rejected tap's record may hold NaN: select, never multiply by 0
                    aS += np.where(ok[..., None], w[..., None] * h["S"][cj, ci], 0.0)
                    aL += np.where(ok, w * h["L"][cj, ci], 0.0)
                    if Q is not None:
                        aQ += np.where(ok[..., None], w[..., None] * h["Q"][cj, ci], 0.0)
                fragile |= cand & (np.abs(Wsum - min_weight) <= EPS)
                usable = cand & (Wsum > min_weight)
                d = np.where(usable, Wsum, 1.0)
                Lu = np.minimum(aL / d + 1.0, max_history)
                alpha = 1.0 / Lu
                L = np.where(usable, Lu, L)
                u3 = usable[..., None]
                out_S = np.where(u3, (1 - alpha[..., None]) * (aS / d[..., None]) +
                                 alpha[..., None] * S, S)
                if Q is not None:
                    out_Q = np.where(u3, (1 - alpha[..., None]) * (aQ / d[..., None]) +
                                     alpha[..., None] * Q, Q)
        user_Q = out_Q
        if Q is not None and p.flags & rt.RT_TEMPORAL_VARIANCE_OF_MEAN:
            rows = float(p.beauty_rows)
            with np.errstate(all="ignore"):
                m = out_S * out_S / rows
                vom = m + np.maximum(0.0, out_Q - m) / np.where(usable, L, 1.0)[..., None]
            user_Q = np.where(usable[..., None], vom, out_Q)
        self.frames = self.frames + 1 if h is not None else 1
        self.h = dict(S=out_S, Q=out_Q, L=L, n=n, z=z, id=mid, fragile=fragile, center=center,
                      minv=adjugate_inverse(M), moments=Q is not None)
        return dict(beauty=out_S, m2=user_Q, hist_len=L, copied=~usable, fragile=fragile)


def error(got, ref, scale, keep):
    """The project's measure (denoise_ref.mean_error) over the pixels `keep`: the max of
    |got - ref| / max(1, |ref|) on got / scale and ref / scale, non-finite positions (which must
    coincide) left out."""
    got = np.asarray(got, np.float64)[keep] / scale
    ref = np.asarray(ref, np.float64)[keep] / scale
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)), "non-finite pixels differ from the reference"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
