"""The edge-avoiding a-trous denoiser of include/rt_mi355x.h restated in f64 numpy: the only
reference of test_denoise_host.py and test_denoise_gpu.py (the device computes the same formulas
in f32). Vectorised over the 25 shifted slices of each level, taps in the header's order (j outer,
i inner). Test infrastructure only."""
import numpy as np

import surely_rt as rt

H_TAPS = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def _span(n, d):
    """Slices (p, q) of an axis of length n with q = p + d inside it, or None."""
    lo, hi = max(0, -d), n - max(0, d)
    if lo >= hi:
        return None
    return slice(lo, hi), slice(lo + d, hi + d)


def denoise_ref(beauty, aov, p):
    """beauty (H, W, 3) raw sums, aov (H, W, 12) raw AOV sums, p an RtDenoiseParams (its f32
    sigmas are read as the f32 values they are). Returns (out f64 (H, W, 3) in the scale of the
    beauty sums, valid bool (H, W)); an invalid pixel's out is its beauty sum."""
    H, W = p.height, p.width
    b32 = np.asarray(beauty, np.float32).reshape(H, W, 3)
    bty = b32.astype(np.float64)
    g = np.asarray(aov, np.float32).reshape(H, W, rt.AOV_CHANNELS).astype(np.float64)
    B, A = float(p.beauty_samples), float(p.aov_samples)
    demod = bool(p.flags & rt.DENOISE_DEMODULATE)
    with np.errstate(all="ignore"):
        c = bty / B
        hits = g[..., rt.AOV_HITS]
        hit = hits > 0
        safe = np.where(hit, hits, 1.0)
        n = np.where(hit[..., None], g[..., rt.AOV_NORMAL:rt.AOV_NORMAL + 3] / safe[..., None], 0.0)
        z = np.where(hit, g[..., rt.AOV_T] / safe, 0.0)
        a = g[..., rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] / A
        e = g[..., rt.AOV_EMISSION:rt.AOV_EMISSION + 3] / A
        m = np.maximum(a, 1e-3)
        x0 = (c - e) / m if demod else c
        valid = np.isfinite(x0).all(axis=-1)
        x = np.where(valid[..., None], x0, 0.0)
        sig = [float(s) for s in (p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo)]
        for k in range(p.levels):
            s = 1 << k
            num = np.zeros((H, W, 3))
            den = np.zeros((H, W))
            for j in range(-2, 3):
                ys = _span(H, s * j)
                if ys is None:
                    continue
                for i in range(-2, 3):
                    xs = _span(W, s * i)
                    if xs is None:
                        continue
                    P, Q = (ys[0], xs[0]), (ys[1], xs[1])
                    E = np.zeros(den[P].shape)
                    if sig[0] > 0:
                        E = E + ((x[P] - x[Q]) ** 2).sum(-1) / (sig[0] * 2.0 ** -k) ** 2
                    if sig[1] > 0:
                        E = E + ((n[P] - n[Q]) ** 2).sum(-1) / sig[1] ** 2
                    if sig[3] > 0:
                        E = E + ((a[P] - a[Q]) ** 2).sum(-1) / sig[3] ** 2
                    if sig[2] > 0:
                        zz = np.maximum(np.maximum(z[P] ** 2, z[Q] ** 2), 1e-30)
                        E = E + (z[P] - z[Q]) ** 2 / (sig[2] ** 2 * zz)
                    w = H_TAPS[i + 2] * H_TAPS[j + 2] * np.exp(-E)
                    w = np.where(valid[Q], w, 0.0)  # an invalid pixel is no one's neighbour
                    num[P] += w[..., None] * x[Q]
                    den[P] += w
            x = np.where(valid[..., None], num / den[..., None], 0.0)
        y = x * m + e if demod else x
        out = np.where(valid[..., None], y * B, bty)
    return out, valid


def mean_error(got, ref, p):
    """max over the frame of |got - ref| / max(1, |ref|) on the MEAN radiance (sums / B), NaN or
    inf positions (which must coincide) left out."""
    B = float(p.beauty_samples)
    got = np.asarray(got, np.float64) / B
    ref = np.asarray(ref, np.float64) / B
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)), "non-finite pixels differ from the reference"
    if not fin.any():
        return 0.0
    d = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    return float(d.max())


def clipped_rmse(mean, truth):
    """RMSE of the mean radiance clipped to [0, 1] (NaN counts as 0)."""
    a = np.clip(np.nan_to_num(np.asarray(mean, np.float64), nan=0.0, posinf=1.0, neginf=0.0), 0, 1)
    t = np.clip(np.asarray(truth, np.float64), 0, 1)
    return float(np.sqrt(np.mean((a - t) ** 2)))
