"""The variance-guided a-trous denoiser of include/rt_mi355x.h (rt_denoise_var*) restated in f64
numpy: the only reference of test_moments_host.py and test_denoise_var_gpu.py. The structure of
denoise_ref.denoise_ref with the per-pixel variance, its 3x3 prefilter, the variance-normalised
colour term and the propagation v' = sum w^2 v / (sum w)^2. Test infrastructure only."""
import numpy as np

import surely_rt as rt
from denoise_ref import H_TAPS, _span

G_TAPS = (0.25, 0.5, 0.25)


def denoise_var_ref(beauty, m2, aov, p):
    """beauty, m2 (H, W, 3) raw sums over p.beauty_rows stratum rows, aov (H, W, 12) raw AOV sums,
    p an RtDenoiseVarParams. Returns (out f64 (H, W, 3) in the scale of the beauty sums, var_out
    f64 (H, W), valid bool (H, W)); an invalid pixel's out is its beauty sum and its var_out 0."""
    H, W = p.height, p.width
    bty = np.asarray(beauty, np.float32).reshape(H, W, 3).astype(np.float64)
    Q = np.asarray(m2, np.float32).reshape(H, W, 3).astype(np.float64)
    g = np.asarray(aov, np.float32).reshape(H, W, rt.AOV_CHANNELS).astype(np.float64)
    B, A, n = float(p.beauty_samples), float(p.aov_samples), float(p.beauty_rows)
    demod = bool(p.flags & rt.DENOISE_DEMODULATE)
    with np.errstate(all="ignore"):
        c = bty / B
        hits = g[..., rt.AOV_HITS]
        hit = hits > 0
        safe = np.where(hit, hits, 1.0)
        nrm = np.where(hit[..., None], g[..., rt.AOV_NORMAL:rt.AOV_NORMAL + 3] / safe[..., None],
                       0.0)
        z = np.where(hit, g[..., rt.AOV_T] / safe, 0.0)
        a = g[..., rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] / A
        e = g[..., rt.AOV_EMISSION:rt.AOV_EMISSION + 3] / A
        m = np.maximum(a, 1e-3)
        x0 = (c - e) / m if demod else c
        var = np.maximum(0.0, np.nan_to_num(Q - bty * bty / n, nan=0.0)) * n / ((n - 1.0) * B * B)
        v_raw = (var / (m * m) if demod else var).sum(-1).astype(np.float32).astype(np.float64)
        valid = np.isfinite(x0).all(-1) & np.isfinite(Q).all(-1) & np.isfinite(v_raw)
        x = np.where(valid[..., None], x0, 0.0)
        v_raw = np.where(valid, v_raw, 0.0)
        # the 3x3 prefilter over the valid in-frame neighbours
        num = np.zeros((H, W))
        den = np.zeros((H, W))
        for j in range(-1, 2):
            ys = _span(H, j)
            if ys is None:
                continue
            for i in range(-1, 2):
                xs = _span(W, i)
                if xs is None:
                    continue
                Pp, Qq = (ys[0], xs[0]), (ys[1], xs[1])
                w = np.where(valid[Qq], G_TAPS[i + 1] * G_TAPS[j + 1], 0.0)
                num[Pp] += w * v_raw[Qq]
                den[Pp] += w
        v = np.where(valid, num / den, 0.0)
        sig = [float(s) for s in (p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo)]
        for k in range(p.levels):
            s = 1 << k
            num = np.zeros((H, W, 3))
            den = np.zeros((H, W))
            numv = np.zeros((H, W))
            for j in range(-2, 3):
                ys = _span(H, s * j)
                if ys is None:
                    continue
                for i in range(-2, 3):
                    xs = _span(W, s * i)
                    if xs is None:
                        continue
                    Pp, Qq = (ys[0], xs[0]), (ys[1], xs[1])
                    E = np.zeros(den[Pp].shape)
                    if sig[0] > 0:
                        E = E + ((x[Pp] - x[Qq]) ** 2).sum(-1) / (sig[0] ** 2 *
                                                                  (v[Pp] + v[Qq] + 1e-10))
                    if sig[1] > 0:
                        E = E + ((nrm[Pp] - nrm[Qq]) ** 2).sum(-1) / sig[1] ** 2
                    if sig[3] > 0:
                        E = E + ((a[Pp] - a[Qq]) ** 2).sum(-1) / sig[3] ** 2
                    if sig[2] > 0:
                        zz = np.maximum(np.maximum(z[Pp] ** 2, z[Qq] ** 2), 1e-30)
                        E = E + (z[Pp] - z[Qq]) ** 2 / (sig[2] ** 2 * zz)
                    w = H_TAPS[i + 2] * H_TAPS[j + 2] * np.exp(-E)
                    w = np.where(valid[Qq], w, 0.0)
                    num[Pp] += w[..., None] * x[Qq]
                    numv[Pp] += w * w * v[Qq]
                    den[Pp] += w
            x = np.where(valid[..., None], num / den[..., None], 0.0)
            v = np.where(valid, numv / (den * den), 0.0)
        y = x * m + e if demod else x
        out = np.where(valid[..., None], y * B, bty)
    return out, v, valid


def var_error(got, ref):
    """max |got - ref| / max(1, |ref|) of the variance output (mean_error's form)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if got.size else 0.0


def moments_from_rows(rows):
    """rows (n, H, W, 3) f64 row totals -> (S, Q) float32 as rt_render_moments would give them."""
    rows = np.asarray(rows, np.float64)
    return rows.sum(0).astype(np.float32), (rows * rows).sum(0).astype(np.float32)
