"""Synthetic frame sequences for the temporal-accumulation tests, host and GPU: the AOVs are
computed analytically per camera from a fronto-parallel plane with a nearer rectangle of another
material id in front of it, so that consecutive frames are geometrically consistent (the same
world point has the same depth and id whichever camera sees it); beauty and m2 are seeded random.
Between frames the camera makes a small lateral step and a small rth_camera_orbit_y turn. Test
infrastructure."""
import numpy as np

import surely_rt as rt

# frame sizes (H, W): one pixel; smaller than a 32x8 tile both ways; one column / one row more than
# a tile's multiple; whole tiles; a bottom row of tiles cut at 5 of 8 rows
SIZES = [(1, 1), (3, 5), (17, 33), (33, 17), (64, 64), (61, 64)]
FRAMES = 3
SPP = 4.0      # what the synthetic sums hold: B of the error measure
ROWS = 2       # stratum rows of the synthetic moments: n of the estimator
PLANE_Z, PLANE_X, PLANE_Y, PLANE_ID = -10.0, (-7.0, 7.5), (-5.0, 5.5), 3.0
RECT_Z, RECT_X, RECT_Y, RECT_ID = -6.0, (-1.5, 1.0), (-1.0, 1.2), 5.0
PIVOT = (0.0, 0.0, -8.0)
STEP, TURN = 0.07, 0.4  # world units and degrees per frame
# name -> (m2 given, VARIANCE_OF_MEAN, params). VARIANCE_OF_MEAN without m2 is an argument error, so
# the fourth variant is one with tolerances at which the edge taps between the two surfaces are
# decided by the depth test and the weight floor too, not by the id alone
VARIANTS = {"plain": (False, False, {}), "m2": (True, False, {}), "m2+vom": (True, True, {}),
            "m2+vom,tight": (True, True, dict(depth_tol=0.02, normal_tol=0.05, min_weight=0.3,
                                              max_history=2.0))}


def camera(H, W):
    """at the origin, looking down -z; the aspect is chosen so that the height comes out as H"""
    cam = rt.camera_new(W / (H + 0.5), W, int(SPP), 8, 60.0, (0, 0, 0), (0, 0, -1), (0, 1, 0), 0.0,
                        10.0, (0, 0, 0))
    assert (cam.image_height, cam.image_width) == (H, W)
    return cam


def shifted(cam, d):
    """`cam` translated by the world vector d"""
    c = cam.copy()
    for k in range(3):
        c.center[k] += d[k]
        c.pixel00_loc[k] += d[k]
    return c


def moved(cam, k):
    """the camera of frame k: k lateral steps and k turns"""
    return rt.camera_orbit_y(shifted(cam, (STEP * k, 0.01 * k, 0.0)), PIVOT, TURN * k)


def analytic_aov(cam, hits=SPP):
    """(H, W, 12) f32 AOV sums of `hits` identical samples through each pixel's centre"""
    H, W = cam.image_height, cam.image_width
    c = np.array(cam.center[:])
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                         indexing="ij")
    D = (np.array(cam.pixel00_loc[:]) + ii[..., None] * np.array(cam.pixel_delta_u[:]) +
         jj[..., None] * np.array(cam.pixel_delta_v[:]) - c)
    aov = np.zeros((H, W, rt.AOV_CHANNELS), np.float64)
    aov[..., rt.AOV_MATID] = -1.0
    done = np.zeros((H, W), bool)
    for z, xr, yr, mid in ((RECT_Z, RECT_X, RECT_Y, RECT_ID), (PLANE_Z, PLANE_X, PLANE_Y, PLANE_ID)):
        with np.errstate(all="ignore"):
            t = (z - c[2]) / D[..., 2]
        X = c + t[..., None] * D
        hit = (~done & np.isfinite(t) & (t > 1e-4) & (X[..., 0] >= xr[0]) & (X[..., 0] <= xr[1]) &
               (X[..., 1] >= yr[0]) & (X[..., 1] <= yr[1]))
        aov[hit, rt.AOV_HITS] = hits
        aov[hit, rt.AOV_T] = t[hit] * hits
        aov[hit, rt.AOV_NORMAL + 2] = hits  # (0, 0, 1) facing the camera
        aov[hit, rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] = 0.5 * hits
        aov[hit, rt.AOV_MATID] = mid
        done |= hit
    return aov.astype(np.float32)


class Sequence:
    """FRAMES frames of one size: cams, aov, beauty, m2 (lists)"""

    def __init__(self, H, W, frames=FRAMES, seed=None, static=False):
        rng = np.random.default_rng(1000 * H + W if seed is None else seed)
        base = camera(H, W)
        self.H, self.W = H, W
        self.cams = [base.copy() if static else moved(base, k) for k in range(frames)]
        self.aov = [analytic_aov(c) for c in self.cams]
        self.beauty = [(rng.random((H, W, 3)) * SPP).astype(np.float32) for _ in range(frames)]
        # Q >= S^2 / n, as real moments are
        self.m2 = [(b.astype(np.float64) ** 2 / ROWS * (1.0 + rng.random((H, W, 3))))
                   .astype(np.float32) for b in self.beauty]

    def params(self, m2=False, vom=False, **kw):
        p = rt.temporal_default_params(self.W, self.H)
        if vom:
            p.flags |= rt.RT_TEMPORAL_VARIANCE_OF_MEAN
        p.beauty_rows = ROWS if m2 else 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p


def sequences():
    return {f"{H}x{W}": Sequence(H, W) for H, W in SIZES}


# ------------------------------------------------------------------ the half-pixel ramp shift
RAMP_K = 2  # the shift is RAMP_K + 1/2 pixels


def ramp_shift(H=9, W=40):
    """Two frames over a plane that fills the view: frame 0's colour is a linear ramp in the
    column, a * i + b per channel; frame 1 (constant colour c) is seen by a camera moved sideways
    so that pixel (i, j) sees what frame 0 had at (i + RAMP_K + 1/2, j). Returns (cams, aovs,
    beauties, expect, full): expect (H, W, 3) f64 = (ramp(i + K + 1/2) + c) / 2 where all of the
    footprint lies in the frame (`full`, bool (H, W))."""
    cam0 = camera(H, W)
    t = PLANE_Z / (cam0.pixel00_loc[2] - cam0.center[2])  # the plane's ray parameter, every pixel
    dx = (RAMP_K + 0.5) * t * cam0.pixel_delta_u[0]
    cams = [cam0, shifted(cam0, (dx, 0.0, 0.0))]
    aovs = []
    for c in cams:  # a plane without bounds: every pixel hits at t
        a = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
        a[..., rt.AOV_HITS] = SPP
        a[..., rt.AOV_T] = np.float32(t * SPP)
        a[..., rt.AOV_NORMAL + 2] = SPP
        a[..., rt.AOV_MATID] = PLANE_ID
        aovs.append(a)
    i = np.arange(W, dtype=np.float64)
    slope, off, const = np.array([0.0625, 0.03125, 0.125]), np.array([0.5, 1.0, 0.25]), \
        np.array([1.0, 2.0, 3.0])
    ramp = lambda x: x[..., None] * slope + off  # noqa: E731  (exact in f32: dyadic values)
    b0 = np.broadcast_to(ramp(i), (H, W, 3)).astype(np.float32)
    b1 = np.broadcast_to(const, (H, W, 3)).astype(np.float32)
    expect = np.broadcast_to(0.5 * ramp(i + RAMP_K + 0.5) + 0.5 * const, (H, W, 3))
    full = np.broadcast_to(i + RAMP_K + 1 <= W - 1, (H, W))
    return cams, aovs, [b0, b1], expect, full
