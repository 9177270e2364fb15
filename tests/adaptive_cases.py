"""Shared by the tile-render and adaptive GPU tests: the scenes of the moments tests on one device
scene each, with helpers that run an entry point over fresh device buffers. Test infrastructure."""
import numpy as np

import surely_rt as rt
from hip_buf import DevBuf

CASES = {
    # 20 x 12: 3 x 2 tiles with a 4-wide right column and a 4-high bottom row; the non-BVH
    # scene-specialised kernel with the deferred light PDF
    "cornell16": ("cornell_box", dict(width=20, spp=16, depth=8, aspect=20 / 12), 0),
    "cornell64": ("cornell_box", dict(width=20, spp=64, depth=8, aspect=20 / 12), 0),
    # the BVH kernels through the interpreter walker: no hiprtc compile
    "final16": ("final_scene", dict(width=16, spp=16, depth=8), rt.RT_FLAG_INTERPRETER),
}
SENTINEL = np.uint32(0x7FC12345)  # a NaN payload: an untouched pixel keeps exactly these bits


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Case:
    def __init__(self, name, spec=None):
        scene, kw, self.flags = spec or CASES[name]  # spec: a case of the caller's own
        self.blob, self.cam = rt.preset_blob(scene, **kw)
        self.ds = rt.DeviceScene(self.blob)
        self.H, self.W, self.S = self.cam.image_height, self.cam.image_width, self.cam.sqrt_spp
        self.tx, self.ty = rt.tile_grid(self.W, self.H)
        self.n_tiles = self.tx * self.ty
        self.shape = (self.H, self.W, 3)
        self._cache = {}

    def opts(self, overwrite=True, **kw):
        f = self.flags | (rt.RT_FLAG_OVERWRITE if overwrite else 0)
        return rt.make_opts(self.cam, seed=1, flags=f, **kw)

    def mask(self, tiles):
        """(H, W) bool: the pixels of the listed tiles"""
        m = np.zeros((self.H, self.W), bool)
        for t in tiles:
            x0, y0 = (int(t) % self.tx) * 8, (int(t) // self.tx) * 8
            m[y0:y0 + 8, x0:x0 + 8] = True
        return m

    def plain(self, o, init=None):
        b = DevBuf(self.shape, init=init)
        try:
            self.ds.render_device(self.cam, o, b.ptr)
            return b.download()
        finally:
            b.free()

    def moments(self, o, init=None, init2=None):
        b, q = DevBuf(self.shape, init=init), DevBuf(self.shape, init=init2)
        try:
            self.ds.render_moments_device(self.cam, o, b.ptr, q.ptr)
            return b.download(), q.download()
        finally:
            b.free()
            q.free()

    def full(self):
        """the whole frame's (accum, m2) of rt_render_moments_device, rendered once"""
        if "full" not in self._cache:
            self._cache["full"] = self.moments(self.opts())
        return self._cache["full"]

    def row(self, r):
        """rt_render_device of stratum row r alone, rendered once"""
        if ("row", r) not in self._cache:
            self._cache["row", r] = self.plain(self.opts(sj_begin=r, sj_count=1))
        return self._cache["row", r]

    def tiles(self, tiles, o, step=1, init=None, init2=None, m2=True, stats=False):
        """rt_render_tiles_device -> (accum, m2 or None[, stats])"""
        b = DevBuf(self.shape, init=init)
        q = DevBuf(self.shape, init=init2) if m2 else None
        try:
            st = self.ds.render_tiles_device(self.cam, o, tiles, step, b.ptr, q.ptr if m2 else 0,
                                             stats=stats)
            res = (b.download(), q.download() if m2 else None)
            return res + (st,) if stats else res
        finally:
            b.free()
            if q:
                q.free()


def sentinel(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)
