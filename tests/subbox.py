"""A W x H x D box in the corner of larger device containers (Wc > W, Hc > H, Dc > D) whose every float outside the box, the pitch
padding included, holds a chosen fill: NaN, or finite values that change the answer of any kernel that reads them.  Outputs start as
a byte sentinel everywhere, so a write outside the box shows as well."""
import numpy as np

SENTINEL_BYTE = 0x7F
SENTINEL_BITS = 0x7F7F7F7F        # 3.39e38


def poison(rng, shape, kind):
    """a host array to fill a container with: "nan", or "finite" (mostly +-(1e4 .. 1.1e4), some exact zeros, so both a larger and
    a smaller value than anything in the box lie next to it)"""
    if kind == "nan":
        return np.full(shape, np.nan, np.float32)
    mag = rng.uniform(1e4, 1.1e4, size=shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return np.where(rng.random(shape) < 0.1, 0.0, sign * mag).astype(np.float32)


class SubBox:
    def __init__(self, f3d, cdims):
        self.f3d = f3d
        self.cdims = cdims
        self.c = f3d.Containers(*cdims)
        self.c.alloc()                                 # fixes the pitch
        self.P = self.c.pitch // 4
        wc, hc, dc = cdims
        self.full = (dc, hc, self.P)                   # the whole allocation as a [plane, row, float] array
        self.c.set_current()

    def put(self, box, fill):
        """a container holding `fill` (a full-shape array) with `box` [d, h, w] in its corner"""
        p = self.c.alloc()
        full = np.array(fill, np.float32)
        d, h, w = box.shape
        full[:d, :h, :w] = box
        self.c.upload(p, full)
        return p

    def sentinel(self):
        return self.c.alloc(fill=SENTINEL_BYTE)

    def get(self, p):
        """the whole allocation [Dc, Hc, P]"""
        self.f3d.sync()
        return self.c.download(p, (self.P, self.cdims[1], self.cdims[2]))

    def set_current(self):
        self.c.set_current()

    def free(self):
        self.f3d.sync()
        self.c.free()


def outside(full, dims):
    """boolean mask of the floats of a [Dc, Hc, P] array that lie outside the W x H x D corner box"""
    w, h, d = dims
    m = np.ones(full.shape, bool)
    m[:d, :h, :w] = False
    return m
