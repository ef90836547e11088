"""A numpy model of jsnoop_batch_pack_coefs: from the coefficient arena of one image -- blocks [n][64] in decode order (MCU after MCU, the
components interleaved inside the MCU, natural order inside a block) -- a cumulative DC per block and the geometry to the tensor of one
component in every layout, element type and order.  Plain indexing, no cleverness: it is what the kernel is compared with, exactly.

Geometry: hv = [(H, V)] per scan component (a lone component: [(1, 1)]), mcu_x x mcu_y MCUs.  Component c has H x V blocks per MCU, V rows
of H blocks, behind the blocks of the components before it; its grid is bw = mcu_x * H by bh = mcu_y * V blocks."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Geometry:
    def __init__(self, hv, mcu_x, mcu_y):
        self.hv = [(int(h), int(v)) for h, v in hv]
        self.mcu_x, self.mcu_y = int(mcu_x), int(mcu_y)
        self.hmax = max(h for h, _ in self.hv); self.vmax = max(v for _, v in self.hv)
        self.bpm = sum(h * v for h, v in self.hv)
        self.ncomp = len(self.hv)
        self.nblocks = self.mcu_x * self.mcu_y * self.bpm

    def grid(self, c):
        h, v = self.hv[c]
        return self.mcu_x * h, self.mcu_y * v                      # (bw, bh)

    def comp_of_block(self):
        """Component of every block of the arena, decode order."""
        one = [c for c, (h, v) in enumerate(self.hv) for _ in range(h * v)]
        return np.tile(np.array(one), self.mcu_x * self.mcu_y)

    def arena_index(self, c):
        """[bh][bw]: the arena's block number of block (bx, by) of component c."""
        h, v = self.hv[c]; bw, bh = self.grid(c)
        first = sum(a * b for a, b in self.hv[:c])
        by, bx = np.mgrid[0:bh, 0:bw]
        return ((by // v) * self.mcu_x + bx // h) * self.bpm + first + (by % v) * h + bx % h


def geometry_of(parsed):
    """Geometry of a file from oracle.harness.parse_jpeg's record (the first scan is the frame's: all components, or the lone one)."""
    hv = [(h, v) for _id, h, v, _tq in parsed.comps] if len(parsed.comps) > 1 else [(1, 1)]
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    return Geometry(hv, -(-parsed.x // (8 * hmax)), -(-parsed.y // (8 * vmax)))


def cum_from_planes(planes, geo):
    """Per block (decode order) the cumulative DC read off the int16 planes of a DC-only decode: component c's block (bx, by) is the
    plane's sample (by * 8 * ev, bx * 8 * eh), ev = vmax / V, eh = hmax / H (the corner of the area the block is expanded to)."""
    cum = np.zeros(geo.nblocks, np.int16)
    for c in range(geo.ncomp):
        h, v = geo.hv[c]; bw, bh = geo.grid(c)
        g = planes[c][::8 * (geo.vmax // v), ::8 * (geo.hmax // h)][:bh, :bw]
        assert g.shape == (bh, bw), (g.shape, bh, bw)
        cum[geo.arena_index(c)] = g
    return cum


def running_dc(blocks, geo, rst_interval=0):
    """Per block (decode order) the int16-wrapping running sum of slot 0 over the blocks of its component, restarted every rst_interval MCUs."""
    comp = geo.comp_of_block(); cum = np.zeros(geo.nblocks, np.int16)
    per = (rst_interval or geo.mcu_x * geo.mcu_y) * geo.bpm
    for c in range(geo.ncomp):
        at = np.flatnonzero(comp == c); d = blocks[at, 0].astype(np.int64)
        s = np.cumsum(d); iv = at // per
        first = np.r_[True, iv[1:] != iv[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(len(at)), 0))
        run = s - (s - d)[start]
        cum[at] = (((run + 32768) & 0xFFFF) - 32768).astype(np.int16)
    return cum


def coef_tensor(blocks, cum, geo, c, layout="blocks", dtype=np.int16, zigzag=False):
    """Component c: [bh][bw][64] ("blocks") or [64][bh][bw] ("freq"); natural index 0 = cum, position z = natural ZIGZAG[z] with zigzag."""
    blocks = np.asarray(blocks); assert blocks.shape == (geo.nblocks, 64) and blocks.dtype == np.int16, (blocks.shape, blocks.dtype)
    idx = geo.arena_index(c)
    t = blocks[idx].copy()
    t[..., 0] = np.asarray(cum, np.int16)[idx]
    if zigzag:
        t = t[..., ZIGZAG]
    if layout == "freq":
        t = np.moveaxis(t, 2, 0)
    else:
        assert layout == "blocks", layout
    return np.ascontiguousarray(t.astype(dtype))
