"""The catalogue of baseline (SOF0) files behind tests/test_dc_scan_cases.py (CPU) and tests/test_gpu_dc_scan.py (GPU): the DC predictor
scan (k_dc_scan, k_dc_scan_parts; dc_scan_range in jpegsnoop_amd/csrc/jsnoop_kernels.hip) at its four seams -- the 64 lanes of a wave,
the 16 wave totals of a 1024-MCU step, the carry that links steps, the 64 part summaries of the two-level form -- and the restart marks.

Every block of every file is [(category, difference), (EOB)], written with tests/base_stream.py over one DC table (categories 0..11,
flat 4-bit codes: no all-ones code, so the pad bits in front of a marker spell none) and one AC table (EOB alone).  A file is all DC.

The MODEL (`model`) is the reference's arithmetic restated in numpy int64: per component one running sum of the dequantised differences
(int16)(diff * Q0), added modulo 2**16 (m_nDcLum += ... in int16), zeroed where the case says a restart lies.  Every case carries a
`check` that proves from the model and from the writer's census that the file holds what its name claims: a reset at exactly MCU m,
so many int16 wraps of the Y predictor, the number of parts and the MCUs of the last one (`parts_of`: the formula of k_dc_scan_parts
restated), the blocks per MCU.

Groups.  "A": MCU counts around the lane, wave and step seams, every layout (the 10- and the 48-block layouts run the generic instance
dc_scan_range<JS_MAX_BLK_PER_MCU>).  "B": the two-level form with parts of one step (up to 65536 MCUs).  "C": parts of two steps (above
65536 MCUs; `per` = 2048).  "D": no restart, every term +32752, so that the kernel's `int` sums pass 2**31, in the image and in the fold of the
part summaries (one file of 33 * 2048 + 1 MCUs, which is also group C's file without restarts).  "E": markers inside an MCU (marks greater than 1) and two markers at one MCU (bit 6 of the mark).
"""
from __future__ import annotations

import numpy as np

import base_stream as BS
import prog_codec as P

DC_THREADS = 1024            # MCUs per step (jsnoop_kernels.hip)
DC_PARTS_MAX = 64            # parts per image in the two-level form
DC_PARTS_IMAGES = 8          # JS_DC_PARTS_IMAGES (jsnoop_launch.h): batches of up to this many images take the two-level form
MAX_BLK_PER_MCU = 48         # JS_MAX_BLK_PER_MCU

DC_TAB = P.flat_table(list(range(12)), 4)        # category n: the 4-bit code n; 1100 .. 1111 are no codes
AC_TAB = ([1] + [0] * 15, [0x00])                # EOB: '0'
TABS = {(0, 0): DC_TAB, (1, 0): AC_TAB}

LAYOUTS = {                  # name: sampling factors per component
    "gray": [(1, 1)], "444": [(1, 1), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)],
    "luma4x2": [(4, 2), (1, 1), (1, 1)], "all4x4": [(4, 4), (4, 4), (4, 4)]}
BLOCKS = {"gray": 1, "444": 3, "422": 4, "420": 6, "luma4x2": 10, "all4x4": 48}
FAST_LAYOUTS = ("444", "422", "420")             # the layouts of this catalogue that the DC-only fast form takes (js_fast_layout)
QPAIRS = [(1, 37), (37, 255), (255, 4099), (4099, 1)]        # DC quantisers (luma, chroma); 4099 makes a 16-bit table: single products wrap


def parts_of(nmcu):
    """(per, parts, MCUs of the last part) of k_dc_scan_parts: `per` = whole steps per part, parts = those that hold an MCU."""
    per = -(-(-(-nmcu // DC_PARTS_MAX)) // DC_THREADS) * DC_THREADS
    parts = -(-nmcu // per)
    return per, parts, nmcu - (parts - 1) * per


def _grid(nmcu):
    """nmcu = mx * my with mx as near to its square root as its divisors allow (mx >= my)."""
    my = max(d for d in range(1, int(nmcu ** 0.5) + 1) if nmcu % d == 0)
    return nmcu // my, my


def frame_of(layout, nmcu, q):
    hv = LAYOUTS[layout]; mx, my = _grid(nmcu)
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    qt = lambda dc: [dc] + [1 + k // 4 for k in range(1, 64)]
    comps = [(h, v, min(c, 1)) for c, (h, v) in enumerate(hv)]
    fr = P.Frame(8 * hmax * mx, 8 * vmax * my, comps, {0: qt(q[0]), 1: qt(q[1])} if len(hv) == 3 else {0: qt(q[0])})
    assert fr.mcu_x * fr.mcu_y == nmcu and len(fr.mcu_blocks()) == BLOCKS[layout] and fr.mcu_x * 8 * hmax < 65536
    return fr


def model(case):
    """(per component: int16 cumulative DC of its blocks in decode order, int16 wraps of the Y predictor)."""
    bpm = case.frame.mcu_blocks(); nb = len(bpm)
    comp = np.tile(np.array([c for c, _v, _h in bpm]), case.nmcu)
    q0 = np.array([case.frame.qtabs[case.frame.comps[c][2]][0] for c in range(case.frame.ncomp)], np.int64)
    term = (case.diffs.astype(np.int64) * q0[comp]) & 0xFFFF
    term = np.where(term >= 32768, term - 65536, term)                     # (int16)(diff * Q0)
    seg = np.zeros(case.nmcu * nb, np.int64); seg[case.resets] = 1; seg = np.cumsum(seg)
    out = []; wraps = 0
    for c in range(case.frame.ncomp):
        at = np.flatnonzero(comp == c); t = term[at]; s = seg[at]
        cum = np.cumsum(t)
        first = np.r_[True, s[1:] != s[:-1]]                               # the component's first block behind a restart
        start = np.maximum.accumulate(np.where(first, np.arange(len(t)), 0))
        run = cum - (cum - t)[start]                                       # the sum since the last restart, not wrapped
        v = ((run + 32768) & 0xFFFF) - 32768                               # ... modulo 2**16: what int16 adds leave
        if c == 0:
            before = np.where(first, 0, np.r_[0, v[:-1]])
            wraps = int(((before + t > 32767) | (before + t < -32768)).sum())
        out.append(v.astype(np.int16))
    return out, wraps


def planes_corner(case, cum):
    """Per component the model's values where the int16 plane has the top-left sample of every block: (rows, columns, values)."""
    fr = case.frame; bpm = fr.mcu_blocks(); out = []
    mcu_h, mcu_w = 8 * fr.vmax, 8 * fr.hmax
    for c in range(fr.ncomp):
        h, v = fr.hv[c]
        val = cum[c].reshape(fr.mcu_y, fr.mcu_x, v, h)
        my, mx, cv, ch = np.meshgrid(np.arange(fr.mcu_y), np.arange(fr.mcu_x), np.arange(v), np.arange(h), indexing="ij")
        out.append(((my * mcu_h + cv * 8).ravel(), (mx * mcu_w + ch * 8).ravel(), val.ravel()))     # SetFullRes: corner = MCU + 8 * (cy, cx)
    return out


def first_block_difference(case, comp, got, exp):
    """Names the first block (decode order of the component) at which two value lists differ: its MCU and where that MCU lies relative
    to the seams of the scan -- lane (MCU % 64), place in the step (MCU % 1024), part (MCU // per)."""
    got = np.asarray(got); exp = np.asarray(exp)
    d = np.flatnonzero(got != exp)
    if not len(d):
        return None
    h, v = case.frame.hv[comp]; k = int(d[0]); m = k // (h * v)
    return ("%s: component %d: %d blocks differ; first is block %d of MCU %d (MCU %% 64 = %d, MCU %% 1024 = %d, MCU // per = %d of %d parts): got %d, expected %d"
            % (case.name, comp, len(d), k % (h * v), m, m % 64, m % 1024, m // case.per, case.parts, int(got[k]), int(exp[k])))


class Case:
    def __init__(self, name, group, layout, nmcu, dri, diffs, q, extra=(), claims=None):
        self.name, self.group, self.layout, self.nmcu, self.dri, self.q = name, group, layout, nmcu, dri, q
        self.frame = frame_of(layout, nmcu, q); nb = BLOCKS[layout]
        self.diffs = np.asarray(diffs, np.int64); assert len(self.diffs) == nmcu * nb
        self.extra = sorted(m * nb + j for m, j in extra)                  # markers besides the regular ones: in front of block j of MCU m
        regular = [u * nb for u in range(dri, nmcu, dri)] if dri else []
        self.resets = np.array(sorted(set(regular) | set(self.extra)), np.int64)
        self.markers = len(regular) + len(self.extra)
        cats = [abs(int(d)).bit_length() for d in self.diffs]
        blocks = [[(s, int(d)), (0x00, 0)] for s, d in zip(cats, self.diffs)]
        st = BS.write(self.frame, TABS, [(0, 0)] * self.frame.ncomp, blocks, dri, rst_before=self.extra)
        self.file = st.file; self.iv_ends = st.iv_ends; self.bits = st.bits
        # what the checks need of the census, then the census goes (two records per block: too much to keep for a million blocks)
        iv = np.array([r.iv for r in st.census if r.k == 0])
        self.census_resets = np.flatnonzero(np.diff(iv)) + 1               # blocks that open an interval
        self.census_blocks = len(iv); self.census_cats = set(r.sym for r in st.census if r.k == 0)
        self.claims = claims or {}
        self.per, self.parts, self.last_part = parts_of(nmcu)

    def reset_mcus(self):
        """{MCU: the blocks of it that a marker stands in front of}."""
        nb = BLOCKS[self.layout]; out = {}
        for b in self.resets.tolist():
            out.setdefault(b // nb, []).append(b % nb)
        return out

    def check(self, c=None):
        nb = BLOCKS[self.layout]; k = self.claims
        assert len(self.frame.mcu_blocks()) == nb and self.census_blocks == self.nmcu * nb
        assert np.array_equal(self.census_resets, self.resets), "the markers are where the model clears its sums"
        assert len(self.iv_ends) == self.markers + 1 and len(self.file) < (1 << 20)
        rm = self.reset_mcus()
        for m, js in k.get("resets_at", {}).items():
            assert rm.get(m) == list(js), (self.name, m, rm.get(m))
        if "only_resets" in k:
            assert sorted(rm) == sorted(k["only_resets"]), (self.name, sorted(rm)[:8])
        if "no_reset_in" in k:
            lo, hi = k["no_reset_in"]; assert not any(lo <= m < hi for m in rm), self.name
        cum, wraps = model(self)
        assert wraps >= k.get("wraps", 0), (self.name, wraps)
        for key in ("per", "parts", "last_part"):
            if key in k:
                assert getattr(self, key) == k[key], (self.name, key, getattr(self, key))
        if "sum_passes_2_31" in k:                                         # the kernel's `int` sums: the terms it adds are the int16 ones
            q0 = self.frame.qtabs[0][0]; t = (self.diffs * q0); assert t.min() == t.max() == 32752 and not len(self.resets)
            assert int(t.sum()) > (1 << 31) and int(t[:self.per * (self.parts - 1)].sum()) > (1 << 31), "in the image, and in the fold of the summaries"
        return wraps


def diffs_random(rng, n, cats=12):
    """n differences of random categories 0 .. cats - 1, either sign."""
    s = rng.integers(0, cats, n)
    half = np.where(s > 0, 1 << np.maximum(s - 1, 0), 0)
    mag = np.where(s > 0, half + rng.integers(0, 1 << 30, n) % np.maximum(half, 1), 0)
    return np.where(rng.integers(0, 2, n) == 1, mag, -mag)


CASES = []


def _add(name, group, layout, nmcu, dri, seed, q, extra=(), const=None, **claims):
    def build():
        rng = np.random.default_rng(seed)
        n = nmcu * BLOCKS[layout]
        d = np.full(n, const) if const is not None else diffs_random(rng, n)
        return Case(name, group, layout, nmcu, dri, d, q, extra, claims)
    build.__name__ = name
    CASES.append(build)


def _regular(nmcu, dri):
    return {m: [0] for m in range(dri, nmcu, dri)} if dri else {}


# ----------------------------------------------------------------------------------------------------------------- group A
# (MCU count, layout, restart interval); every count has a file without restarts and one whose interval puts a reset on its last seam
_A = [(63, "444", 0), (63, "420", 62), (64, "422", 0), (64, "gray", 63), (65, "gray", 0), (65, "420", 64),
      (1023, "420", 0), (1023, "444", 1022), (1024, "444", 0), (1024, "422", 1023), (1025, "422", 0), (1025, "gray", 1024), (1025, "420", 1),
      (2048, "gray", 0), (2048, "444", 1025), (2048, "422", 2047),
      (2049, "luma4x2", 0), (2049, "all4x4", 0), (2049, "luma4x2", 2048), (2049, "all4x4", 1024), (2049, "luma4x2", 63), (2049, "420", 65),
      (3073, "420", 0), (3073, "444", 1024), (3073, "gray", 1)]
for _i, (_n, _l, _d) in enumerate(_A):
    _add("a_%s_%d_%s" % (_l, _n, "no_restart" if not _d else "dri_%d" % _d), "A", _l, _n, _d, 1000 + _i, QPAIRS[(_i + 1) % 4],
         only_resets=list(_regular(_n, _d)), resets_at=_regular(_n, _d), wraps=1 if _n >= 1023 and not _d else 0)     # (those have a luma quantiser >= 37)

# ----------------------------------------------------------------------------------------------------------------- group B
_B = [(1025, "444", 1023), (1025, "420", 0), (2048, "420", 1024), (2048, "422", 0), (2049, "gray", 1025), (2049, "444", 2048), (2049, "422", 1024),
      (65536, "gray", 0), (65536, "gray", 1024), (65536, "gray", 1023), (65536, "gray", 1025), (65536, "gray", 33 * 1024)]
for _i, (_n, _l, _d) in enumerate(_B):
    _add("b_%s_%d_%s" % (_l, _n, "no_restart" if not _d else "dri_%d" % _d), "B", _l, _n, _d, 2000 + _i, QPAIRS[(_i + 2) % 4],
         only_resets=list(_regular(_n, _d)), resets_at=_regular(_n, _d), per=1024, parts=-(-_n // 1024), last_part=(_n - 1) % 1024 + 1,
         wraps=(1000 if not _d else 1) if _n == 65536 else 0)             # (65536 MCUs without restart: quantiser 37)

# ------------------------------------------------------------------------------------------------------------ groups C and D
# A file has one restart interval, so the six intervals of group C take six files above 65536 MCUs; the one without restarts is group D's:
# 33 * 2048 + 1 MCUs, because the FOLD of the summaries passes 2**31 only behind 65569 terms of 32752 -- the lone MCU of the last part
# folds 33 * 2048 = 67584 of them (in a picture of 257 x 256 MCUs the fold ends at 65536 terms, 2**31 - 1048576).
_add("d_gray_67585_no_restart_terms_32752", "D", "gray", 33 * 2048 + 1, 0, 3000, (16, 16), const=2047,
     only_resets=[], per=2048, parts=34, last_part=1, wraps=30000, sum_passes_2_31=True)
_C = [(33 * 2048 + 1, 2048, dict(last_part=1, parts=34)), (32 * 2048 + 1025, 1024, dict(last_part=1025, parts=33)),
      (257 * 256, 2047, dict(last_part=256, parts=33)), (257 * 256, 2049, dict(last_part=256, parts=33)),
      # one reset in the whole image: MCU 64000 = part 31 (63488 ..), its first step; none in its second
      (32 * 2048 + 1025, 64000, dict(last_part=1025, parts=33, only_resets=[64000], no_reset_in=(31 * 2048 + 1024, 32 * 2048)))]
for _i, (_n, _d, _k) in enumerate(_C):
    _lay = "444" if _d == 2047 else "gray"                                 # (one file with three components: what the DC-only fast form takes)
    _add("c_%s_%d_dri_%d" % (_lay, _n, _d), "C", _lay, _n, _d, 3001 + _i, [(37, 37), (255, 255), (4099, 37), (1, 1), (37, 37)][_i],
         resets_at=_regular(_n, _d), per=2048, wraps=1, **_k)

# ----------------------------------------------------------------------------------------------------------------- group E
# Regular markers, and markers inside an MCU: (layout, restart interval, [(MCU, block)], what the name says)
_E = [("420", 700, [(1024, 2)], "marker_before_block_2_of_mcu_1024"), ("luma4x2", 700, [(1023, 9)], "marker_before_last_block_of_mcu_1023"),
      ("luma4x2", 700, [(64, 1)], "marker_before_block_1_of_mcu_64"), ("420", 1024, [(1024, 3)], "markers_at_mcu_1024_and_before_its_block_3"),
      ("luma4x2", 1024, [(1024, 3)], "markers_at_mcu_1024_and_before_its_block_3"), ("420", 63, [(63, 3)], "markers_at_mcu_63_and_before_its_block_3"),
      ("luma4x2", 63, [(63, 3)], "markers_at_mcu_63_and_before_its_block_3")]
for _i, (_l, _d, _x, _what) in enumerate(_E):
    _at = _regular(2049, _d)
    for _m, _j in _x:
        _at[_m] = sorted(_at.get(_m, []) + [_j])
    _add("e_%s_2049_dri_%d_%s" % (_l, _d, _what), "E", _l, 2049, _d, 4000 + _i, QPAIRS[(_i + 2) % 4], extra=_x, resets_at=_at, only_resets=list(_at))


# ------------------------------------------------------------------------------------------------------------------ access
_BUILT = None


def build_all():
    """Every case, built once per process, in catalogue order."""
    global _BUILT
    if _BUILT is None:
        out = [fn() for fn in CASES]
        assert len({c.name for c in out}) == len(out)
        _BUILT = out
    return _BUILT


def built(name):
    return next(c for c in build_all() if c.name == name)
