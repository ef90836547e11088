"""The catalogue behind tests/test_batch_stats_cases.py (CPU) and tests/test_gpu_batch_stats.py (GPU): pictures for the seams of jsnoop_batch_pack_stats
(k_stats_batch, k_stats_order in jpegsnoop_amd/csrc/jsnoop_stats.hip), built with stats_cases.Case -- baseline files over one flat DC table and a quantiser
of 1, all DC where whole blocks will do, `peaks` (single samples moved by AC coefficients) where single samples are needed; such a file's checks take
the planes the oracle decoded with Full IDCT.

How the kernels deal the work, restated here and read back from the source by the CPU test:
  UNIT      pixels of one picture row a wave takes at a time: a lane owns eight consecutive samples (jsnoop_types.h:165 JS_STATS_UNIT, jsnoop_stats.hip:136)
  WAVES     waves of a workgroup, interleaved over its contiguous share of the units (jsnoop_stats.hip:35 SB_WAVES, :126 `u += SB_WAVES`)
  ORDER_STEP  pixels of a listed picture row k_stats_order walks per step (jsnoop_stats.hip:239 `x0 += 64u`)
  ORDER_ROWS  picture rows whose event counts k_stats_order scans per step (jsnoop_stats.hip:34 SB_THREADS, :222 `base += SB_THREADS`)

Groups.  "S" unit seams: gray and 4:4:4 pictures 8, UNIT - 8, UNIT, UNIT + 8 and 2 UNIT + 8 wide and 16 high.  Block row 0 is grey but for single samples:
the largest Y in sample 0 of lane 0 (x = 0), the smallest in sample 7 of the first unit's last lane (x = min(W, UNIT) - 1), and where there is a second
unit the second largest (gray) or the largest Cb (4:4:4) in its first lane (x = UNIT); every range event, and nothing else that is not grey, lies in the
picture's last block.  "L" layouts: 4:2:0, 4:2:2 and 4:4:0 at widths 16 and UNIT + 16, levels from a random walk that leaves the range.  "O" order and
budget: totals of exactly 10 and 11, the 10th event on the last pixel of a picture row and on the first of the next, 11 rows with one event each, all
events in the last row, the 10th and 11th events in different units of one row and on both sides of a step of the row walk, a pixel of three events
entered with 9 used.  "M" many small pictures: 8 x 8 and 16 x 16, every one with levels of its own, every third with range events.
"""
from __future__ import annotations

import numpy as np

import stats_cases as SC
from stats_cases import Case, DEEP, HIGH, OVER, UNDER, frame_of

UNIT = 512
WAVES = 4
ORDER_STEP = 64
ORDER_ROWS = 256
MARK_HI, MARK_LO, MARK_2ND = 900, -900, 700       # single samples that stay in range: (900 + 1024) / 8 = 240, (-900 + 1024) / 8 = 15

CASES = []


def _add(name, fn):
    fn.__name__ = name
    CASES.append(fn)


def _peaks(marks):
    """[(x, y, component, height)] -> Case's (component, block row, block column, sample row, sample column, height)."""
    return [(c, y // 8, x // 8, y % 8, x % 8, h) for x, y, c, h in marks]


# ----------------------------------------------------------------------------------------------------------------- group S
SEAM_WIDTHS = (8, UNIT - 8, UNIT, UNIT + 8, 2 * UNIT + 8)


def seam_marks(layout, width):
    """{role: (x, y, component, height)} of a unit-seam picture."""
    m = {"lane0_sample0": (0, 3, 0, MARK_HI), "lane63_sample7": (min(width, UNIT) - 1, 5, 0, MARK_LO)}
    if width > UNIT:
        m["unit1_lane0"] = (UNIT, 2, 0 if layout == "gray" else 1, MARK_2ND if layout == "gray" else MARK_HI)
    return m


def _s(layout, width):
    name = "s_%s_%dx16" % (layout, width)

    def build():
        fr = frame_of(layout, width, 16); g = SC._grids(fr)
        last = (UNDER,) if layout == "gray" else (0, UNDER, OVER)          # the last block: Y under (gray), or Cb under and Cr over with Y grey
        for c in range(fr.ncomp):
            g[c][1, width // 8 - 1] = last[c]
        marks = seam_marks(layout, width)
        return Case(name, "S", layout, width, 16, g, claims=dict(found=[64 * (1 if layout == "gray" else 2)], warn=[10], seam=marks), peaks=_peaks(marks.values()))
    _add(name, build)


for _l in ("gray", "444"):
    for _w in SEAM_WIDTHS:
        _s(_l, _w)


def check_seam(case, res):
    """The claims of a group S picture from the model's pixels of pass 0 (res = case.model(1, planes))."""
    q = res.pix[0]; W = case.img_x; n = case.name
    last = np.zeros(case.npix, bool).reshape(case.img_y, W); last[8:, W - 8:] = True; last = last.reshape(-1)
    ev = ((q.clipv > 255) | (q.clipv < 0)).any(0)
    assert ev.any() and not (ev & ~last).any(), (n, "every range event lies in the last block")
    assert {e[0] for e in res.events[0]} <= set(np.flatnonzero(last).tolist())
    for role, (x, y, c, h) in case.claims["seam"].items():
        pix = y * W + x; v = np.where(last, 0, q.pre[c])
        if h == MARK_HI:
            assert int(v.argmax()) == pix and int((v == v.max()).sum()) == 1 and abs(int(v[pix]) - h) < 40, (n, role, int(v.argmax()), int(v.max()))
        elif h == MARK_LO:
            assert int(v.argmin()) == pix and int((v == v.min()).sum()) == 1 and abs(int(v[pix]) - h) < 40, (n, role, int(v.argmin()), int(v.min()))
        else:                                                              # the second largest: nothing but the lane-0 mark is above it
            assert int((v > v[pix]).sum()) == 1 and int((v == v[pix]).sum()) == 1 and abs(int(v[pix]) - h) < 40, (n, role)
        lane, sample, unit = (x % UNIT) // 8, x % 8, x // UNIT
        want = {"lane0_sample0": (0, 0, 0), "lane63_sample7": (min(W, UNIT) // 8 - 1, 7, 0), "unit1_lane0": (0, 0, 1)}[role]
        assert (lane, sample, unit) == want, (n, role, lane, sample, unit)
    rec = res.records[0][:36].view(np.int32)
    if case.layout == "gray":
        assert rec[1] == int(q.pre[0][3 * W]) and rec[0] == UNDER, (n, rec[:3].tolist())          # the largest Y is the lane-0 mark; the smallest is the last block's
    else:
        assert rec[1] == int(q.pre[0][3 * W]) and rec[0] == int(q.pre[0][5 * W + min(W, UNIT) - 1]), (n, rec[:3].tolist())
        assert rec[3] == UNDER and rec[7] == OVER, n


# ----------------------------------------------------------------------------------------------------------------- group L
def _l(layout, width, seed):
    name = "l_%s_%dx16" % (layout, width)

    def build():
        fr = frame_of(layout, width, 16); rng = np.random.default_rng(seed)
        g = [SC._walk(rng, fr, c, -1300, 1300) for c in range(fr.ncomp)]
        return Case(name, "L", layout, width, 16, g, claims=dict(events_some=True))
    _add(name, build)


for _k, _lay in enumerate(("420", "422", "440")):
    _l(_lay, 16, 300 + _k); _l(_lay, UNIT + 16, 310 + _k)


# ----------------------------------------------------------------------------------------------------------------- group O
def _o(name, width, height, events, layout="444", **claims):
    """events: [(x, y, component, height)], single samples out of range."""
    def build():
        fr = frame_of(layout, width, height)
        return Case(name, "O", layout, width, height, SC._grids(fr), claims=claims, peaks=_peaks(events))
    _add(name, build)


def _ys(points, h=HIGH):
    return [(x, y, 0, h) for x, y in points]


_P9 = [(3, 0), (17, 0), (5, 1), (20, 2), (9, 3), (1, 4), (22, 5), (13, 6), (7, 9)]                 # nine events of a 24-wide picture, raster order
_o("o_total_10", 24, 16, _ys(_P9 + [(11, 12)]), found=[10], warn=[10], tenth=(0, 12 * 24 + 11, "Y Overflow", None))
_o("o_total_11", 24, 16, _ys(_P9 + [(11, 12)]) + [(2, 14, 0, DEEP)], found=[11], warn=[10], tenth=(0, 12 * 24 + 11, "Y Overflow", None))
_o("o_tenth_on_last_pixel_of_row", 24, 16, _ys(_P9 + [(23, 10), (0, 11), (12, 13)]), found=[12], warn=[10], tenth=(0, 10 * 24 + 23, "Y Overflow", None))
_o("o_tenth_on_first_pixel_of_next_row", 24, 16, _ys(_P9 + [(0, 11), (1, 11), (23, 15)]), found=[12], warn=[10], tenth=(0, 11 * 24 + 0, "Y Overflow", None))
_o("o_eleven_rows_one_event_each", 24, 16, _ys([((5 * r + 2) % 24, r + 2) for r in range(11)]), found=[11], warn=[10], tenth=(0, 11 * 24 + (5 * 9 + 2) % 24, "Y Overflow", None),
   rows_of_counted=list(range(2, 12)))
_o("o_all_in_last_row", 24, 16, [(x, 15, k % 3, DEEP if k % 3 == 2 else HIGH) for k, x in enumerate(range(0, 24, 2))], found=[12], warn=[10], last_row_only=True,
   rows_of_counted=[15])
_UX = [4, 60, 130, 200, 260, 330, 390, 450, 480]                                                   # nine events inside unit 0 of row 6
_o("o_tenth_and_eleventh_in_two_units", UNIT + 8, 8, _ys([(x, 6) for x in _UX + [UNIT - 1, UNIT, UNIT + 7]]), found=[12], warn=[10],
   tenth=(0, 6 * (UNIT + 8) + UNIT - 1, "Y Overflow", None), rows_of_counted=[6])
_o("o_tenth_in_the_second_unit", UNIT + 8, 8, _ys([(x, 6) for x in _UX + [UNIT + 2, UNIT + 5]]), found=[11], warn=[10], tenth=(0, 6 * (UNIT + 8) + UNIT + 2, "Y Overflow", None))
_o("o_tenth_and_eleventh_across_a_walk_step", 136, 8, _ys([(x, 2) for x in (1, 9, 18, 27, 36, 45, 54, 60, 62, 63, 64, 127, 128)]), found=[13], warn=[10],
   tenth=(0, 2 * 136 + 63, "Y Overflow", None), rows_of_counted=[2])
_o("o_tenth_on_the_first_pixel_of_a_walk_step", 136, 8, _ys([(x, 2) for x in (1, 9, 18, 27, 36, 45, 54, 60, 63, 64, 65)]), found=[11], warn=[10],
   tenth=(0, 2 * 136 + 64, "Y Overflow", None))
_T = [(14, 7, 0, HIGH), (14, 7, 1, DEEP), (14, 7, 2, HIGH)]                                         # over in Y, under in Cb, over in Cr
_o("o_three_events_entered_with_9_used", 24, 16, _ys(_P9[:8] + [(2, 7)]) + _T, found=[12], warn=[10], events_in_pixel=(0, 7 * 24 + 14, 3, 1), tenth=(0, 7 * 24 + 14, "Y Overflow", None))
_o("o_three_events_entered_with_8_used", 24, 16, _ys(_P9[:8]) + _T, found=[11], warn=[10], events_in_pixel=(0, 7 * 24 + 14, 3, 2), tenth=(0, 7 * 24 + 14, "Cb Underflow", None))
_o("o_three_events_gray_column", 8, 32, [(3, y, 0, DEEP if y % 2 else HIGH) for y in range(4, 30, 2)], layout="gray", found=[13], warn=[10],
   tenth=(0, 22 * 8 + 3, "Y Overflow", None), rows_of_counted=list(range(4, 24, 2)))


# ----------------------------------------------------------------------------------------------------------------- group M
SMALL = 198


def _m(k):
    layout, side = (("gray", 8), ("444", 8), ("420", 16), ("444", 16), ("422", 16), ("gray", 16))[k % 6]
    name = "m_%03d_%s_%d" % (k, layout, side)

    def build():
        fr = frame_of(layout, side, side); rng = np.random.default_rng(5000 + k); g = SC._grids(fr)
        for c in range(fr.ncomp):
            g[c][:] = rng.integers(-1000, 1001, g[c].shape)                # in range: (-1000 + 1024) / 8 = 3, (1000 + 1024) / 8 = 253
        if k % 3 == 0:                                                     # every third: one block of one component out of range
            c = (k // 3) % fr.ncomp
            g[c][-1, -1] = OVER if (k // 6) % 2 else UNDER
        return Case(name, "M", layout, side, side, g, claims=dict(found=[0] if k % 3 else None))
    _add(name, build)


for _k in range(SMALL):
    _m(_k)


# ------------------------------------------------------------------------------------------------------------------ access
_BUILT = None


def build_all():
    """Every case, built once per process, in catalogue order."""
    global _BUILT
    if _BUILT is None:
        out = [fn() for fn in CASES]
        assert len({c.name for c in out}) == len(out), "names are unique"
        for c in out:
            if c.claims.get("found", 0) is None:
                del c.claims["found"]
        _BUILT = out
    return _BUILT


def built(name):
    return next(c for c in build_all() if c.name == name)
