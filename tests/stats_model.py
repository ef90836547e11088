"""A plain numpy MODEL of the bHistoEn / bStatClipEn colour statistics -- TEST INFRASTRUCTURE.

Written from the reference's source/ImgDecode.cpp, not from the kernels and not from the oracle's C restatement:

  * CalcChannelPreviewFull :4619-4821 -- the pixel walk (rows, then columns), the plane index py * (m_nBlkXMax * 8) + px (:4631, :4701), Cb = Cr = 0
    where the scan has one component (:4709-4715), the shift of every pixel whose MCU index py / mcu_h * (img_x / mcu_w) + px / mcu_w -- both
    divisions floor, so the pixels of a partial last MCU column share the index of the next row's first MCU -- is not below
    shift_mcu_y * (img_x / mcu_w) + shift_mcu_x (:4679, :4704-4705, :4735-4739), and ConvertYCCtoRGB when either option is set (:4742-4743);
  * ConvertYCCtoRGB :4229-4326 -- the Prerange records and the 2048-bin Y histogram with its clamp to [-1024, 1023] (:4238-4261), (v + 1024) / 8
    in C, which truncates toward zero (:4266-4268), the three float lines (:4287-4294) and the 128-bin histograms of the final bytes (:4313-4322);
  * CapYccRange :4341-4475 -- the Clip records and nCount (:4354-4365), then six checks in the order Y over, Y under, Cb over, Cb under, Cr over,
    Cr under; each clips always, but counts (and warns) only while m_nWarnYccClipNum < 10, a number that is cleared by Reset() (:130) and so
    lives across the decode and every re-render; the warning prints the three values with the earlier clips of the pixel applied;
  * CapRgbRange :4495-4601 -- (int) truncation first (:4500-4502), the Preclip RGB records of the truncated ints, the six counters (unconditional,
    :4516-4581: a float in (-1, 0) truncates to 0 and is no underflow, one in (255, 256) is no overflow), the Clip RGB records.

The records start from memset(0) (:3146-3147): a minimum never rises above 0, a maximum never falls below 0.  Everything is int64 here; the sums
are reduced modulo 2**32 when the record is written (the reference adds ints; where such a sum passes 2**31 its C++ is undefined and the
compiled reference wraps).  The colour lines are float32, one rounding per operation in the reference's order, a true division by 0.587f.

`run` takes the three int16 planes at their pitch (blk_xmax * 8), the image size, the MCU size, the component count and a list of passes
(histo_en, shift_mcu_x, shift_mcu_y, shift_y, shift_cb, shift_cr) -- the decode, then each re-render -- and returns per pass the record
accumulated so far (the JSNOOP_STATS_WORDS layout of include/jsnoop_gpu.h), the counted events and the running warning count.
"""
from __future__ import annotations

import numpy as np

STATS_WORDS = 2482
REPORT_MAX = 10                       # YCC_CLIP_REPORT_MAX
# PixelCcHisto (ImgDecode.h:238-279): twelve (min, max, sum) triplets, then nCount; PixelCcClip (:220-234) follows at word 37
GROUPS = ("PreclipY", "PreclipCb", "PreclipCr", "ClipY", "ClipCb", "ClipCr", "ClipR", "ClipG", "ClipB", "PreclipR", "PreclipG", "PreclipB")
CLIP_NAMES = ("Y<0", "Y>255", "Cb<0", "Cb>255", "Cr<0", "Cr>255", "R<0", "R>255", "G<0", "G>255", "B<0", "B>255", "White")
KINDS = ("Y Overflow", "Y Underflow", "Cb Overflow", "Cb Underflow", "Cr Overflow", "Cr Underflow")       # the order of the checks (:4371-4466)
KIND_CLIP_WORD = (1, 0, 3, 2, 5, 4)   # where PixelCcClip keeps the counter of each kind: the struct has Under in front of Over
PASS0 = (1, 0, 0, 0, 0, 0)

FLAWS = ("floor_division", "min_from_first_sample", "no_cap_at_10", "cb_before_y", "mcus_across_rounded_up", "range_check_before_truncation")


def word_name(k):
    """What word k of the record means."""
    if k < 36:
        return "%s.%s" % (GROUPS[k // 3], ("min", "max", "sum")[k % 3])
    if k == 36:
        return "count"
    if k < 50:
        return "clip[%s]" % CLIP_NAMES[k - 37]
    if k < 434:
        return "%s bin %d" % ("RGB"[(k - 50) // 128], (k - 50) % 128)
    return "Y bin %d" % (k - 434)


def _div8(v):
    """(v) / 8 of C: toward zero."""
    return np.where(v < 0, -((-v) // 8), v // 8)


class Pixels:
    """The per-pixel values of one pass, raster order: pre / clipv / fin (3, n) ints, rgbf (3, n) float32 in the order R, G, B, lim / rgb ints."""


def pixels(planes, img_x, img_y, mcu_w, mcu_h, ncomp, p, flaw=None):
    _h, smx, smy, sy, scb, scr = p
    py, px = np.divmod(np.arange(img_x * img_y, dtype=np.int64), img_x)
    o = Pixels()
    pre = np.zeros((3, img_x * img_y), np.int64)
    for c in range(3 if ncomp == 3 else 1):
        pre[c] = np.asarray(planes[c])[:img_y, :img_x].reshape(-1)
    across = img_x // mcu_w if flaw != "mcus_across_rounded_up" else -(-img_x // mcu_w)
    o.mcu_x, o.mcu_y = px // mcu_w, py // mcu_h
    shifted = o.mcu_y * across + o.mcu_x >= smy * across + smx
    pre += np.where(shifted, np.array([[sy], [scb], [scr]], np.int64), 0)
    o.pre = pre; o.shifted = shifted
    o.clipv = _div8(pre + 1024) if flaw != "floor_division" else (pre + 1024) // 8
    o.fin = np.clip(o.clipv, 0, 255)
    f32 = np.float32
    kr, kg, kb = f32(0.299), f32(0.587), f32(0.114)
    vy, vcb, vcr = [(o.fin[c] - 128).astype(f32) for c in range(3)]
    r = vcr * (f32(2) - f32(2) * kr) + vy
    b = vcb * (f32(2) - f32(2) * kb) + vy
    g = ((vy - kb * b) - kr * r) / kg
    o.rgbf = np.stack([r + f32(128), g + f32(128), b + f32(128)])
    assert o.rgbf.dtype == np.float32
    o.lim = o.rgbf.astype(np.int64)                                  # (int): toward zero
    if flaw == "range_check_before_truncation":
        o.rgb_under, o.rgb_over = o.rgbf < 0, o.rgbf > 255
    else:
        o.rgb_under, o.rgb_over = o.lim < 0, o.lim > 255
    o.rgb = np.clip(o.lim, 0, 255)
    return o


class Result:
    """records[k]: the uint32 record after pass k; events[k]: the counted events of pass k, each (pixel, (mcu_x, mcu_y), kind, (y, cb, cr));
    warn[k]: m_nWarnYccClipNum after pass k; found[k]: how many range events pass k met, counted or not; pix[k]: the pass's Pixels."""


def run(planes, img_x, img_y, mcu_w, mcu_h, ncomp, passes=(PASS0,), flaw=None, keep_pixels=True):
    assert flaw is None or flaw in FLAWS
    mn = [0] * 12; mx = [0] * 12; sm = [0] * 12; count = 0
    clip = np.zeros(13, np.int64); bins = np.zeros((3, 128), np.int64); ybins = np.zeros(2048, np.int64)
    warn = 0
    res = Result(); res.records, res.events, res.warn, res.found, res.pix = [], [], [], [], []
    for p in passes:
        q = pixels(planes, img_x, img_y, mcu_w, mcu_h, ncomp, p, flaw)
        n = img_x * img_y
        if p[0]:
            for gi, v in enumerate(list(q.pre) + list(q.clipv) + list(q.rgb) + list(q.lim)):
                if flaw == "min_from_first_sample" and count == 0:
                    mn[gi] = int(v[0])
                mn[gi] = min(mn[gi], int(v.min())); mx[gi] = max(mx[gi], int(v.max())); sm[gi] += int(v.sum())
            count += n
            for c in range(3):
                bins[c] += np.bincount(q.rgb[c] // 2, minlength=128)
            ybins += np.bincount(np.clip(q.pre[0], -1024, 1023) + 1024, minlength=2048)
        for c in range(3):
            clip[6 + 2 * c] += int(q.rgb_under[c].sum()); clip[7 + 2 * c] += int(q.rgb_over[c].sum())
        # the range events in visiting order: pixel by pixel, Y before Cb before Cr; a value is over or under, never both
        over, under = q.clipv > 255, q.clipv < 0
        order = (1, 0, 2) if flaw == "cb_before_y" else (0, 1, 2)
        hit = (over | under)[list(order)]                            # (3, n) in checking order
        at = np.flatnonzero(hit.T.reshape(-1))                       # index = pixel * 3 + place in the order
        res.found.append(len(at))
        left = max(REPORT_MAX - warn, 0) if flaw != "no_cap_at_10" else len(at)
        ev = []
        for k in at[:left].tolist():
            pix, c = k // 3, order[k % 3]
            kind = 2 * c + (0 if over[c, pix] else 1)
            done = order[:order.index(c)]                            # the components checked before this one are printed clipped
            vals = tuple(int(q.fin[j, pix]) if j in done else int(q.clipv[j, pix]) for j in range(3))
            ev.append((pix, (int(q.mcu_x[pix]), int(q.mcu_y[pix])), KINDS[kind], vals))
            clip[KIND_CLIP_WORD[kind]] += 1
        warn += len(ev)
        rec = np.zeros(STATS_WORDS, np.int64)
        for gi in range(12):
            rec[3 * gi], rec[3 * gi + 1], rec[3 * gi + 2] = mn[gi], mx[gi], sm[gi]
        rec[36] = count; rec[37:50] = clip; rec[50:434] = bins.reshape(-1); rec[434:] = ybins
        res.records.append((rec & 0xFFFFFFFF).astype(np.uint32))
        res.events.append(ev); res.warn.append(warn); res.pix.append(q if keep_pixels else None)
    res.sums = list(sm)                                              # not reduced
    return res


def first_difference(got, exp):
    """(word index, its name, got, expected) of the first differing word of two records, or None."""
    got = np.asarray(got, np.uint32); exp = np.asarray(exp, np.uint32)
    d = np.flatnonzero(got != exp)
    if not len(d):
        return None
    k = int(d[0])
    sg = lambda v: int(np.uint32(v).astype(np.int32)) if k < 36 else int(v)
    return k, word_name(k), sg(got[k]), sg(exp[k])


def warning_lines(events, warn_before, offset_text):
    """The lines CapYccRange logs for one pass's counted events (:4374-4381)."""
    out = []
    for i, (_pix, (mx, my), kind, (y, cb, cr)) in enumerate(events):
        out.append("*** NOTE: YCC Clipped. MCU=(%4u,%4u) YCC=(%5d,%5d,%5d) %s @ Offset %s" % (mx, my, y, cb, cr, kind, offset_text))
        if warn_before + i + 1 == REPORT_MAX:
            out.append("    Only reported first %u instances of this message..." % REPORT_MAX)
    return out
