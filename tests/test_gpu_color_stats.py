"""-m gpu: the bHistoEn / bStatClipEn colour statistics (k_color_stats, k_clip_order, stat_pixel; the budget logic of
JsnoopBatch::color_stats_pass) on the catalogue of tests/stats_cases.py: pictures above one and above two sweeps of k_color_stats whose only
events lie in the last block row, the 10th range event on the last pixel of a k_clip_order step, on the first of the next, inside a pixel of
three events and in the last partial step, samples on the edges of the truncating division, records that stay at 0, sums past 2**31 and
2**32, RGB values within 1 of the clip limits, shift origins around every row seam, and the 10-warning budget across re-renders.
tests/test_stats_cases.py proves on the CPU that every file holds what its name says, that a plain numpy model of the statistics equals the
oracle on every file, and that the oracle's records and the warnings are the compiled reference's.

Everything is compared exactly: the DIB, the int16 planes and the 2482 words, after the decode and after each re-render, through the
single-image decoder (with a log sink: every event goes through k_clip_order; without one: the totals of k_color_stats while they fit the
budget) and through JpegBatch.  A failure names the first differing word by meaning (`PreclipY.min`, `clip[Y>255]`, `R bin 127`) and, for
a clip counter, the model's first event that the counters miss: its pixel, pixel % 1024, pixel // SWEEP, MCU and kind.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import stats_cases as SC
import stats_model as SM
from stats_cases_util import OPTION_SETS, explain, recorded_log, run_passes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_cases.json")


@pytest.fixture(scope="module")
def world(harness, oracle):
    """{case name: (case, {option set: the oracle's run_passes}, {option set: the model on the oracle's planes})}, built once."""
    out = {}
    for c in SC.build_all():
        ans = {key: run_passes(harness, oracle, c, key, keep=True) for key in OPTION_SETS}
        mod = {key: c.model(OPTION_SETS[key][1], planes=ans[key]["planes"], keep_pixels=False) for key in OPTION_SETS}
        out[c.name] = (c, ans, mod)
    return out


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_reach(world):
    """What the catalogue reaches, computed from SWEEP, CLIP_STEP and the model's events on the oracle's planes: it cannot shrink unnoticed."""
    sweeps = {c.name: -(-c.npix // SC.SWEEP) for c, _, _ in world.values()}
    assert sum(1 for n in sweeps.values() if n == 2) >= 4 and sum(1 for n in sweeps.values() if n >= 3) >= 1, sweeps
    late = [c.name for c, _, m in world.values() if sweeps[c.name] >= 2 and m["histo"].events[0] and all(e[0] >= SC.SWEEP for e in m["histo"].events[0])]
    assert len(late) >= 4, "files whose every counted event lies behind the first sweep: %s" % late
    assert any(sweeps[c.name] == 3 and all(e[0] >= 2 * SC.SWEEP for e in m["histo"].events[0]) for c, _, m in world.values() if m["histo"].events[0])
    tenth_at = set(); inside_pixel = 0; last_step = 0
    for c, _, m in world.values():
        r = m["histo"]
        for p, ev in enumerate(r.events):
            if not ev or r.warn[p] != SM.REPORT_MAX or (p and r.warn[p - 1] == SM.REPORT_MAX):
                continue
            pix = ev[-1][0]                                                # the pixel of the event that uses the budget up
            tenth_at.add(pix % SC.CLIP_STEP)
            if r.found[p] > len(ev):                                       # events behind it: are some in the same pixel?
                q = c.model(1, planes=world[c.name][1]["histo"]["planes"]).pix[p]
                has = int(((q.clipv[:, pix] > 255) | (q.clipv[:, pix] < 0)).sum())
                inside_pixel += has > sum(1 for e in ev if e[0] == pix)
            last_step += pix // SC.CLIP_STEP == (c.npix - 1) // SC.CLIP_STEP and c.npix % SC.CLIP_STEP != 0 and c.npix > SC.CLIP_STEP
    assert SC.CLIP_STEP - 1 in tenth_at and 0 in tenth_at, sorted(tenth_at)
    assert inside_pixel >= 2 and last_step >= 2, (inside_pixel, last_step)
    used = {(m["histo"].warn[0], len(m["histo"].warn)) for c, _, m in world.values() if c.group == "G"}
    assert {u for u, _ in used} == {0, 4, 10} and {n for _, n in used} == {2, 3}, used


def compare(case, key, got, ans, mod, errs, what, log=None):
    """got / ans: run_passes of the library and of the oracle."""
    for p in range(len(ans["words"])):
        tag = "%s [%s] %s pass %d" % (case.name, key, what, p)
        if got["dibs"][p].shape != ans["dibs"][p].shape or not np.array_equal(got["dibs"][p], ans["dibs"][p]):
            errs.append("%s: the DIB differs" % tag)
        if not np.array_equal(got["words"][p], ans["words"][p]):
            assert np.array_equal(ans["words"][p], mod.records[p]), "the model is the oracle (tests/test_stats_cases.py)"
            errs.append("%s: %s" % (what, explain(case, key, p, got["words"][p], mod)))
        if log is not None and got["log"][p] != log[p]:
            k = next((i for i, (a, b) in enumerate(zip(got["log"][p], log[p])) if a != b), min(len(got["log"][p]), len(log[p])))
            errs.append("%s: warning %d is %r, the reference wrote %r (%d lines, %d)" % (
                tag, k, got["log"][p][k] if k < len(got["log"][p]) else None, log[p][k] if k < len(log[p]) else None, len(got["log"][p]), len(log[p])))
    for k in range(case.ncomp):
        if not np.array_equal(got["planes"][k], ans["planes"][k]):
            errs.append("%s [%s] %s: plane %d differs in %d samples" % (case.name, key, what, k, int((got["planes"][k] != ans["planes"][k]).sum())))


@pytest.mark.parametrize("key", list(OPTION_SETS))
def test_single_image_decoder_with_a_log_sink(harness, gpu, world, want, key):
    """Decode, then the case's re-renders: DIB, planes, the record and the clip warnings after each pass.  The warnings are the compiled
    reference's lines, in order; with a log sink every pass that has an event and budget left goes through k_clip_order."""
    errs = []; forms = {}
    for c, ans, mod in world.values():
        got = run_passes(harness, gpu, c, key, keep=True, probe=lambda b: int(b.lib.jsnoop_last_form(C.c_void_p(b.h))))
        forms.setdefault(got["probe"], set()).add(c.layout)
        compare(c, key, got, ans[key], mod[key], errs, "single", recorded_log(want[c.name], key))
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
    assert set(forms) == {1}, forms                                         # (a decoder with a log sink keeps the coefficient arena: the generic kernels, also DC only)


def test_single_image_decoder_without_a_log_sink(harness, gpu, world):
    """No sink: a pass whose events fit what is left of the budget takes its counters from k_color_stats' totals, one that exceeds it goes through
    k_clip_order, one that finds the budget used up through neither -- groups B and G arrange which, the model's pass list is the history.
    And with decode_ac = 0 the files of the fast layouts are decoded by the DC-only fast form, the others by the generic kernels: the
    statistics behind both (a re-render then repeats the decode in the generic form)."""
    b = harness.Backend(gpu.lib, "jsnoop_", "hip, no log sink")
    try:
        b._f("set_log_callback")(b.h, type(b._log_cb)(), None)             # a null function pointer: no sink
        errs = []; arms = set(); forms = {key: {} for key in ("histo", "histo_dc", "clip_dc")}
        for c, ans, mod in world.values():
            for key in forms:
                got = run_passes(harness, b, c, key, keep=True, probe=lambda d: int(d.lib.jsnoop_last_form(C.c_void_p(d.h))))
                assert not any(got["log"]), "a decoder without a sink logs nothing"
                forms[key].setdefault(got["probe"], set()).add(c.layout)
                compare(c, key, got, ans[key], mod[key], errs, "no sink")
                r = mod[key]
                for p in range(len(r.found)):
                    left = SM.REPORT_MAX - (r.warn[p - 1] if p else 0)
                    arms.add("totals" if r.found[p] <= left else "order" if left else "spent")
        assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
        assert arms == {"totals", "order", "spent"}, arms
        assert set(forms["histo"]) == {1}, forms
        for key in ("histo_dc", "clip_dc"):
            assert forms[key][2] == set(SC.FAST_LAYOUTS) and forms[key][1] == {"gray"}, forms
    finally:
        b.close()


def _batch(world, names, decode_ac, want, form, log=True):
    import jpegsnoop_amd as J
    hk, ck = ("histo", "clip") if decode_ac else ("histo_dc", "clip_dc")
    b = J.JpegBatch(decode_ac=decode_ac, want_planes=True)
    errs = []
    try:
        if log:
            b.enable_log()                                                  # (keeps the decoder's event records: the generic kernels, also DC only)
        for n in names:
            b.add_jpeg(world[n][0].file)
        b.upload(); b.decode(); b.sync()
        assert b.last_form() == form, (b.last_form(), form)
        for i, n in enumerate(names):
            c, ans, mod = world[n]
            dib = b.dib(i)
            if dib.shape != ans[hk]["dibs"][0].shape or not np.array_equal(dib, ans[hk]["dibs"][0]):
                errs.append("%s (image %d): the DIB differs" % (n, i))
            for k, pl in enumerate(b.planes(i)):
                if not np.array_equal(pl, ans[hk]["planes"][k]):
                    errs.append("%s (image %d): plane %d differs" % (n, i, k))
            for key, histo_en in ((hk, True), (ck, False)):
                got = b.color_stats(i, histo_en=histo_en)
                if not np.array_equal(got, ans[key]["words"][0]):
                    errs.append("batch image %d: %s" % (i, explain(c, key, 0, got, mod[key])))
                if not log:
                    continue
                lines = ["W:" + t for lvl, t in b.log_lines(i, histo_en=histo_en, stat_clip_en=not histo_en, quiet=True) if lvl == 1 and ("YCC Clipped" in t or "Only reported first" in t)]
                if lines != recorded_log(want[n], key)[0]:
                    errs.append("%s (image %d) [%s]: log_lines wrote %d clip warnings, the reference %d; first %r" % (n, i, key, len(lines), len(recorded_log(want[n], key)[0]), lines[:1]))
        assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
    finally:
        b.close()


def test_batch_full_idct(world, want):
    """Every catalogue file in one batch: mixed geometries, plane_off non-zero; color_stats with and without bHistoEn, and the clip warnings of log_lines."""
    _batch(world, list(world), True, want, 1)


def test_batch_dc_only_fast_form(world, want):
    """The files of the fast layouts with decode_ac = False: the batch's last form is the DC-only one (a batch that keeps event records for
    log_lines decodes in the generic form: that one second, with the warnings)."""
    names = [n for n, (c, _, _) in world.items() if c.layout in SC.FAST_LAYOUTS]
    assert len(names) >= 30
    _batch(world, names, False, want, 2, log=False)
    _batch(world, names, False, want, 1)                                   # with the event records kept: the generic kernels, and log_lines


def test_batch_dc_only_generic(world, want):
    names = [n for n, (c, _, _) in world.items() if c.layout not in SC.FAST_LAYOUTS]
    assert len(names) >= 8
    _batch(world, names, False, want, 1)
