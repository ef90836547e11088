"""CPU: the colour statistics catalogue (tests/stats_cases.py) holds what it claims; the plain numpy MODEL of tests/stats_model.py
(ConvertYCCtoRGB / CapYccRange / CapRgbRange / the walk of CalcChannelPreviewFull, restated from the reference's source) equals the oracle
word for word on every catalogue file, under every option set and after every pass, on every golden file and on the small pictures of
tests/backend_images.py; and the oracle equals the compiled reference (tests/golden/stats_cases.json, written by
tests/golden/make_stats_cases.py: one digest of the record per case, option set and pass, and the reference's clip warnings verbatim).
The GPU tests of tests/test_gpu_color_stats.py compare k_color_stats / k_clip_order with the oracle on these files, so this pins what they
check to the reference and to arithmetic anyone can read.

Group D (sums that pass 2**31 and 2**32: signed overflow, undefined in the reference's C++): the compiled reference wraps modulo 2**32 on all
three files, as the oracle and the model do, so none is left out of the JSON (make_stats_cases.py would name such a file under "_left_out").

Six deliberately wrong variants of the model were tried (stats_model.FLAWS).  test_wrong_models_are_refused keeps the trial of five: each is
refused by the `check` of the case named in REFUSED_BY and by the comparison with the oracle on that file.  The sixth, `mcus_across` rounded
up, cannot be refused by any file: the statistics walk the MCU-padded picture, so img_x / mcu_w is exact and there is no partial last MCU column to
alias (test_mcus_across_rounded_up_cannot_be_told_apart)."""
import json
import os

import numpy as np
import pytest

import stats_cases as SC
import stats_model as SM
from stats_cases_util import OPTION_SETS, explain, recorded_log, run_passes, words

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_cases.json")


@pytest.fixture(scope="module")
def cases():
    return SC.build_all()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def decoded(harness, oracle, cases):
    """{(case, option set): run_passes of the oracle}, once for the module."""
    return {(c.name, key): run_passes(harness, oracle, c, key, keep=True) for c in cases for key in OPTION_SETS}


def test_the_constants_are_the_kernels():
    """SWEEP and CLIP_STEP restate the launch of k_color_stats and the step of k_clip_order: read them back from the source."""
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "jpegsnoop_amd", "csrc", "jsnoop_kernels.hip")).read()
    assert "#define ST_THREADS 256" in src and "hipLaunchKernelGGL(k_color_stats, dim3(512), dim3(ST_THREADS)" in src and SC.SWEEP == 512 * 256
    assert "for (uint32_t base = 0; base < npix; base += 1024)" in src and "hipLaunchKernelGGL(k_clip_order, dim3(1), dim3(1024)" in src and SC.CLIP_STEP == 1024


def test_the_oracle_decodes_the_planes_the_cases_know(cases, decoded):
    """An all-DC file decodes to its cumulative DC in every sample, with the IDCT (a DC-only block adds nothing) and without it, over the whole int16 range."""
    for c in cases:
        for key in OPTION_SETS:
            got = decoded[c.name, key]["planes"]
            if c.planes is None:
                assert c.group == "H" or c.peaks
                continue
            for k in range(c.ncomp):
                assert np.array_equal(got[k], c.planes[k]), (c.name, key, k)


def test_every_check_holds(cases, decoded):
    for c in cases:
        c.check(planes=decoded[c.name, "histo"]["planes"] if c.planes is None else None)
    assert {c.group for c in cases} == set("ABCDEFGH")
    a = [c for c in cases if c.group == "A"]
    for layout, mcu_h in (("gray", 8), ("444", 8), ("420", 16)):                # one row of MCUs below a sweep, a sweep, one row above
        assert {c.npix for c in a if c.layout == layout} >= {SC.SWEEP - mcu_h * 512, SC.SWEEP, SC.SWEEP + mcu_h * 512}, layout
    assert any(2 * SC.SWEEP < c.npix <= 3 * SC.SWEEP for c in a)
    assert {c.layout for c in cases if c.npix > SC.SWEEP} >= {"gray", "444", "420", "440"}, "fast layouts and gray above one sweep"
    c_ = [c for c in cases if c.group == "C"]
    assert {c.claims["division"][0] for c in c_} == {0, 1, 2} and {c.layout for c in c_ if c.claims["division"][0] == 0} == {"gray", "444"}
    assert set(SC.DIVISION) == {-1033, -1032, -1031, -1025, -1024, -1023, -8, -1, 0, 1015, 1016, 1023, 1024, 1031, 1032, -32768, 32767}
    big = max(c.npix for c in a)
    assert all(c.npix <= big for c in cases) and all(c.width <= 512 and c.height <= 512 for c in cases if c.group == "E")
    g = [c for c in cases if c.group == "G"]
    assert {c.claims["found"][0] for c in g} == {0, 4, 10, 16} and {len(c.rerenders) for c in g} == {1, 2}
    rel = set()                                                            # a re-render's own total against what is left of the budget
    for c in g:
        for p in range(1, len(c.claims["found"])):
            left = 10 - c.claims["warn"][p - 1]; t = c.claims["found"][p]
            rel.add((left > 0, "none" if t == 0 else "below" if t < left else "equal" if t == left else "above"))
    assert rel == {(True, "none"), (True, "below"), (True, "equal"), (True, "above"), (False, "none"), (False, "above")}, rel
    f = [c for c in cases if c.group == "F"]
    assert {(c.layout, c.width % c.mcu_w) for c in f} >= {("420", 0), ("420", 1), ("420", 15), ("gray", 7), ("gray", 0)}
    assert all(c.img_x % c.mcu_w == 0 and c.img_x // c.mcu_w == c.frame.mcu_x for c in cases), "the walked picture has whole MCUs only"
    h = [c for c in cases if c.group == "H"]
    assert sorted(c.npix > SC.SWEEP for c in h) == [False, True] and any(c.dri for c in h)


def test_the_writer_is_deterministic_and_the_files_are_the_recorded_ones(harness, cases, want):
    assert sorted(c.name for c in cases) == sorted(n for n in want if n != "_left_out")
    for c in cases:
        assert harness.hash_bytes(c.file) == want[c.name]["sha256"], c.name
    for i in (0, 20, len(cases) - 1):
        again = SC.CASES[i]()
        assert again.file == cases[i].file and again.name == cases[i].name


def test_the_model_is_the_oracle_on_the_catalogue(cases, decoded):
    """model(oracle.planes(), ...) == oracle.color_stats(), word for word: bHistoEn, bStatClipEn alone, Full IDCT and DC only, after each pass."""
    errs = []
    for c in cases:
        for key, (_opt, histo_en) in OPTION_SETS.items():
            d = decoded[c.name, key]
            res = c.model(histo_en, planes=d["planes"], keep_pixels=False)
            for p, got in enumerate(d["words"]):
                e = explain(c, key, p, got, res)
                if e:
                    errs.append(e)
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:20]))


def _model_against(harness, oracle, data, rerender=(1, 1, 500, -200, 100)):
    out = []
    for key, (opt, histo_en) in OPTION_SETS.items():
        oracle.set_options(**opt)
        try:
            harness.drive(oracle, data)
            if oracle.dib() is None:
                continue
            g = oracle.geometry(); pl = oracle.planes()
            res = SM.run(pl, g[6], g[7], g[0], g[1], 3 if pl[1] is not None else 1, [(histo_en, 0, 0, 0, 0, 0), (histo_en,) + rerender], keep_pixels=False)
            out.append((key, 0, SM.first_difference(words(oracle), res.records[0])))
            oracle.set_preview_ycc_offset(*rerender)
            out.append((key, 1, SM.first_difference(words(oracle), res.records[1])))
            oracle.set_preview_ycc_offset(0, 0, 0, 0, 0)
        finally:
            oracle.set_options()
    return out


def test_the_model_is_the_oracle_on_the_golden_files_and_the_small_pictures(harness, oracle):
    import backend_images as BI
    from golden_util import load_case, manifest
    files = {name: load_case(name) for name in sorted(manifest()["cases"])}
    for layout in BI.LAYOUTS:
        files["flat_%s_white" % layout] = BI.flat(harness, layout, "white")
    for layout in ("420", "444", "gray"):
        files["fields_%s" % layout] = BI.fields(harness, layout)
    files["raster_tie_440"] = BI.raster_tie(harness, "440")
    seen = 0
    for name, data in files.items():
        for key, p, d in _model_against(harness, oracle, data):
            seen += 1
            assert d is None, (name, key, p, d)
    assert seen > 4 * len(BI.LAYOUTS)


def test_the_model_writes_the_reference_s_warnings(cases, want, decoded):
    """The model's event lists -- MCU, kind, the three values with the earlier clips of the pixel applied, the "first 10" line -- as the lines
    the compiled reference logged, after the decode and after each re-render, under every option set (the offset text is the reader's
    position, taken from the record)."""
    n = 0
    for c in cases:
        for key, (_opt, histo_en) in OPTION_SETS.items():
            res = c.model(histo_en, planes=decoded[c.name, key]["planes"], keep_pixels=False)
            rec = recorded_log(want[c.name], key)
            text = next((l.split("@ Offset ")[1] for ls in rec for l in ls if "@ Offset " in l), "")
            for p, lines in enumerate(rec):
                got = ["W:" + l for l in SM.warning_lines(res.events[p], res.warn[p - 1] if p else 0, text)]
                assert got == lines, (c.name, key, p, got[:3], lines[:3])
                n += len(lines)
    assert n > 1000


def test_oracle_and_reference_reproduce_the_records(harness, cases, want, decoded):
    assert "_left_out" not in want, "see the module docstring: group D"
    for c in cases:
        for key in OPTION_SETS:
            assert decoded[c.name, key]["digest"] == want[c.name]["stats"][key], ("oracle", c.name, key)
    if not harness.have_ref():
        return
    ref = harness.ref_backend()
    try:
        for c in cases:
            for key in OPTION_SETS:
                r = run_passes(harness, ref, c, key)
                assert r["digest"] == want[c.name]["stats"][key] and r["log"] == recorded_log(want[c.name], key), ("reference", c.name, key)
                assert r["dib"] == decoded[c.name, key]["dib"], (c.name, key)
    finally:
        ref.close()


# which case's check refuses which wrong model (and why)
REFUSED_BY = {"floor_division": "c_division_edges_y_gray",                 # -1031 .. -1025 would give -1 and an underflow each
              "min_from_first_sample": "d_positive_y_negative_cb",        # PreclipY.min would be the smallest sample, not 0
              "no_cap_at_10": "b_total_11",                                # the 11th event would be counted
              "cb_before_y": "b_three_events_first_counted",               # the pixel's one counted event would be Cb Underflow
              "range_check_before_truncation": "e_rgb_edges"}             # a float in (-1, 0) would count as an underflow


@pytest.mark.parametrize("flaw", sorted(REFUSED_BY))
def test_wrong_models_are_refused(flaw, decoded):
    """Each deliberately wrong variant of the model fails the check of the case built against it, and differs from the oracle on that file.
    (Floor division was tried first: it fails c_division_edges_* at -1031, where it makes -1 of -7 / 8.)"""
    import functools
    c = SC.built(REFUSED_BY[flaw]); d = decoded[c.name, "histo"]
    planes = d["planes"] if c.planes is None else None
    c.check(planes=planes)
    with pytest.raises(AssertionError):
        c.check(planes=planes, run=functools.partial(SM.run, flaw=flaw))
    res = c.model(1, planes=d["planes"], flaw=flaw, keep_pixels=False)
    assert any(SM.first_difference(got, res.records[p]) for p, got in enumerate(d["words"])), "the oracle would accept it"


def test_mcus_across_rounded_up_cannot_be_told_apart(cases):
    """The sixth variant, img_x / mcu_w rounded up in the MCU index of the shift threshold, is NOT refused by anything, and cannot be: the
    picture CalcChannelPreviewFull walks is mcu_xmax * mcu_w wide (DecodeScanImg :2871-2872), so the division is exact whatever the frame header
    says -- frames of width = 1, 15 (4:2:0) and 7 (gray) modulo the MCU width included.  The variant gives the true model's records on every
    group F file, origins at the index of the next row's first MCU included."""
    assert "mcus_across_rounded_up" in SM.FLAWS and "mcus_across_rounded_up" not in REFUSED_BY
    f = [c for c in cases if c.group == "F"]
    assert len(f) >= 5
    for c in f:
        a = c.model(1, keep_pixels=False); b = c.model(1, flaw="mcus_across_rounded_up", keep_pixels=False)
        assert all(np.array_equal(x, y) for x, y in zip(a.records, b.records)) and a.events == b.events, c.name
