"""CPU: the batch statistics catalogue (tests/batch_stats_cases.py) holds what it claims -- every claim proven from the plain numpy model of
tests/stats_model.py on the planes the oracle decoded --, the model equals the oracle word for word on every file and under every option set, and
the oracle's records are the compiled reference's (tests/golden/batch_stats_cases.json, written by tests/golden/make_batch_stats_cases.py).  The GPU
test of tests/test_gpu_batch_stats.py compares jsnoop_batch_pack_stats with the oracle on these files, so this pins what it checks to the reference and
to arithmetic anyone can read."""
import json
import os
import re

import numpy as np
import pytest

import batch_stats_cases as BC
import stats_model as SM
from stats_cases_util import OPTION_SETS, explain, run_passes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "batch_stats_cases.json")
CSRC = os.path.join(HERE, "..", "jpegsnoop_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    return BC.build_all()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def decoded(harness, oracle, cases):
    """{(case, option set): run_passes of the oracle}, once for the module."""
    return {(c.name, key): run_passes(harness, oracle, c, key, keep=True) for c in cases for key in OPTION_SETS}


def _model(c, decoded, key="histo"):
    return c.model(OPTION_SETS[key][1], planes=decoded[c.name, key]["planes"])


def test_the_constants_are_the_kernels():
    """UNIT, WAVES, ORDER_STEP and ORDER_ROWS restate the deal of k_stats_batch and the steps of k_stats_order: read them back from the source, at the
    lines the catalogue's docstring names."""
    types = open(os.path.join(CSRC, "jsnoop_types.h")).read().split("\n")
    src = open(os.path.join(CSRC, "jsnoop_stats.hip")).read().split("\n")
    doc = BC.__doc__
    at = lambda name: [int(x) for x in re.search(r"%s\s.*\((.*)\)" % name, doc).group(1).replace("jsnoop_types.h", "").replace("jsnoop_stats.hip", "").replace(":", " ").split() if x.isdigit()]
    assert "#define JS_STATS_UNIT %du" % BC.UNIT in types[at("UNIT")[0] - 1]
    assert "JS_STATS_UNIT + lane * 8u" in src[at("UNIT")[1] - 1] and BC.UNIT == 64 * 8
    assert "#define SB_WAVES   (SB_THREADS / 64)" in src[at("WAVES")[0] - 1] and "u += SB_WAVES" in src[at("WAVES")[1] - 1]
    assert "x0 += 64u" in src[at("ORDER_STEP")[0] - 1] and BC.ORDER_STEP == 64
    assert "#define SB_THREADS 256" in src[at("ORDER_ROWS")[0] - 1] and "base += SB_THREADS" in src[at("ORDER_ROWS")[1] - 1]
    assert BC.WAVES == 256 // 64 and BC.ORDER_ROWS == 256


def test_every_check_holds(cases, decoded):
    for c in cases:
        r = c.check(planes=decoded[c.name, "histo"]["planes"] if c.planes is None else None)
        if c.group == "S":
            BC.check_seam(c, r)
        if "rows_of_counted" in c.claims:
            assert sorted({e[0] // c.img_x for e in r.events[0]}) == c.claims["rows_of_counted"], (c.name, [e[0] for e in r.events[0]])
        if c.claims.get("events_some"):
            assert 10 < r.found[0] < c.npix and len(set(r.records[0][37:43].tolist())) > 1, (c.name, r.found)
    assert {c.group for c in cases} == set("SLOM")
    assert all(c.img_x <= 2 * BC.UNIT + 8 and 8 <= c.img_y <= 32 for c in cases)
    s = [c for c in cases if c.group == "S"]
    assert {(c.layout, c.img_x) for c in s} == {(l, w) for l in ("gray", "444") for w in (8, BC.UNIT - 8, BC.UNIT, BC.UNIT + 8, 2 * BC.UNIT + 8)}
    assert sum("unit1_lane0" in c.claims["seam"] for c in s) == 4
    assert {(c.layout, c.width) for c in cases if c.group == "L"} == {(l, w) for l in ("420", "422", "440") for w in (16, BC.UNIT + 16)}


def test_order_and_budget_reach_the_seams_of_k_stats_order(cases, decoded):
    """From the model's events alone: where the 10th counted event lies, and where the first one that is no longer counted."""
    o = {c.name: (c, _model(c, decoded)) for c in cases if c.group == "O"}
    seen = set()
    for name, (c, r) in o.items():
        q = r.pix[0]; W = c.img_x
        per = ((q.clipv > 255) | (q.clipv < 0)).sum(0)
        assert r.found[0] == int(per.sum()) >= 10 and r.warn[0] == 10 and len(r.events[0]) == 10
        tenth = r.events[0][-1][0]
        behind = np.flatnonzero(per); behind = behind[behind > tenth]
        nxt = int(behind[0]) if len(behind) else None                     # the pixel of the first event that is not counted (or the 10th's own)
        if r.found[0] == 10:
            seen.add("exactly 10")
        if r.found[0] == 11:
            seen.add("11")
        if tenth % W == W - 1:
            seen.add("10th on the last pixel of a row")
        if tenth % W == 0:
            seen.add("10th on the first pixel of a row")
        if len({e[0] // W for e in r.events[0]}) == 10 and nxt is not None and nxt // W not in {e[0] // W for e in r.events[0]}:
            seen.add("one event a row")
        if {e[0] // W for e in r.events[0]} == {c.img_y - 1} and not per[:(c.img_y - 1) * W].any():
            seen.add("all in the last row")
        if nxt is not None and nxt // W == tenth // W and (nxt % W) // BC.UNIT != (tenth % W) // BC.UNIT:
            seen.add("10th and 11th in two units of one row")
        if (tenth % W) // BC.UNIT == 1 and sum(1 for e in r.events[0] if e[0] // W == tenth // W and (e[0] % W) < BC.UNIT) == 9:
            seen.add("10th in the second unit")
        if nxt is not None and nxt // W == tenth // W and (nxt % W) // BC.ORDER_STEP == (tenth % W) // BC.ORDER_STEP + 1 and tenth % W % BC.ORDER_STEP == BC.ORDER_STEP - 1:
            seen.add("10th and 11th on both sides of a walk step")
        if tenth % W % BC.ORDER_STEP == 0 and tenth % W:
            seen.add("10th on the first pixel of a walk step")
        if per[tenth] == 3 and sum(1 for e in r.events[0] if e[0] == tenth) in (1, 2):
            seen.add("inside a pixel of three events, %d counted" % sum(1 for e in r.events[0] if e[0] == tenth))
    assert seen == {"exactly 10", "11", "10th on the last pixel of a row", "10th on the first pixel of a row", "one event a row", "all in the last row",
                    "10th and 11th in two units of one row", "10th in the second unit", "10th and 11th on both sides of a walk step",
                    "10th on the first pixel of a walk step", "inside a pixel of three events, 1 counted", "inside a pixel of three events, 2 counted"}, sorted(seen)


def test_the_small_pictures_differ_from_their_neighbours(cases, decoded):
    """About 200 pictures of one or a few units: each with levels of its own, every third with events -- a flush into a neighbour's row changes a word."""
    m = [c for c in cases if c.group == "M"]
    assert len(m) == BC.SMALL >= 190 and {(c.img_x, c.img_y) for c in m} == {(8, 8), (16, 16)}
    assert {c.layout for c in m} == {"gray", "444", "420", "422"}
    recs = [decoded[c.name, "histo"]["words"][0] for c in m]
    clip = [decoded[c.name, "clip"]["words"][0] for c in m]
    for k in range(1, len(m)):
        assert not np.array_equal(recs[k][:36], recs[k - 1][:36]) and not np.array_equal(recs[k][434:], recs[k - 1][434:]), m[k].name
    with_events = [k for k in range(len(m)) if recs[k][37:43].any()]
    assert with_events == list(range(0, len(m), 3)) and all(clip[k][37:43].sum() == 10 for k in with_events)
    assert {int(np.flatnonzero(recs[k][37:43])[0]) for k in with_events} == {0, 1, 2, 3, 4, 5}, "every kind of range event"
    assert all(int(recs[k][36]) == m[k].npix for k in range(len(m)))


def test_the_model_is_the_oracle_on_the_catalogue(cases, decoded):
    """model(oracle.planes(), ...) == oracle.color_stats(), word for word: bHistoEn, bStatClipEn alone, Full IDCT and DC only."""
    errs = []
    for c in cases:
        for key, (_opt, histo_en) in OPTION_SETS.items():
            d = decoded[c.name, key]
            res = c.model(histo_en, planes=d["planes"], keep_pixels=False)
            e = explain(c, key, 0, d["words"][0], res)
            if e:
                errs.append(e)
            if c.planes is not None:
                assert all(np.array_equal(d["planes"][k], c.planes[k]) for k in range(c.ncomp)), (c.name, key, "an all-DC file decodes to its levels")
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:20]))


def test_oracle_and_reference_reproduce_the_records(harness, cases, want, decoded):
    assert sorted(c.name for c in cases) == sorted(want)
    for c in cases:
        assert harness.hash_bytes(c.file) == want[c.name]["sha256"], c.name
        for key in OPTION_SETS:
            assert decoded[c.name, key]["digest"][0] == want[c.name]["stats"][key], ("oracle", c.name, key)
    again = BC.CASES[3]()
    assert again.file == cases[3].file
    if not harness.have_ref():
        return
    ref = harness.ref_backend()
    try:
        for c in cases:
            for key in OPTION_SETS:
                r = run_passes(harness, ref, c, key)
                assert r["digest"][0] == want[c.name]["stats"][key] and r["dib"] == decoded[c.name, key]["dib"], ("reference", c.name, key)
    finally:
        ref.close()


def test_a_wrong_kind_order_or_a_missing_cap_is_refused(decoded):
    """Two deliberately wrong variants of the model (stats_model.FLAWS) against the order cases: they differ from the oracle where the name says."""
    for flaw, name in (("cb_before_y", "o_three_events_entered_with_9_used"), ("no_cap_at_10", "o_total_11")):
        c = BC.built(name); d = decoded[c.name, "histo"]
        res = c.model(1, planes=d["planes"], flaw=flaw, keep_pixels=False)
        assert SM.first_difference(d["words"][0], res.records[0]) is not None, (flaw, name)
