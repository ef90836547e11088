"""CPU census of tests/prog_damage_cases.py: the catalogue of damaged and irregular progressive files is what it says it is, before
tests/test_gpu_prog_damaged.py holds the kernels to it.

* every case's `check` passes: the event is in the stream where it was meant to be (scan, interval, unit, reason from the model's record);
* every stop case is flagged, and the STRICT decoder refuses it (the file really is irregular);
* every accepted case decodes its intended coefficients (the checks assert them) without a flag;
* the truth of every case but the named wide-DC ones has a baseline form (the GPU module compares pixels through it);
* six deliberately wrong readings of the damage contract are each refused by a named case;
* the random-damage set meets its share conditions, from the model alone.
"""
import time

import numpy as np
import pytest

import prog_codec as P
import prog_damage_cases as DC


@pytest.mark.parametrize("name", DC.NAMES)
def test_the_event_is_where_it_was_meant_to_be(name):
    c = DC.built(name)
    c.check(c)
    assert c.expect_flagged is not None and c.flagged == c.expect_flagged, c.record()
    assert len(c.file) < 20000
    if c.kind != "seam":
        assert c.frame.width <= 64 and c.frame.height <= 64 and all(max(q) == 1 for q in c.frame.qtabs.values())
    # the damage shows in the coefficients, or the case says that it does not (a stop where the EOB stood, an irregular script, fill bytes)
    assert all(np.array_equal(a, b) for a, b in zip(c.truth, c.clean.coefs)) == c.same_as_clean


@pytest.mark.parametrize("name", [n for n in DC.NAMES if n.startswith(("stop_", "seam_"))])
def test_the_strict_decoder_refuses_every_stop(name):
    c = DC.built(name)
    assert c.flagged and any(s["stops"] for s in c.dec.scans)
    with pytest.raises((AssertionError, KeyError, IndexError)):
        P.decode(c.file)


def test_every_stop_reason_in_every_scan_kind_and_block_position():
    """Each reason in each scan kind where it can occur, in the first, a middle and the last block of an interval."""
    seen = set()
    for c in DC.build_all():
        if c.kind != "stop":
            continue
        for i, s in enumerate(c.dec.scans):
            kind = "dc" if s["ss"] == 0 else "ac_first" if s["ah"] == 0 else "refinement"
            ri = s["dri"]
            seen |= {(kind, why, "first" if u % ri == 0 else "last" if u % ri == ri - 1 else "middle") for _iv, u, why in s["stops"]}
    want = {(k, w, p) for k, ws in (("dc", ("no_code", "dc_category")), ("ac_first", ("no_code", "run_past_se")), ("refinement", ("no_code", "refine_s")))
            for w in ws for p in ("first", "middle", "last")}
    assert want <= seen, sorted(want - seen)


def test_two_bad_intervals_share_a_wave_in_every_form():
    """k_prog_scan puts intervals [wg * per, (wg + 1) * per) into one wave (per = pg_lanes 2..16), k_prog_scan_lanes 64 neighbours."""
    a, b = DC.PAIR
    assert a != b and all(a // per == b // per for per in (2, 4, 8, 16, 64))
    for kind, scan, _n in DC.SEAM_SCANS:
        s = DC.built("seam_%s_two_bad_intervals_in_one_wave" % kind).dec.scans[scan]
        assert {iv for iv, _u, _w in s["stops"]} == {a} and {iv for iv, _u, _w in s["overran"]} == {b}


def test_interleaved_dc_stops_cover_both_rows_of_the_2x2():
    """A stop in luma block 0 or 1 of a 4:2:0 MCU has blocks of the SAME component behind it in the MCU (the second row): they stay zero."""
    names = [n for n in DC.NAMES if n.startswith("stop_dc_interleaved_") or n.startswith("seam_interleaved_")]
    assert {n.rsplit("_", 2)[1] for n in names} == {"first", "second", "fourth"}
    for pos in ("first", "middle", "last"):
        for why in ("no_code", "dc_category"):
            for nb in ("first", "second", "fourth"):
                assert "stop_dc_interleaved_%s_%s_mcu_%s_block" % (why, pos, nb) in DC.NAMES


def test_only_the_named_wide_cases_have_no_baseline_form():
    """The cap: at most the wide-DC cases (DC differences of 12..15 bits, which no sequential file codes) are compared without pixels."""
    none = sorted(c.name for c in DC.build_all() if c.base is None)
    assert none == sorted(DC.WIDE), none
    for c in DC.build_all():
        if c.base is not None:
            D = P.decode(c.base)
            assert all(np.array_equal(a, b) for a, b in zip(D.coefs, c.truth)), c.name


def test_the_catalogue_builds_quickly_and_the_same_twice():
    t = time.perf_counter()
    files = [fn().build().file for _name, fn in DC.CASES]
    assert time.perf_counter() - t < 20.0
    assert files == [c.file for c in DC.build_all()]


# variant of the model -> the catalogue case that refuses it
WRONG = {
    "stop_scan": "stop_dc_no_code_first_block",                                # the interval behind the stopped one must decode
    "discard_block": "stop_refinement_refine_s_middle_block_after_corrections_and_a_new_value",
    "refuse_dc12": "accepted_dc_category_12_al0",
    "flag_surplus": "runout_surplus_rstn_at_the_end",
    "no_flag_missing": "runout_file_cut_exactly_at_an_rstn",
    "carry_eobrun": "accepted_eobrun_32767_in_an_interval_of_3",
}


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_a_wrong_reading_of_the_contract_is_refused(variant):
    """Each wrong variant of the lenient model gives other coefficients or another flag than the truth on its named case: a decoder that
    read the contract that way fails tests/test_gpu_prog_damaged.py on that file."""
    c = DC.built(WRONG[variant])
    W = P.decode(c.file, lenient=True, variant=variant)
    same = W.flagged == c.flagged and all(np.array_equal(a, b) for a, b in zip(W.coefs, c.truth))
    assert not same
    R = P.decode(c.file, lenient=True)                                        # (and the truth is the truth again without the variant)
    assert R.flagged == c.flagged and all(np.array_equal(a, b) for a, b in zip(R.coefs, c.truth))


def test_random_damage_share_conditions():
    """From the model alone.  If these fail, the mutation mix or the seed changes, not the shares."""
    cases = DC.random_damage()
    assert len(cases) == DC.N_RANDOM == 200
    assert {c.name.split("_")[2] for c in cases} >= {"flip", "delete", "insert", "truncate", "rst"}
    flagged = sum(c.flagged for c in cases)
    far = sum(int((c.arena != c.clean_arena).any(1).sum()) > 1 for c in cases)
    assert all(c.frame.width <= 64 and c.frame.height <= 64 for c in cases)
    assert 4 * flagged >= 3 * len(cases), flagged
    assert 4 * far >= len(cases), far
