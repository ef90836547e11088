"""CPU: the damaged-file catalogue (tests/side_report_cases.py) holds what it claims -- every event lies at the seam its name says,
proved from the writer's census --, the files are the recorded ones, the oracle decodes every file as the compiled reference did
(tests/golden/side_report_cases.json, written by tests/golden/make_side_report_cases.py), the reference itself (where it is built)
still writes the recorded log, and EVERY case is flagged by the reference: tests/test_gpu_side_report.py compares the HIP path's
report with these records and has no case to skip."""
import collections
import json
import os

import pytest

import base_stream as BS
import side_report_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_report_cases.json")


@pytest.fixture(scope="module")
def cases():
    return SC.build_all()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_check_holds(cases):
    for c in cases:
        c.check(c)
    assert all(len(c.file) < 65536 for c in cases) and 80 <= len(cases) <= 120
    per = collections.Counter(c.group for c in cases)
    assert set(per) == set(SC.GROUPS), per
    geo = {(c.stream.frame.ncomp, len(c.stream.frame.mcu_blocks()), SC.chunk_mcus(SC.nmcu_of(c.stream))) for c in cases if c.group == "where"}
    assert geo == {(1, 1, 4), (3, 6, 4), (3, 18, 4), (1, 1, 5)}, "gray, 4:2:0, luma 4x4, and the image of more than 32768 MCUs (chunks of five)"
    assert any(SC.nmcu_of(c.stream) % 4 == 1 for c in cases if c.group == "where"), "a last chunk of one MCU"
    modes = collections.Counter(c.mode for c in cases)
    assert modes[1] >= 6 and modes["not1"] >= 9 and modes[2] == 1 and modes[3] == 1
    assert {c.stream.dri for c in cases if c.group == "restart"} >= {1, 3, 4, 5, 7}


def test_the_thresholds_are_the_codes(cases):
    """The constants the catalogue restates, read from the sources."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jpegsnoop_amd", "csrc")
    with open(os.path.join(src, "jsnoop_types.h")) as f:
        assert "#define JS_ANOM_MAX %d " % SC.JS_ANOM_MAX in f.read()
    with open(os.path.join(src, "jsnoop_parallel.cpp")) as f:
        text = f.read()
    assert text.count("+ %du >= (uint64_t)" % SC.LOOK_AHEAD) == 2, "the look-ahead threshold of js_side_only, at the scan end and at an interval end"
    assert "std::max<uint32_t>(4u, (nmcu + 8191u) / 8192u)" in text and "std::min<uint32_t>(im.err_max, 64u) + 32u" in text


def test_literal_bits_are_written_where_the_census_says():
    s = SC.make(SC.BC.gray(3, 1), {1: [(1, 1), (BS.BITS, (0b1011, 4)), (0, 0)]})
    r = next(r for r in s.census if r.sym == BS.BITS)
    assert (r.blk, r.k, r.tab, r.len, r.size) == (1, 1, None, 0, 4) and BS.window(s, r.pos, 4) == 0b1011 and s.coefs[1] is None and s.coefs[0] is not None


def test_the_files_are_the_recorded_ones(harness, cases, want):
    assert sorted(c.name for c in cases) == sorted(want)
    for c in cases:
        assert harness.hash_bytes(c.file) == want[c.name]["sha256"], c.name
        assert sorted(want[c.name]["runs"]) == sorted(str(e) for e in c.err_max), c.name
        assert (c.clean is not None) == ("clean_status" in want[c.name]), c.name
    again = SC.CASES[5]()
    assert again.file == cases[5].file


def test_every_case_is_flagged_by_the_reference(cases, want):
    """Its recorded status differs from a clean decode's (the undamaged file's, recorded beside it), or its section holds a message."""
    for c in cases:
        for em, r in want[c.name]["runs"].items():
            msgs = SC.messages(r["section"])
            clean = want[c.name].get("clean_status")
            assert msgs or (clean is not None and r["status"] != clean), (c.name, em)
            assert r["section"][0].endswith(SC.FIRST) and SC.LAST in r["section"][-1] and r["preview"]
        if c.clean is None:
            assert all(SC.messages(r["section"]) for r in want[c.name]["runs"].values()), c.name
        for k, v in c.status.items():
            assert all(r["status"][k] == v for r in want[c.name]["runs"].values()), (c.name, k)


def test_the_counter_cuts_inside_a_blocks_three_lines(cases, want):
    """The err_max variants of the counter files really differ, and the cut falls inside a failing block's lines in a later chunk."""
    for c in cases:
        if c.group != "counter":
            continue
        runs = want[c.name]["runs"]
        n = {int(em): len(SC.messages(r["section"])) for em, r in runs.items()}
        assert len(set(n.values())) >= len(n) - 2 and all(runs[str(em)]["status"]["warn_bad"] == min(em, max(r["status"]["warn_bad"] for r in runs.values())) for em in n), (c.name, n)


def test_oracle_and_reference_reproduce_the_records(harness, cases, want):
    backends = [harness.oracle_backend()] + ([harness.ref_backend()] if harness.have_ref() else [])
    try:
        for b in backends:
            for c in cases:
                for em in c.err_max:
                    r = SC.run(harness, b, c.file, em, log=b.name != "oracle")
                    for k, v in r.items():
                        assert v == want[c.name]["runs"][str(em)][k], (b.name, c.name, em, k)
                if c.clean is not None and b.name != "oracle":
                    assert SC.run(harness, b, c.clean, 20)["status"] == want[c.name]["clean_status"], c.name
    finally:
        for b in backends:
            b.set_options(); b.close()
