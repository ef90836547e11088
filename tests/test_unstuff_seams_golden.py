"""CPU: the inputs of the un-stuffing seam tests (tests/unstuff_inputs.py) really put their bytes where the tests need them, and the oracle decodes
every one of them as the compiled reference did (tests/golden/unstuff_seams.json, written by tests/golden/make_unstuff_seams.py).

The GPU tests (tests/test_gpu_unstuff_seams.py) compare the HIP path with the oracle on these files; this module pins the oracle to the reference
on the same files, and asserts the census conditions -- restart markers and stuffed bytes split over a 4 KiB and a 16 KiB seam in all four
positions, all 16 scan-start phases, scans ending on, before and behind a grid line, interval tables with one entry to spare / exactly full / one
short -- so that a change of the generator fails here instead of quietly losing the coverage."""
import json
import os

import pytest

import unstuff_inputs as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unstuff_seams.json")


@pytest.fixture(scope="module")
def cases(harness):
    return U.all_inputs(harness)


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_census_counts_what_a_byte_walk_counts(harness):
    """The numpy census against a byte-at-a-time walk of the same rules, on a restart-rich file under three pads."""
    base = harness.synth_jpeg(width=640, height=480, restart_interval=1, quality=95, seed=9)
    for k in (0, 7, 11):
        d = U.pad_header(base, k)
        p = harness.parse_jpeg(d)
        assert (p.scan_start, p.scan_end) == U.scan_range(d) and p.scan_start == harness.parse_jpeg(base).scan_start + 16 + k
        c = U.census(d)
        phase = p.scan_start & 15
        slow = {P: [0, 0, 0, 0] for P in U.PERIODS}
        for i in range(p.scan_start, p.scan_end - 1):
            if d[i] != 0xFF:
                continue
            g, nx = i - p.scan_start + phase, d[i + 1]
            for P in U.PERIODS:
                if (g + 1) % P == 0 and nx == 0:
                    slow[P][0] += 1
                if (g + 1) % P == 0 and 0xD0 <= nx <= 0xD7:
                    slow[P][1] += 1
                if (g + 2) % P == 0 and 0xD0 <= nx <= 0xD7 and i + 2 < p.scan_end:
                    slow[P][2] += 1
                if g % P == 0 and g and 0xD0 <= nx <= 0xD7:
                    slow[P][3] += 1
        assert c["phase"] == phase and c["scan_len"] == p.scan_end - p.scan_start
        for P in U.PERIODS:
            assert c[str(P)] == slow[P], (k, P)
        assert sum(slow[16]) > 100 and sum(slow[1024]) > 0                # the walk itself saw seams


def test_padding_moves_the_scan_and_nothing_else(harness, oracle):
    import numpy as np
    base = harness.synth_jpeg(**U.END_KW)
    harness.drive(oracle, base)
    dib, coefs = oracle.dib(), harness.oracle_coefs(oracle)
    for k, d in enumerate(U.end_all_pads(harness).values()):
        assert len(d) == len(base) + 16 + k
        harness.drive(oracle, d)
        assert np.array_equal(oracle.dib(), dib) and np.array_equal(harness.oracle_coefs(oracle), coefs), k


def test_the_seam_conditions_hold(harness):
    U.check_seam_set(U.seam_set(harness))
    U.check_plain_set(U.plain_set(harness))
    U.check_end_set(U.end_set(harness))
    U.check_tiny_set(U.tiny_set(harness))
    U.check_count_set(U.count_set(harness))
    U.check_edge_set(U.edge_set(harness))
    U.check_damaged_set(harness, U.damaged_set(harness))


def test_a_file_without_the_seams_fails_the_conditions(harness):
    """The conditions bite: the same picture under another seed, or under fewer pads, does not pass them."""
    other = harness.synth_jpeg(**dict(U.SEAM_KW, seed=6, width=320, height=240))
    with pytest.raises(AssertionError):
        U.check_seam_set({k: U.pad_header(other, k) for k in U.PADS})
    few = dict(list(U.seam_set(harness).items())[:8])
    with pytest.raises(AssertionError):
        U.check_seam_set(few)
    with pytest.raises(AssertionError):
        U.check_end_set({"end_p%02d" % k: U.pad_header(harness.synth_jpeg(**dict(U.END_KW, seed=122)), k) for k in U.END_PADS})
    with pytest.raises(AssertionError):
        U.check_edge_set({k: U.set_dri(v, 2) for k, v in U.edge_set(harness).items()})


def test_the_files_are_the_recorded_ones(harness, cases, want):
    assert sorted(cases) == sorted(want)
    for name, data in cases.items():
        assert harness.hash_bytes(data) == want[name]["sha256"], name
        assert U.census(data) == want[name]["census"], name
    assert len({r["sha256"] for r in want.values()}) == len(want)


def test_the_records_pin_the_edges(want):
    """What the records must show for the tests built on them to mean anything."""
    for prefix in ("seam_p", "plain_p", "tiny_gray8_p", "tiny_c420_16_p", "end_"):
        rs = [r for k, r in want.items() if k.startswith(prefix)]
        assert len(rs) >= 4 and len({(r["dib"], tuple(r["planes"]), tuple(r["blk_dc"])) for r in rs}) == 1, prefix     # pads change no pixel
        assert len({r["mcu_map"] for r in rs}) == len(rs) == 16 + (prefix == "end_"), prefix                            # ... and every file position (end_: the unpadded file too)
    for n, read in ((54, 53), (57, 56), (58, 57)):
        st = want["edge_%d" % n]["status"]
        assert st["restart_read"] == read and st["scan_bad"] == 0 and st["scan_end"] == 0, n       # the reference follows every marker of the stream
    assert all(r["status"]["scan_bad"] == 0 for k, r in want.items() if not k.startswith("bad_"))
    assert len({r["dib"] for k, r in want.items() if k.startswith("bad_")}) >= 10                    # the damages differ in what they do


def test_oracle_and_reference_reproduce_the_records(harness, cases, want):
    backends = [harness.oracle_backend()] + ([harness.ref_backend()] if harness.have_ref() else [])
    try:
        for b in backends:
            for name, data in sorted(cases.items()):
                got = U.record(harness, b, data)
                got["census"] = want[name]["census"]
                assert got == want[name], (b.name, name)
    finally:
        for b in backends:
            b.close()
