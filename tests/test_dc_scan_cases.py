"""CPU: the DC scan catalogue (tests/dc_scan_cases.py) holds what it claims, the writer is deterministic, the plain numpy MODEL of the DC
predictors (running int16 sums of the dequantised differences, zeroed at restarts) reproduces the oracle's decode of every file, and the
oracle decodes every file as the compiled reference did (tests/golden/dc_scan_cases.json, written by tests/golden/make_dc_scan_cases.py).
The GPU tests of tests/test_gpu_dc_scan.py compare k_dc_scan / k_dc_scan_parts with the oracle on these files, so this pins what they
check to the reference and to arithmetic anyone can read."""
import json
import os

import numpy as np
import pytest

import dc_scan_cases as DC
from golden_util import record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_scan_cases.json")


@pytest.fixture(scope="module")
def cases():
    return DC.build_all()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_parts_formula():
    """`per` and the part count of k_dc_scan_parts, restated in parts_of, against values worked out by hand: per = the MCUs of 1/64 of
    the image rounded up to whole steps of 1024."""
    assert DC.parts_of(1024) == (1024, 1, 1024)
    assert DC.parts_of(1025) == (1024, 2, 1)
    assert DC.parts_of(65536) == (1024, 64, 1024)           # 65536 / 64 = 1024: one step per part, every part in use
    assert DC.parts_of(65537) == (2048, 33, 1)              # ceil(65537 / 64) = 1025 MCUs: two steps; 32 * 2048 = 65536 MCUs in front of the last
    assert DC.parts_of(65792) == (2048, 33, 256)            # 257 x 256 MCUs: 65792 - 65536


def test_every_check_holds(cases):
    for c in cases:
        c.check()
    assert {c.group for c in cases} == set("ABCDE")
    assert {c.layout for c in cases if c.nmcu >= 1025} == set(DC.LAYOUTS), "every layout past one step"
    assert {c.layout for c in cases if c.group == "A" and c.nmcu == 2049} >= {"luma4x2", "all4x4"}
    assert DC.BLOCKS["all4x4"] == DC.MAX_BLK_PER_MCU and DC.BLOCKS["luma4x2"] > 6, "the generic instance, at its first layout and at its largest"
    assert {c.nmcu for c in cases if c.group == "A"} == {63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3 * 1024 + 1}
    for n in {c.nmcu for c in cases if c.group == "A"}:
        assert 0 in {c.dri for c in cases if c.group == "A" and c.nmcu == n}
    assert {c.dri for c in cases if c.group == "A"} >= {0, 1, 63, 64, 65, 1023, 1024, 1025} and any(c.dri == c.nmcu - 1 for c in cases if c.group == "A")
    assert {q for c in cases for q in c.q[:min(c.frame.ncomp, 2)]} >= {1, 37, 255, 4099}
    big = [c for c in cases if c.nmcu > 65536]
    assert all(c.per == 2048 for c in big) and all(c.per == 1024 for c in cases if c.nmcu <= 65536)
    assert {c.group for c in big} == {"C", "D"} and {c.dri for c in big} == {0, 2048, 2047, 2049, 1024, 64000}
    assert {c.last_part for c in big} == {256, 1, 1025} and all(c.layout in ("gray", "444") for c in big)
    assert sum(1 for c in cases if c.group == "E") >= 3


def test_the_writer_is_deterministic_and_the_files_are_the_recorded_ones(harness, cases, want):
    assert sorted(c.name for c in cases) == sorted(want)
    for c in cases:
        assert harness.hash_bytes(c.file) == want[c.name]["sha256"], c.name
    for i in (3, 12, len(cases) - 1):
        again = DC.CASES[i]()
        assert again.file == cases[i].file and again.name == cases[i].name


def test_the_reference_met_every_marker_and_no_error(cases, want):
    for c in cases:
        st = want[c.name]["status"]
        assert st["scan_bad"] == 0 and st["restart_read"] == c.markers and want[c.name]["preview"], (c.name, st)


def test_the_model_is_the_oracle(harness, oracle, cases):
    """One-component files: the oracle's block-DC map is one value per block -- compared whole.  Sub-sampled frames keep the reference's
    replication there (Y[0, 1] of a 4:2:0 file holds the MCU's block 2), so the model is tied to the oracle through the int16 planes:
    the top-left sample of every block is what SetFullRes makes of a block that holds only that cumulative DC -- the IDCT output of such
    a block (oracle.idct_block; the sum leaves the DC term out, so it is zero) times 8, truncated, plus the predictor."""
    shift = {}
    for dc in (-32768, -1, 0, 1, 255, 32767):
        blk = np.zeros(64, np.int16); blk[0] = dc
        f = oracle.idct_block(blk); shift[dc] = int(np.int16(np.int32(f[0] * 8)))
        assert not f.any(), "the IDCT of a DC-only block"
    assert set(shift.values()) == {0}
    errs = []
    for c in cases:
        harness.drive(oracle, c.file)
        cum, _ = DC.model(c)
        assert oracle.status()["scan_bad"] == 0 and oracle.status()["restart_read"] == c.markers, c.name
        planes = oracle.planes()
        if c.frame.ncomp == 1:
            e = DC.first_block_difference(c, 0, oracle.blk_dc()[0].ravel(), cum[0])
            if e:
                errs.append("block-DC map, " + e)
        for comp, (rows, cols, vals) in enumerate(DC.planes_corner(c, cum)):
            e = DC.first_block_difference(c, comp, planes[comp][rows, cols], vals)
            if e:
                errs.append("plane, " + e)
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:20]))


def test_oracle_and_reference_reproduce_the_records(harness, cases, want):
    backends = [harness.oracle_backend()] + ([harness.ref_backend()] if harness.have_ref() else [])
    try:
        for b in backends:
            for c in cases:
                harness.drive(b, c.file)
                r = record(harness, b)
                if b.name == "oracle":
                    r["coefs"] = harness.hash_bytes(harness.oracle_coefs(b))
                for k, v in r.items():
                    assert v == want[c.name][k], (b.name, c.name, k)
    finally:
        for b in backends:
            b.close()
