"""CPU: the baseline catalogue (tests/base_cases.py, written symbol by symbol with tests/base_stream.py) holds what it claims, the
writer is deterministic, and the oracle decodes every file as the compiled reference did (tests/golden/base_cases.json, written by
tests/golden/make_base_cases.py) -- the GPU tests of tests/test_gpu_base_walks.py compare the HIP path with the oracle, so this pins
what they check to the reference itself on symbols no encoder of pictures writes."""
import json
import os

import numpy as np
import pytest

import base_cases as BC
import base_stream as BS
import prog_codec as P
from golden_util import record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "base_cases.json")


@pytest.fixture(scope="module")
def cases():
    return BC.build_all()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_census_holds(cases):
    for c in cases:
        c.check(c)
    assert all(len(c.file) < 65536 for c in cases)
    groups = {c.group for c in cases}
    assert groups == {None, "over_limit", "nosync", "overshoot", "pad_is_code"}
    big = max(BS.n_subseq(c.stream) for c in cases if c.group == "nosync")
    assert big > 2 * BC.SYNC_WG_SUBSEQ, "more sub-sequences than one k_sync workgroup holds, at 64 B and at 128 B"


def test_the_census_positions_are_where_the_codes_are(cases):
    """The census against the bytes: at every recorded position the un-stuffed data spells the recorded symbol's code."""
    for c in cases:
        s = c.stream
        codes = {key: P._codes(t) for key, t in s.tabs.items()}
        step = max(1, len(s.census) // 4000)
        for r in s.census[::step] + s.census[-3:]:
            code, ln = codes[r.tab][r.sym]
            assert ln == r.len and BS.window(s, r.pos, ln) == code, (c.name, r)


def test_the_second_level_rule_is_the_builders(cases):
    """lut2_need restates js_build_parallel_luts: the ladder of 16 lengths keeps one group of 128 entries, a table without codes longer
    than 9 bits needs none."""
    assert BS.lut2_need({(0, 0): BC.DC_LADDER, (1, 0): BC.AC_LADDER}, [(0, 0)], 1) == 256
    assert BS.lut2_need({(0, 0): BC.DC2, (1, 0): P.flat_table([0, 1], 9)}, [(0, 0)], 1) == 0
    assert BS.lut2_need({(0, 0): BC.DC2, (1, 0): P.flat_table([0, 1, 2], 10)}, [(0, 0)], 1) == 4
    same = {(cls, i): BC.AC_LADDER for cls in (0, 1) for i in range(3)}
    assert BS.lut2_need(same, [(0, 0), (1, 1), (2, 2)], 3) == 256, "identical tables of one class share a row; a DC and an AC table never do"


def test_the_files_are_the_recorded_ones(harness, cases, want):
    assert sorted(c.name for c in cases) == sorted(want)
    for c in cases:
        assert harness.hash_bytes(c.file) == want[c.name]["sha256"], c.name
    again = BC.CASES[3]()
    assert again.file == BC.built(again.name).file


def test_wellformed_means_the_reference_raised_no_error(cases, want):
    for c in cases:
        bad = want[c.name]["status"]["scan_bad"]
        assert (bad == 0) == (c.group not in ("overshoot", "pad_is_code")), (c.name, want[c.name]["status"])
        if c.wellformed:
            assert bad == 0 and want[c.name]["preview"]


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


def test_a_conforming_decoder_reads_the_intended_coefficients(cases):
    """prog_codec.decode (Annex F, written from the standard) on every case whose tokens a conforming decoder accepts."""
    n = 0
    for c in cases:
        if not c.standard:
            continue
        s = c.stream; fr = s.frame; D = P.decode(c.file); bpm = fr.mcu_blocks(); n += 1
        for bi, want in enumerate(s.coefs):
            u, j = divmod(bi, len(bpm)); comp, y, x = bpm[j]; my, mx = divmod(u, fr.mcu_x); h, v = fr.hv[comp]
            got = D.coefs[comp][my * v + y, mx * h + x]
            assert np.array_equal(got, np.array(want, np.int64).astype(np.int16)), (c.name, bi)
    assert n >= 40
