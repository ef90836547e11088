"""CPU: tests/export_opt_model.py, the definition of the export with optimal Huffman tables.

K.2 the kernel's way (a group id per symbol, no OTHERS chains) gives prog_codec.optimal_table's answer on every table of the content catalogue and on
2000 seeded random frequency sets; the model's file is read by three decoders that share nothing with it as the same coefficients, and by libjpeg as the
same pixels as the Annex K export of the same input; its tables and entropy-coded segment are prog_codec.encode_baseline's, a second derivation of the
counts; on the content cases of tests/export_cases.py it is no longer than the Annex K file; every case of tests/export_opt_cases.py holds its claim,
and four wrong readings of the definition are each refused by a named case."""
import io

import numpy as np
import pytest

import coef_model as CM
import export_cases as X
import export_model as EM
import export_opt_cases as XO
import export_opt_model as OM
import prog_codec as PC
from test_export_model import LAYOUTS, SIZES, random_frame

CASES = XO.cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


# ------------------------------------------------------------------------------------------------ K.2 by group ids against the chains
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_group_id_k2_is_the_chains_on_every_table_of_the_catalogue_and_the_case_holds_its_claim(case):
    XO.check_census(case)
    _T, freq, tabs, f = case.model()
    for slot in range(2):
        assert OM.group_k2(freq[slot]) == PC.optimal_table(freq[slot]) == tabs[slot], slot
        counts, syms = tabs[slot]
        assert sum(counts) == len(syms) == len(freq[slot]) and sum(n << (16 - ln) for ln, n in enumerate(counts, 1)) < 1 << 16      # a prefix code, a point to spare
    if case.nblocks <= 700:
        D = PC.decode(f)
        assert D.sof == 0xC0 and np.array_equal(D.coefs[0], case.coefs[0])


def test_group_id_k2_is_the_chains_on_2000_random_frequency_sets():
    rng = np.random.default_rng(20261020)
    depth = 0
    for i in range(2000):
        n = 256 if i < 8 else 1 + int(255 * rng.random() ** 3)      # 1 .. 256 symbols (the 257th is the reserved one), small sets more often: the chains are slow
        syms = rng.choice(256, n, replace=False)
        kind = i % 4                                      # small counts with many ties, wide counts, geometric counts (deep trees), all equal
        if kind == 0:
            cnt = rng.integers(1, 4, n)
        elif kind == 1:
            cnt = rng.integers(1, 1 << 32, n)
        elif kind == 2:
            cnt = np.maximum(1, (1.7 ** rng.permutation(n).clip(0, 40)).astype(np.int64) + rng.integers(0, 2, n))
        else:
            cnt = np.full(n, int(rng.integers(1, 1000)))
        freq = {int(s): int(c) for s, c in zip(syms, cnt)}
        want = PC.optimal_table(freq)
        assert OM.group_k2(freq) == want, (i, freq)
        depth = max(depth, max(OM.group_codesizes(freq).values()))
    assert depth > 16, "no set reached Adjust_BITS"


WRONG = {"ties taken smallest symbol first": (dict(ties_largest_first=False), "three_symbols_of_equal_count"),
         "no reserved code point": (dict(reserve=False), "two_symbols_of_equal_count"),
         "Adjust_BITS skipped": (dict(adjust=False), "fibonacci_17"),
         "symbols ordered by final length": (dict(order_by_final=True), "fibonacci_20")}


@pytest.mark.parametrize("reading", list(WRONG))
def test_a_wrong_reading_of_the_definition_is_refused_by_its_case(reading):
    kw, name = WRONG[reading]
    _T, freq, tabs, _f = BY_NAME[name].model()
    assert OM.group_k2(freq[1]) == tabs[1]
    got = OM.group_k2(freq[1], **kw)
    assert got != tabs[1] and PC._dht(1, 0, got) != PC._dht(1, 0, tabs[1]), reading


# ------------------------------------------------------------------------------------------------ the file
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_three_decoders_read_the_optimal_file_and_libjpeg_sees_the_annex_k_pixels(harness, oracles, layout, size):
    from PIL import Image
    w, h = size
    f, coefs = random_frame(layout, w, h, seed=int(layout, 10) + w if layout != "grey" else 9000 + w)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    res, detail, data, freq, tabs = OM.export_parts(arena, dccum, geo, w, h, qnat)
    assert (res, detail) == (OM.OK, 0) and len(tabs) == (2 if layout == "grey" else 4)
    _, _, annex = EM.export_file(arena, dccum, geo, w, h, qnat)
    first = annex.index(b"\xFF\xC4")
    assert data[:first] == annex[:first] and data != annex
    D = PC.decode(data)
    assert D.sof == 0xC0 and (D.frame.width, D.frame.height) == (w, h) and D.frame.hv == f.hv
    for c in range(f.ncomp):
        assert np.array_equal(D.coefs[c], coefs[c]), c
    full, dc = oracles
    p = harness.drive(dc, data)
    assert CM.geometry_of(p).hv == geo.hv and np.array_equal(CM.cum_from_planes(dc.planes(), geo), dccum)
    harness.drive(full, data)
    assert np.array_equal(harness.oracle_coefs(full)[:, 1:], arena[:, 1:])
    a = Image.open(io.BytesIO(data)); a.load(); b = Image.open(io.BytesIO(annex)); b.load()
    assert a.size == (w, h) and a.mode == b.mode and a.tobytes() == b.tobytes()
    _, _, bare = OM.export_file(arena, dccum, geo, w, h, qnat, jfif=False)
    assert bare == data[:2] + data[20:]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_tables_and_entropy_segment_are_encode_baselines(layout):
    """Two derivations of the counts: prog_codec.encode_baseline from the coefficients, the model from arena, dccum and multipliers."""
    f, coefs = random_frame(layout, 72, 40, seed=7)
    ref = PC.encode_baseline(f, coefs)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    res, _, data, freq, tabs = OM.export_parts(arena, dccum, geo, 72, 40, qnat)
    assert res == OM.OK
    a, b = ref.index(b"\xFF\xC4"), data.index(b"\xFF\xC4")
    assert ref[a:] == data[b:]
    for s, t in enumerate(tabs):
        assert PC._dht(s & 1, s >> 1, t) in ref[a:a + 900]


def test_the_counters_limit_is_host_arithmetic():
    class Geo:                                            # (nothing but the block count is read before the refusal)
        nblocks = OM.MAX_BLOCKS
    assert OM.export_file(None, None, Geo, 8, 8, None) == (OM.UNSUPPORTED, 0, None)
    assert 63 * (OM.MAX_BLOCKS - 1) < 1 << 32


SMALL = [c for c in X.cases() if c.nblocks <= 600]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_on_the_content_cases_the_optimal_file_is_no_longer_than_the_annex_k_file(case):
    """Asserted on these inputs only: K.2 with Adjust_BITS is not provably optimal under the 16-bit limit, so this is no universal claim."""
    arena, dccum, geo, qnat = case.inputs()
    annex = case.model()[4]
    res, _, data = OM.export_file(arena, dccum, geo, case.frame.width, case.frame.height, qnat)
    assert res == OM.OK and len(data) <= len(annex), (len(data), len(annex))
    assert np.array_equal(PC.decode(data).coefs[0], PC.decode(annex).coefs[0])
