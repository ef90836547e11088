"""CPU pins of tests/prog_codec.py -- the plain Annex F / G codec that is the only reference answer the progressive (SOF2) kernels
have (tests/test_gpu_progressive_forms.py) -- and the census of tests/prog_cases.py.

The codec is held from four sides before anything on the GPU trusts it:
* its decoder inverts its encoder on every catalogue file (coded blocks);
* its decoder reads libjpeg-turbo's progressive and baseline files of one picture (tests/golden/pillow) to the same coefficients;
* its baseline writer, decoded by the project's own oracle, gives the dequantised truth;
* the repository's C generator (oracle/jpeg_synth.c) agrees with its decoder, progressive against baseline form;
* libjpeg (through Pillow, where present) reads every catalogue file to the pixels of the baseline form of its truth.

The LENIENT mode of the decoder (decode(file, lenient=True): the truth for damaged files, tests/prog_damage_cases.py) is held from two:
* on every well-formed file it is the strict mode, with nothing on its record;
* where libjpeg tolerates the damage the way the contract does, libjpeg reads the damaged file to the pixels of the baseline form of
  the lenient truth.
"""
import io
import json
import os

import numpy as np
import pytest

import prog_cases as PC
import prog_codec as P

HERE = os.path.dirname(os.path.abspath(__file__))
PIL_DIR = os.path.join(HERE, "golden", "pillow")
PILLOW = json.load(open(os.path.join(PIL_DIR, "manifest.json")))["cases"]


def same_on_coded_blocks(frame, a, b):
    for c in range(frame.ncomp):
        m = frame.coded_mask(c)
        if not np.array_equal(a[c][m], b[c][m]):
            by, bx, k = [int(x) for x in np.argwhere((a[c] != b[c]) & m[..., None])[0]]
            return "component %d block (%d, %d) zig-zag %d: %d against %d" % (c, by, bx, k, a[c][by, bx, k], b[c][by, bx, k])
    return None


@pytest.mark.parametrize("name", PC.NAMES)
def test_decode_inverts_encode_and_the_census_holds(name):
    c = PC.built(name)
    assert c.dec.sof == 0xC2 and len(c.dec.scans) == len(c.script)
    assert same_on_coded_blocks(c.frame, c.truth, c.coefs) is None
    assert all(s["overrun"] == 0 for s in c.dec.scans)
    D = P.decode(c.base)                                              # the baseline form carries the truth, padding blocks included
    assert D.sof == 0xC0 and all(np.array_equal(a, b) for a, b in zip(D.coefs, c.truth))
    assert c.check is not None
    c.check(c)


@pytest.mark.parametrize("name", ["eobrun_lengths", "refinement_stretches_and_zrl", "eobrun_32767_then_a_shorter_one_and_long_scans"])
def test_census_fails_without_the_crafted_coefficients(name):
    """The census is no formality: the same frame and script over plain noise does not pass it."""
    c = PC.CASES[PC.NAMES.index(name)]()
    c.coefs = PC.noise(c.frame, 5, density=0.2)
    c.build()
    with pytest.raises(AssertionError):
        c.check(c)


def test_catalogue_is_deterministic():
    c = PC.CASES[PC.NAMES.index("geometry_4x2")]().build()
    assert c.file == PC.built("geometry_4x2").file


@pytest.mark.parametrize("c", PILLOW, ids=lambda c: c["name"])
def test_decoder_against_libjpeg_turbo_files(c):
    """libjpeg-turbo wrote both files from the same coefficients (same picture, quality and sub-sampling)."""
    prog = P.decode(open(os.path.join(PIL_DIR, c["name"] + "_prog.jpg"), "rb").read())
    base = P.decode(open(os.path.join(PIL_DIR, c["name"] + "_base.jpg"), "rb").read())
    assert prog.sof == 0xC2 and base.sof == 0xC0 and len(prog.scans) > 1
    assert prog.frame.comps == base.frame.comps
    assert same_on_coded_blocks(prog.frame, prog.coefs, base.coefs) is None


def wrap16(a):
    return (np.asarray(a, np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


@pytest.mark.parametrize("name", PC.NAMES)
def test_baseline_writer_through_the_oracle(harness, oracle, name):
    """The oracle keeps one row of 64 dequantised coefficients per block in decode order, natural order inside: AC slots
    (int16)(coef * Q); slot 0 holds the dequantised DC DIFFERENCE of the sequential coder, (int16)(DIFF * Q0)."""
    c = PC.built(name)
    harness.drive(oracle, c.base)
    got = harness.oracle_coefs(oracle)
    assert got.shape == c.arena.shape
    assert np.array_equal(got[:, 1:], c.arena[:, 1:])
    q0 = np.array([c.frame.qtabs[c.frame.comps[comp][2]][0] for comp, _v, _h in c.frame.mcu_blocks()] * (c.frame.mcu_x * c.frame.mcu_y))
    assert np.array_equal(got[:, 0], wrap16(P.baseline_dc_diffs(c.frame, c.truth) * q0))


def _synth_cases():
    from test_gpu_parity import PROGRESSIVE
    return [kw for kw in PROGRESSIVE if kw["width"] < 1000]             # the 1080p entry takes the Python decoder too long


@pytest.mark.parametrize("kw", _synth_cases(), ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_decoder_against_the_c_generator(harness, kw):
    base = P.decode(harness.synth_jpeg(seed=61, progressive=0, **kw))
    for mode in (1, 2):
        prog = P.decode(harness.synth_jpeg(seed=61, progressive=mode, **kw))
        assert prog.sof == 0xC2
        assert same_on_coded_blocks(prog.frame, prog.coefs, base.coefs) is None, mode


@pytest.mark.parametrize("name", PC.NAMES)
def test_libjpeg_reads_the_catalogue(name):
    """A script that libjpeg reads differently from the codec shows here, before a kernel is blamed for it."""
    pytest.importorskip("PIL")
    from PIL import Image
    c = PC.built(name)
    out = []
    for data in (c.file, c.base):
        im = Image.open(io.BytesIO(data)); im.load()
        out.append(np.asarray(im))
    assert out[0].shape[:2] == (c.frame.height, c.frame.width)
    assert out[0].shape == out[1].shape and np.array_equal(out[0], out[1])


def test_libjpeg_reads_random_scripts():
    pytest.importorskip("PIL")
    from PIL import Image
    for c in PC.build_random(24):
        a, b = [np.asarray(Image.open(io.BytesIO(d))) for d in (c.file, c.base)]
        assert np.array_equal(a, b), c.name
        assert same_on_coded_blocks(c.frame, c.truth, c.coefs) is None, c.name


# ------------------------------------------------------------------------------------------------------------ the lenient mode
def _lenient_is_strict(c):
    L = P.decode(c.file, lenient=True)
    assert len(L.scans) == len(c.dec.scans) and not L.flagged, c.name
    assert all(np.array_equal(a, b) for a, b in zip(L.coefs, c.truth)), c.name
    for s in L.scans:
        assert not (s["stops"] or s["overran"] or s["irregular"] or s["missing"] or s["surplus"]), (c.name, s)


@pytest.mark.parametrize("name", PC.NAMES)
def test_lenient_mode_is_the_strict_mode_on_the_catalogue(name):
    _lenient_is_strict(PC.built(name))


def test_lenient_mode_is_the_strict_mode_on_random_scripts():
    for c in PC.build_random(32):
        _lenient_is_strict(c)


# Damaged catalogue cases that libjpeg decodes the way the contract says: data that ends early reads as zero bits, an interval that is
# not there leaves its blocks alone, fill bytes and a surplus RSTn at the end are passed over, a ZRL may leave the band, a correction
# bit leaves a coefficient whose bit is set alone.
# DROPPED, because libjpeg recovers differently: every case whose damage is in front of an RSTn of a scan that goes on
# (runout_interval_emptied_ac_first, runout_cut_inside_value_bits, runout_cut_inside_an_eobn_length_field, runout_file_cut_inside_scan_1,
# runout_last_rstn_deleted, runout_last_rstn_deleted_dc, accepted_eobrun_32767_in_an_interval_of_3: libjpeg resynchronises on the
# marker numbers and carries or discards state differently), the two runs longer than the zeros left (libjpeg stores the new value one
# position PAST the band, the contract drops it), the two DC scans with irregular component lists (libjpeg refuses the scan), the
# stop cases (libjpeg goes on behind a bad code with a zero), the wide-DC cases (no baseline form) and runout_file_ends_in_an_ff_that_is_data
# (libjpeg waits for the byte behind an FF and, at the end of the file, takes neither).
LIBJPEG_AGREES = [
    "runout_file_cut_inside_the_last_scan", "runout_file_cut_inside_the_last_scan_no_restarts", "runout_file_cut_exactly_at_an_rstn",
    "runout_interval_emptied_dc", "runout_interval_emptied_refinement", "runout_cut_inside_a_code", "runout_cut_inside_a_correction_stretch",
    "runout_surplus_rstn_in_the_middle", "runout_surplus_rstn_at_the_end", "runout_fill_bytes_before_an_rstn",
    "runout_fill_bytes_behind_a_cut_interval", "runout_stuffed_ff_is_the_last_byte_of_a_cut_interval",
    "accepted_zrl_out_of_the_band_ac_first", "accepted_zrl_out_of_the_band_refinement", "accepted_zrl_out_of_the_band_refinement_over_history",
    "accepted_correction_bit_on_a_set_bit",
]


@pytest.mark.parametrize("name", LIBJPEG_AGREES)
def test_libjpeg_reads_damaged_files_to_the_lenient_truth(name):
    pytest.importorskip("PIL")
    from PIL import Image, ImageFile
    import prog_damage_cases as DC
    c = DC.built(name)
    assert c.base is not None
    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        out = []
        for data in (c.file, c.base):
            im = Image.open(io.BytesIO(data)); im.load()
            out.append(np.asarray(im))
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old
    assert out[0].shape == out[1].shape and np.array_equal(out[0], out[1])
    if not c.same_as_clean and c.file != c.clean_file:                 # (and the damage shows: these are not the pixels of the whole file)
        assert not np.array_equal(out[0], np.asarray(Image.open(io.BytesIO(c.clean_file))))
