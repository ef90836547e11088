"""-m gpu: the second symbol of a write-pass step when it comes from a table read of its own (k_write2 and its HALF / REC forms,
k_write_dc: DESIGN.md §4.1), on the catalogue of tests/second_symbol_cases.py -- files written symbol by symbol in which the pair rows of
the tables cannot show the second symbol (len1 + size1 + len2 > 9), each with a census that proves its event
(tests/test_second_symbol_cases.py).

Every file goes through every sub-sequence length (JsnoopTuning.sub_wl 4 .. 8, the knob of test_every_subsequence_length) in a batch
of the catalogue tiled to two copies.  The comparison with the oracle is exact: DIB, coefficient arena, status words; well-formed cases
must come from the parallel path without a flag, the others (a run past coefficient 64, an interval that ends inside the pair) with
whatever path and flags make the outputs the oracle's -- printed per form (-s).  The same with the sample precision set to 12 (the
divider), with decode_ac = 0 through the DC-only fast form and through the Full-IDCT kernels, and alone through the single-image call,
whose write pass records the side outputs itself (REC): the code-length histogram must hold the second symbols too.
"""
import numpy as np
import pytest

import second_symbol_cases as SC
from test_gpu_base_walks import Answer, first_difference

pytestmark = pytest.mark.gpu

STATUS = ("scan_bad", "scan_end", "restart_read", "num_pixels", "pos0", "align", "warn_bad", "first")


@pytest.fixture(scope="module")
def world(harness, oracle):
    cases = SC.build_all()
    return cases, [Answer(harness, oracle, c) for c in cases]


@pytest.fixture(scope="module")
def world12(harness, oracle):
    """The catalogue with 12-bit sample precision in the frame header: every decoded value is divided by 16, truncating."""
    class C12:
        def __init__(self, c):
            self.name, self.stream, self.wellformed, self.group, self.file = c.name + "_p12", c.stream, c.wellformed, c.group, SC.with_precision(c.file, 12)
    cases = [C12(c) for c in SC.build_all() if c.group != "cut_interval"]
    return cases, [Answer(harness, oracle, c) for c in cases]


def arena_of_the_pixels(c, a):
    """The oracle's coefficient record as the arena the pixels are made from.  They differ in one block, in the "cut_interval" cases only: the block in
    which the reference's decode of the image ENDS (value or code bits past the end of the data: ReadScanVal reports the underflow and DecodeScanComp
    returns before its IDCT, :1737-1757).  The oracle's record keeps what had been read of that block -- here the one AC value of the pair's first
    symbol, tests/test_second_symbol_cases.py proves it -- but no output of the reference holds it; the arena has the block as its pixels are: empty
    behind the DC term (k_dead_fill).  The same on the commit before this test existed."""
    want = a.coefs
    if c.group == "cut_interval":
        want = want.copy(); want[SC.last_block_read(want), 1:] = 0
    return want


def status_list(d):
    return [int(v) for v in d.values()]


def check_batch(b, cases, answers, what, coefs=True):
    errs = []; seen = {}
    assert len(b) > 0 and len(b) % len(cases) == 0
    sums = b.dib_checksums()
    for i in range(len(b)):
        c = cases[i % len(cases)]; a = answers[i % len(cases)]; inf = b.info(i)
        if c.wellformed:
            if inf["path"] != 1 or inf["flags"] != 0:
                errs.append("%s (image %d): path %d flags %#x" % (c.name, i, inf["path"], inf["flags"]))
        else:
            seen.setdefault(c.name, set()).add((inf["path"], inf["flags"]))
        if int(sums[i]) != a.cks or not np.array_equal(b.dib(i), a.dib):
            errs.append("%s (image %d): DIB differs from the oracle's" % (c.name, i))
        if coefs:
            e = first_difference(c, b.coefs(i), arena_of_the_pixels(c, a), a.stopped)
            if e:
                errs.append("%s (image %d): %s" % (c.name, i, e))
        if i < len(cases):
            st = status_list(b.side_outputs(i, bright=False)["status"])
            if st != [int(a.side["status"][k]) for k in STATUS]:
                errs.append("%s (image %d): status %s, oracle %s" % (c.name, i, st, a.side["status"]))
    for name in sorted(seen):
        print("%s [%s]: %s" % (name, what, ", ".join("path %d flags %#x" % pf for pf in sorted(seen[name]))))
    assert not errs, "%s: %d findings\n%s" % (what, len(errs), "\n".join(errs[:25]))


def run_batch(cases, answers, what, copies=2, coefs=True, decode_ac=True, **tuning):
    import jpegsnoop_amd as J
    b = J.JpegBatch(decode_ac=decode_ac)
    try:
        b.set_tuning(**tuning)
        for c in cases:
            b.add_jpeg(c.file)
        if copies > 1:
            b.tile(copies * len(cases))
        b.upload(); b.decode(); b.sync()
        form = b.last_form()                       # (before anything asks for the coefficient arena: a fast-form batch is decoded again for that)
        check_batch(b, cases, answers, what, coefs)
        return form
    finally:
        b.close()


@pytest.mark.parametrize("wl", [4, 5, 6, 7, 8])
def test_every_subsequence_length(world, wl):
    cases, answers = world
    run_batch(cases, answers, "sub_wl %d" % wl, sub_wl=wl)


@pytest.mark.parametrize("form,tuning", [("one_lane_per_subsequence", {"write_lanes": 1}), ("two_lanes_per_subsequence", {"write_lanes": 2}),
                                         ("rounds_only", {"cand_rounds": -1, "sub_wl": 4}), ("split_2", {"split": 2})])
def test_write_pass_forms(world, form, tuning):
    """k_write2 with one lane per sub-sequence and with two (HALF: the first lane's range ends in the middle of the sub-sequence)."""
    cases, answers = world
    run_batch(cases, answers, form, **tuning)


@pytest.mark.parametrize("wl", [4, 5, 6, 7, 8])
def test_precision_divider(world12, wl):
    cases, answers = world12
    run_batch(cases, answers, "precision 12, sub_wl %d" % wl, copies=1, sub_wl=wl)


@pytest.fixture(scope="module")
def world_dc(harness, oracle):
    cases = SC.build_all(colour=True)              # (three components each: what the fast form takes)
    oracle.set_options(decode_ac=0)
    try:
        return cases, [Answer(harness, oracle, c) for c in cases]
    finally:
        oracle.set_options()


@pytest.mark.parametrize("wl", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("form", ["fast", "generic"])
def test_dc_only(world_dc, form, wl):
    """decode_ac = 0: the walk of k_write_dc (form 2) and of k_write2 with the AC stores masked off (JSNOOP_XC_DC_GENERIC, form 1)."""
    import jpegsnoop_amd as J
    cases, answers = world_dc
    xc = J.capi.XC_DC_GENERIC if form == "generic" else 0
    got = run_batch(cases, answers, "dc-only %s, sub_wl %d" % (form, wl), coefs=False, decode_ac=False, sub_wl=wl, cross_checks=xc)
    assert got == (1 if form == "generic" else 2)


def test_alone_with_side_outputs(harness, gpu, world):
    """The single-image call with a log callback: the decode's own write pass records MCU positions and the code-length histogram (REC)."""
    cases, answers = world
    errs = []
    for c, a in zip(cases, answers):
        harness.drive(gpu, c.file)
        path, flags = gpu.lib.jsnoop_last_path(gpu.h), gpu.lib.jsnoop_last_flags(gpu.h)
        if c.wellformed and (path != 1 or flags != 0):
            errs.append("%s: path %d flags %#x" % (c.name, path, flags))
        if gpu.image_size() != a.size or not np.array_equal(gpu.dib(), a.dib):
            errs.append("%s: DIB differs" % c.name)
        if gpu.status() != a.side["status"]:
            errs.append("%s: status %s, oracle %s" % (c.name, gpu.status(), a.side["status"]))
        if not np.array_equal(gpu.dht_histo(), a.side["dht_histo"]):
            errs.append("%s: dht_histo differs: %s, oracle %s" % (c.name, gpu.dht_histo()[1, 0].tolist(), a.side["dht_histo"][1, 0].tolist()))
        if not np.array_equal(gpu.mcu_map(), a.side["mcu_map"]):
            errs.append("%s: MCU file map differs" % c.name)
        for i, (pa, pb) in enumerate(zip(a.side["blk_dc"], gpu.blk_dc())):
            if pa is not None and not np.array_equal(pa, pb):
                errs.append("%s: block-DC map %d differs" % (c.name, i))
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
