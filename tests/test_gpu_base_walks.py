"""-m gpu: the baseline Huffman walks (walk_sync, the candidate kernels, k_write / k_write2, walk_slow and the table forms of
js_build_parallel_luts) on the catalogue of tests/base_cases.py -- streams written symbol by symbol, each with a census that proves its
event (tests/test_base_cases.py, which also pins the oracle's answers to the compiled reference's recorded digests).

Every file goes through every form of the entropy path: once in a batch of the catalogue, once more in a batch tiled to four copies
(other neighbours, other sub-sequence offsets inside the batch), and alone through the single-image call.  The comparison with the
oracle is exact: the whole DIB, the whole coefficient arena, the DIB checksum; through the single-image call also the status words,
the code-length histogram, the MCU file map and the block-DC maps.  Well-formed cases must come from the parallel path (path 1)
without a flag.  For the groups "over_limit", "nosync", "overshoot" (and "pad_is_code") only the outputs are asserted; what path and
flags they reported is printed per form (run with -s).
"""
import numpy as np
import pytest

import base_cases as BC

pytestmark = pytest.mark.gpu

XC_WRITE_V1 = 2          # jpegsnoop_amd.capi.XC_WRITE_V1
FORMS = [("default", {})] + [("sub_wl_%d" % w, {"sub_wl": w}) for w in (4, 5, 6, 7, 8)] + [
    ("rounds_only", {"cand_rounds": -1}), ("one_walk_round", {"cand_rounds": 1}), ("too_large", {"cand_max_walks": 1}),
    ("two_sync_launches", {"sync_launches": 2}), ("write_lanes_1", {"write_lanes": 1}), ("write_lanes_2", {"write_lanes": 2}),
    ("write_v1", {"cross_checks": XC_WRITE_V1}), ("split_1", {"split": 1}), ("split_2", {"split": 2})]


class Answer:
    def __init__(self, harness, oracle, c):
        import jpegsnoop_amd as J
        harness.drive(oracle, c.file)
        self.size = oracle.image_size(); self.dib = oracle.dib(); self.coefs = harness.oracle_coefs(oracle); self.cks = J.dib_checksum_numpy(self.dib)
        self.stopped = bool(oracle.status()["scan_end"] and oracle.status()["scan_bad"])     # DecodeScanImg left its MCU loop early
        self.side = dict(mcu_map=oracle.mcu_map(), blk_dc=oracle.blk_dc(), dht_histo=oracle.dht_histo(), status=oracle.status(), planes=oracle.planes())


@pytest.fixture(scope="module")
def world(harness, oracle):
    import jpegsnoop_amd as J
    assert XC_WRITE_V1 == J.capi.XC_WRITE_V1
    cases = BC.build_all()
    return cases, [Answer(harness, oracle, c) for c in cases]


def first_difference(c, got, want, stopped=False):
    """Where two arenas differ first, and the census records of that block."""
    if stopped and got.shape[0] > want.shape[0]:
        got = got[:want.shape[0]]                  # the reference gave the scan up: the rows it decoded (what it left undecoded shows in the DIB)
    if got.shape != want.shape:
        return "arena of %s rows, expected %s" % (got.shape, want.shape)
    d = np.argwhere(got != want)
    if not len(d):
        return None
    row, nat = int(d[0][0]), int(d[0][1])
    recs = [r for r in c.stream.census if r.blk == row]
    return ("%d coefficients differ; first at block %d, natural index %d: got %d, expected %d; the block's symbols: %s"
            % (len(d), row, nat, got[row, nat], want[row, nat], "; ".join("k%d %#04x @%d (%d+%d bits)" % (r.k, r.sym, r.pos, r.len, r.size) for r in recs[:12])))


def check_batch(b, cases, answers, what, report):
    errs = []
    assert len(b) > 0 and len(b) % len(cases) == 0
    sums = b.dib_checksums()
    for i in range(len(b)):
        c = cases[i % len(cases)]; a = answers[i % len(cases)]; inf = b.info(i)
        if c.wellformed:
            if inf["path"] != 1 or inf["flags"] != 0:
                errs.append("%s (image %d): path %d flags %#x" % (c.name, i, inf["path"], inf["flags"]))
        else:
            report.setdefault(c.name, set()).add((inf["path"], inf["flags"]))
        if int(sums[i]) != a.cks:
            errs.append("%s (image %d): DIB checksum differs from the oracle's" % (c.name, i))
        e = first_difference(c, b.coefs(i), a.coefs, a.stopped)
        if e:
            errs.append("%s (image %d): %s" % (c.name, i, e))
        g = b.dib(i)
        if g.shape != a.dib.shape or not np.array_equal(g, a.dib):
            errs.append("%s (image %d): DIB differs in %d bytes" % (c.name, i, int((g != a.dib).sum()) if g.shape == a.dib.shape else -1))
    assert not errs, "%s: %d findings\n%s" % (what, len(errs), "\n".join(errs[:25]))
    return sums


@pytest.mark.parametrize("form,tuning", FORMS, ids=[f for f, _ in FORMS])
def test_every_form_decodes_every_case(world, form, tuning):
    import jpegsnoop_amd as J
    cases, answers = world
    report = {}
    for copies in (1, 4):
        b = J.JpegBatch()
        try:
            b.set_tuning(**tuning)
            for c in cases:
                b.add_jpeg(c.file)
            if copies > 1:
                b.tile(copies * len(cases))
            b.upload(); b.decode(); b.sync()
            sums = check_batch(b, cases, answers, "%s, %d x the catalogue" % (form, copies), report)
            b.decode(); b.sync()                   # a second decode of the resident batch
            assert [int(s) for s in b.dib_checksums()] == [int(s) for s in sums], form
        finally:
            b.close()
    for name in sorted(report):
        print("%s [%s]: %s" % (name, form, ", ".join("path %d flags %#x" % pf for pf in sorted(report[name]))))


def test_every_case_alone_through_the_single_image_call(harness, gpu, world):
    cases, answers = world
    errs = []
    for c, a in zip(cases, answers):
        harness.drive(gpu, c.file)
        path, flags = gpu.lib.jsnoop_last_path(gpu.h), gpu.lib.jsnoop_last_flags(gpu.h)
        if c.wellformed:
            if path != 1 or flags != 0:
                errs.append("%s: path %d flags %#x" % (c.name, path, flags))
        else:
            print("%s [single image]: path %d flags %#x" % (c.name, path, flags))
        if gpu.image_size() != a.size or not np.array_equal(gpu.dib(), a.dib):
            errs.append("%s: DIB differs" % c.name)
        for i, (pa, pb) in enumerate(zip(a.side["planes"], gpu.planes())):
            if pa is not None and not np.array_equal(pa, pb):
                errs.append("%s: plane %d differs" % (c.name, i))
        if gpu.status() != a.side["status"]:
            errs.append("%s: status %s, oracle %s" % (c.name, gpu.status(), a.side["status"]))
        if not np.array_equal(gpu.dht_histo(), a.side["dht_histo"]):
            errs.append("%s: dht_histo differs" % c.name)
        if not np.array_equal(gpu.mcu_map(), a.side["mcu_map"]):
            errs.append("%s: MCU file map differs" % c.name)
        for i, (pa, pb) in enumerate(zip(a.side["blk_dc"], gpu.blk_dc())):
            if pa is not None and not np.array_equal(pa, pb):
                errs.append("%s: block-DC map %d differs" % (c.name, i))
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
