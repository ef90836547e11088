"""-m gpu: every form of the progressive (SOF2) scan kernels against the plain Annex G codec of tests/prog_codec.py.

The reference refuses SOF2, so these kernels have no compiled reference answer; what pins them is the codec (itself pinned on the
CPU in tests/test_prog_codec.py to libjpeg-turbo's files, to the oracle and to libjpeg through Pillow) and the oracle's pixels of
the baseline form of the codec's truth.  Which form decodes a batch is a matter of its size (js_prog_upload) or of
JsnoopTuning.pg_lanes: 1 = a wave per restart interval (WReader), 2 / 4 / 8 / 16 = that many intervals per wave (PReader), 64 = the
lane-per-interval kernel (LReader, its own refinement algorithm).  Every catalogue file of tests/prog_cases.py goes through every
form; the comparison is exact and covers the WHOLE coefficient arena (padding blocks included; slot 0 is zero after
k_prog_finalize, the DC shows in the pixels) and the whole MCU-rounded DIB.
"""
import ctypes as C

import numpy as np
import pytest

import prog_cases as PC
import prog_codec as P

pytestmark = pytest.mark.gpu

FORMS = (1, 2, 4, 8, 16, 64)
UNZIGZAG = {n: k for k, n in enumerate(P.ZIGZAG)}
N_RANDOM = 32


class Answer:
    """The oracle's decode of the baseline form of a case's truth."""

    def __init__(self, harness, oracle, c):
        import jpegsnoop_amd as J
        harness.drive(oracle, c.base)
        self.size = oracle.image_size(); self.dib = oracle.dib(); self.planes = oracle.planes(); self.bright = oracle.bright_avg()
        self.cks = J.dib_checksum_numpy(self.dib)


_ANSWERS = {}


def answer(harness, oracle, c):
    if c.name not in _ANSWERS:
        _ANSWERS[c.name] = Answer(harness, oracle, c)
    return _ANSWERS[c.name]


def first_difference(c, got, want):
    """Where two arenas differ first: image, block, zig-zag position and the scans that own that position."""
    if got.shape != want.shape:
        return "%s: arena of %s rows, expected %s" % (c.name, got.shape, want.shape)
    d = np.argwhere(got != want)
    if not len(d):
        return None
    row, nat = int(d[0][0]), int(d[0][1]); fr = c.frame; blocks = fr.mcu_blocks()
    mcu, j = divmod(row, len(blocks)); comp, v, h = blocks[j]; my, mx = divmod(mcu, fr.mcu_x)
    H, V = fr.hv[comp]; by, bx = my * V + v, mx * H + h; nby, nbx = fr.coded(comp); k = UNZIGZAG[nat]
    own = ["#%d (Ss %d Se %d Ah %d Al %d, DRI %d, %d intervals)" % (i, s["ss"], s["se"], s["ah"], s["al"], s["dri"], len(s["intervals"]))
           for i, s in enumerate(c.dec.scans) if i in c.owner(comp, k)]
    return ("%s: %d coefficients differ; first at arena row %d = component %d block (y %d, x %d) [%s the coded %d x %d grid], zig-zag %d (natural %d): "
            "got %d, expected %d; scans that write it: %s" % (c.name, len(d), row, comp, by, bx, "inside" if by < nby and bx < nbx else "OUTSIDE", nby, nbx, k, nat,
                                                            got[row, nat], want[row, nat], "; ".join(own)))


def check_batch(harness, oracle, b, cases, what, every=1):
    """Image i of batch b is cases[i % len(cases)]: path, flags, whole arena, whole DIB."""
    errs = []
    assert len(b) > 0 and len(b) % len(cases) == 0, (len(b), len(cases))
    sums = b.dib_checksums()
    for i in range(len(b)):
        c = cases[i % len(cases)]; inf = b.info(i); a = answer(harness, oracle, c)
        if inf["path"] != 3 or inf["flags"] != 0:
            errs.append("%s: path %d flags %#x" % (c.name, inf["path"], inf["flags"]))
        if int(sums[i]) != a.cks:
            errs.append("%s (image %d): DIB checksum differs from the oracle's" % (c.name, i))
        if i % every == 0 or i == len(b) - 1:
            e = first_difference(c, b.coefs(i), c.arena)
            if e:
                errs.append("image %d " % i + e)
            g = b.dib(i)
            if g.shape != a.dib.shape or not np.array_equal(g, a.dib):
                errs.append("%s (image %d): DIB differs in %d bytes" % (c.name, i, int((g != a.dib).sum()) if g.shape == a.dib.shape else -1))
    assert not errs, "%s: %d findings\n%s" % (what, len(errs), "\n".join(errs[:25]))


def decode_batch(b, form):
    b.set_tuning(pg_lanes=form)                  # (a tuning change un-uploads the batch and marks the work lists for rebuilding)
    b.upload(); b.decode(); b.sync()


@pytest.mark.parametrize("form", FORMS)
def test_every_form_decodes_every_case(harness, oracle, form):
    import jpegsnoop_amd as J
    cases = PC.build_all()
    b = J.JpegBatch()
    try:
        for c in cases:
            b.add_jpeg(c.file)
        decode_batch(b, form)
        check_batch(harness, oracle, b, cases, "pg_lanes=%d" % form)
    finally:
        b.close()


def _single_tuning(gpu, **kw):
    import jpegsnoop_amd as J
    t = J.capi.Tuning()
    gpu.lib.jsnoop_tuning_defaults(C.byref(t))
    for k, v in kw.items():
        setattr(t, k, v)
    assert gpu.lib.jsnoop_set_tuning(C.c_void_p(gpu.h), C.byref(t)) == 0, J.last_error()


@pytest.mark.parametrize("form", FORMS)
def test_every_form_through_the_single_file_call(harness, oracle, gpu, form):
    """jsnoop_decode_progressive: the decoder's private batch takes the form through jsnoop_set_tuning.  Whole DIB, whole planes and
    the brightest-pixel / average-Y record against the oracle; the number of scans against the script."""
    errs = []
    _single_tuning(gpu, pg_lanes=form)
    try:
        for c in PC.build_all():
            a = answer(harness, oracle, c)
            n = gpu.decode_progressive(c.file)
            if n != len(c.script):
                errs.append("%s: %d scans, script has %d (%s)" % (c.name, n, len(c.script), gpu.lib.jsnoop_last_error())); continue
            if gpu.lib.jsnoop_last_path(gpu.h) != 3 or gpu.lib.jsnoop_last_flags(gpu.h) != 0:
                errs.append("%s: path %d flags %#x" % (c.name, gpu.lib.jsnoop_last_path(gpu.h), gpu.lib.jsnoop_last_flags(gpu.h)))
            if gpu.image_size() != a.size or not np.array_equal(gpu.dib(), a.dib):
                errs.append("%s: DIB differs" % c.name)
            for i, (pa, pb) in enumerate(zip(a.planes, gpu.planes())):
                if pa is not None and not np.array_equal(pa, pb):
                    errs.append("%s: plane %d differs" % (c.name, i))
            if gpu.bright_avg() != a.bright:
                errs.append("%s: bright / average record %s, oracle %s" % (c.name, gpu.bright_avg(), a.bright))
    finally:
        _single_tuning(gpu, pg_lanes=0)
    assert not errs, "pg_lanes=%d: %d findings\n%s" % (form, len(errs), "\n".join(errs[:25]))


def _threshold_cases():
    out = []
    for i, (geo, w, h) in enumerate([("grey", 256, 256), ("1x1", 128, 128), ("grey", 256, 256)]):
        fr = PC.frame_of(geo, w, h)
        out.append(PC.Case("threshold_%d_%s" % (i, geo), fr, PC.noise(fr, 300 + i, density=0.3), PC.script_standard(fr.ncomp, dri=8)).build())
    return out


@pytest.mark.parametrize("copies,form", [(1, 1), (4, 4), (22, 8), (48, 64)])
def test_forms_agree_where_the_batch_size_picks_them(harness, oracle, copies, form):
    """pg_lanes = 0: js_prog_upload picks the form from the batch's total number of restart intervals (> 7 000: 4 per wave, > 40 000: 8,
    >= 88 000 with >= 16 per scan: the lane kernel).  Three pictures, tiled until each rule applies; the interval counts come from the
    codec's record of the files."""
    import jpegsnoop_amd as J
    cases = _threshold_cases()
    per_trio = sum(len(s["intervals"]) for c in cases for s in c.dec.scans); nsc = sum(len(c.dec.scans) for c in cases)
    total = per_trio * copies
    rule = 64 if (total // (nsc * copies) >= 16 and total >= 88000) else 8 if total > 40000 else 4 if total > 7000 else 1
    assert rule == form, (total, rule)
    b = J.JpegBatch()
    try:
        for c in cases:
            b.add_jpeg(c.file)
        b.tile(3 * copies)
        decode_batch(b, 0)
        check_batch(harness, oracle, b, cases, "%d images, automatic form" % (3 * copies), every=7)
    finally:
        b.close()


MIXED = ["dc_interleaved_ac_whole_cr_y_cb", "successive_approximation_three_and_two_levels", "geometry_grey_declares_2x2", "geometry_4x2", "dri_1",
         "values_every_category_al0", "geometry_2x2_2x1_1x1", "dc_al3_three_refinements_between_ac", "refinement_stretches_and_zrl"]


def test_mixed_batch_tiled_and_decoded_again_in_every_form(harness, oracle):
    """Files with different numbers of dependency levels, components and geometries in one batch, tiled to an odd multiple: the
    batch runs as many launches as its deepest image has levels, and images with fewer sit the rest out.  ONE batch object goes through
    every form in turn (a tuning change rebuilds the work lists); every decode must leave the same arena."""
    import jpegsnoop_amd as J
    cases = [PC.built(n) for n in MIXED]
    assert len({len(c.script) for c in cases}) >= 4 and {c.frame.ncomp for c in cases} == {1, 3}
    b = J.JpegBatch()
    try:
        for c in cases:
            b.add_jpeg(c.file)
        b.tile(3 * len(cases))
        for form in FORMS + (0, 64, 1):
            decode_batch(b, form)
            check_batch(harness, oracle, b, cases, "mixed batch, pg_lanes=%d" % form)
    finally:
        b.close()


@pytest.mark.parametrize("form", FORMS)
def test_progressive_truly_random_scripts(harness, oracle, form):
    """The sibling of test_progressive_random_scripts (tests/test_gpu_parity.py, which draws one of the C generator's two scripts):
    random LEGAL scripts from the Python encoder -- bands and bit planes cut at random per component and per plane, DC scans
    interleaved or not, a random restart interval per scan, random geometry, sparse to dense coefficients; fixed seed."""
    import jpegsnoop_amd as J
    cases = PC.build_random(N_RANDOM)
    b = J.JpegBatch()
    try:
        for c in cases:
            b.add_jpeg(c.file)
        decode_batch(b, form)
        check_batch(harness, oracle, b, cases, "random scripts, pg_lanes=%d" % form)
    finally:
        b.close()
