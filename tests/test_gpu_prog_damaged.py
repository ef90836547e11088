"""-m gpu: every form of the progressive (SOF2) scan kernels on DAMAGED and IRREGULAR files, against the lenient mode of the plain
Annex G codec (tests/prog_codec.py: decode(file, lenient=True), the damage contract of DESIGN.md 4.5).

tests/test_gpu_progressive_forms.py pins the three decoders (a wave per restart interval, 2..16 intervals per wave, a lane per
interval) to each other on well-formed files; here they get the catalogue of tests/prog_damage_cases.py -- every file with one
named irregularity whose place the CPU suite has proved (tests/test_prog_damage_cases.py) -- and 200 randomly damaged files.  Every
comparison is exact: the WHOLE coefficient arena (padding blocks included), the flag (JSNOOP_FLAG_BAD_CODE exactly when the model
says an interval stopped or overran or a scan lacks intervals), path 3, and the whole MCU-rounded DIB and its checksum against the
oracle's decode of the baseline form of the lenient truth.  The four wide-DC cases have no baseline form (DC differences of more
than 11 bits): their DC is pinned through JpegBatch.coefs_to_torch instead; the back end that turns coefficients into pixels is the
one every other case and tests/test_gpu_progressive_forms.py cover.  The damaged files sit in one batch beside well-formed ones,
first and last, tiled to twice its size: a decoder that leaves its image's slice of the arena, or stalls a neighbour, shows in the
bystanders.  A failure names the case, the form and what the model saw go wrong where (scan, interval, unit, reason).
"""
import ctypes as C

import numpy as np
import pytest

import prog_cases as PC
import prog_codec as P
import prog_damage_cases as DC
from test_gpu_progressive_forms import FORMS, MIXED, answer, first_difference, decode_batch, _single_tuning

pytestmark = pytest.mark.gpu

BAD_CODE = 0x0001                                   # JSNOOP_FLAG_BAD_CODE (include/jsnoop_gpu.h)


def flagged_of(c):
    return bool(getattr(c, "flagged", False))      # (the well-formed bystanders of tests/prog_cases.py carry no such field: never flagged)


def record_of(c):
    return c.record() if hasattr(c, "record") else "well-formed bystander"


def layout():
    """The catalogue between well-formed files: a damaged file first, the bystanders spread through, a damaged file last."""
    dam = DC.build_all(); by = [PC.built(n) for n in MIXED]
    out = []; step = (len(dam) - 1) // len(by)
    for i, c in enumerate(dam[:-1]):
        out.append(c)
        if i % step == step - 1 and i // step < len(by):
            out.append(by[i // step])
    out.append(dam[-1])
    assert len(out) == len(dam) + len(by) and hasattr(out[0], "kind") and hasattr(out[-1], "kind")
    return out


def dc_planes(b, i, c):
    """Non-encodable truth: the cumulative DC (natural index 0 of coefs_to_torch, int16) against the model's, per component."""
    errs = []
    for comp, t in enumerate(b.coefs_to_torch(images=[i])[0]):
        got = t[..., 0].cpu().numpy(); q0 = c.frame.qtabs[c.frame.comps[comp][2]][0]
        want = (c.truth[comp][..., 0].astype(np.int64) * q0 & 0xFFFF).astype(np.uint16).view(np.int16)
        if got.shape != want.shape or not np.array_equal(got, want):
            errs.append("component %d: DC plane differs in %d blocks" % (comp, int((got != want).sum()) if got.shape == want.shape else -1))
    return errs


def check_images(harness, oracle, b, cases, what, pixels=True):
    """Image i of batch b is cases[i % len(cases)]."""
    errs = []
    assert len(b) > 0 and len(b) % len(cases) == 0
    sums = b.dib_checksums()
    for i in range(len(b)):
        c = cases[i % len(cases)]; inf = b.info(i); e = []
        if inf["path"] != 3:
            e.append("path %d" % inf["path"])
        if bool(inf["flags"] & BAD_CODE) != flagged_of(c) or (inf["flags"] & ~BAD_CODE):
            e.append("flags %#x, the model says %s" % (inf["flags"], "flagged" if flagged_of(c) else "not flagged"))
        d = first_difference(c, b.coefs(i), c.arena)
        if d:
            e.append(d)
        if c.base is not None and pixels:
            a = answer(harness, oracle, c)
            g = b.dib(i)
            if int(sums[i]) != a.cks:
                e.append("DIB checksum differs from the oracle's")
            if g.shape != a.dib.shape or not np.array_equal(g, a.dib):
                e.append("DIB differs in %d bytes" % (int((g != a.dib).sum()) if g.shape == a.dib.shape else -1))
        elif c.base is None:
            e += dc_planes(b, i, c)
        errs += ["%s, image %d = %s [%s]: %s" % (what, i, c.name, record_of(c), x) for x in e]
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))


@pytest.mark.parametrize("form", FORMS)
def test_every_form_decodes_the_damaged_catalogue(harness, oracle, form):
    import jpegsnoop_amd as J
    cases = layout()
    b = J.JpegBatch()
    try:
        for c in cases:
            b.add_jpeg(c.file)
        b.tile(2 * len(cases))
        decode_batch(b, form)
        check_images(harness, oracle, b, cases, "pg_lanes=%d" % form)
        # once more, resident: the status words are zeroed per decode, nothing of the first decode shows in the second
        sums = b.dib_checksums().copy(); flags = [b.info(i)["flags"] for i in range(len(b))]
        b.decode(); b.sync()
        assert np.array_equal(b.dib_checksums(), sums) and [b.info(i)["flags"] for i in range(len(b))] == flags
        assert any(flags) and not all(flags)
    finally:
        b.close()


def test_one_batch_through_every_form_in_turn_leaves_the_same_arena(harness, oracle):
    """The three decoders on the SAME resident batch, one after the other and back: they stop at the same symbol and leave the same
    coefficients (each is compared with the model; pixels are covered per form above)."""
    import jpegsnoop_amd as J
    cases = layout()
    b = J.JpegBatch()
    try:
        for c in cases:
            b.add_jpeg(c.file)
        for form in (64, 1, 8, 64):
            decode_batch(b, form)
            check_images(harness, oracle, b, cases, "same batch, pg_lanes=%d" % form, pixels=False)
    finally:
        b.close()


@pytest.mark.parametrize("form", (1, 64))
def test_the_single_file_call_on_every_damaged_file(harness, oracle, gpu, form):
    """jsnoop_decode_progressive: scan count, last_flags, whole DIB and planes, and the log's
    '*** ERROR: progressive scan data is malformed' line exactly when the model says flagged."""
    errs = []
    _single_tuning(gpu, pg_lanes=form)
    try:
        for c in DC.build_all():
            n = gpu.decode_progressive(c.file); e = []
            if n != len(c.dec.scans):
                errs.append("%s [%s]: returned %d, the file has %d scans (%s)" % (c.name, c.record(), n, len(c.dec.scans), gpu.lib.jsnoop_last_error())); continue
            fl = gpu.lib.jsnoop_last_flags(gpu.h)
            if gpu.lib.jsnoop_last_path(gpu.h) != 3 or bool(fl & BAD_CODE) != c.flagged or fl & ~BAD_CODE:
                e.append("path %d flags %#x, the model says %s" % (gpu.lib.jsnoop_last_path(gpu.h), fl, "flagged" if c.flagged else "not flagged"))
            said = sum("progressive scan data is malformed" in ln for ln in gpu.log_lines())
            if said != int(c.flagged):
                e.append("%d malformed-data lines in the log, the model says %s" % (said, "flagged" if c.flagged else "not flagged"))
            if c.base is not None:
                a = answer(harness, oracle, c)
                if gpu.image_size() != a.size or not np.array_equal(gpu.dib(), a.dib):
                    e.append("DIB differs")
                for i, (pa, pb) in enumerate(zip(a.planes, gpu.planes())):
                    if pa is not None and not np.array_equal(pa, pb):
                        e.append("plane %d differs" % i)
            errs += ["pg_lanes=%d, %s [%s]: %s" % (form, c.name, c.record(), x) for x in e]
    finally:
        _single_tuning(gpu, pg_lanes=0)
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))


@pytest.mark.parametrize("form", (1, 8, 64))
def test_random_damage(harness, oracle, form):
    """200 files, each a random legal script with ONE mutation inside the entropy-coded bytes of one scan (a byte flipped, deleted or
    inserted, the tail cut, an RSTn deleted or doubled; fixed seed): the parser refuses none, the truth is the lenient model; arena
    and flags, and the DIB where the truth has a baseline form.  The set's shares (flagged, far from the undamaged arena) are asserted
    on the CPU in tests/test_prog_damage_cases.py."""
    import jpegsnoop_amd as J
    cases = DC.random_damage()
    b = J.JpegBatch()
    try:
        for c in cases:
            assert b.add_jpeg(c.file) >= 0
        assert len(b) == len(cases) == 200
        decode_batch(b, form)
        check_images(harness, oracle, b, cases, "random damage, pg_lanes=%d" % form)
    finally:
        b.close()


def test_job_with_damaged_refused_and_good_files(harness, oracle):
    """A damaged progressive file and a file the progressive parser refuses between a good progressive and a good baseline file: counted
    as flagged / refused / ok, and the good files come out as in a job without the bad ones."""
    import jpegsnoop_amd as J
    dam = DC.built("stop_refinement_refine_s_middle_block_after_corrections_and_a_new_value")
    refused = dict((n, f) for n, f, _t in DC.refusals()[1])["scan_al_14"]
    good_p = PC.built("dri_1"); good_b = harness.synth_jpeg(width=64, height=48, hs=2, vs=1, quality=80, seed=5)

    def run(files):
        job = J.JpegJob(devices=[0])
        try:
            for f in files:
                job.add(f)
            st = job.run()
            return st, job.results()
        finally:
            job.close()
    st, res = run([dam.file, good_p.file, refused, good_b])
    st0, res0 = run([good_p.file, good_b])
    assert (st["files"], st["ok"], st["refused"], st["unreadable"], st["flagged"]) == (4, 3, 1, 0, 1), st
    assert (st0["files"], st0["ok"], st0["refused"], st0["flagged"]) == (2, 2, 0, 0), st0
    assert [r.status for r in res] == ["ok", "ok", "refused", "ok"] and res[2].message
    assert res[0].kind == "progressive" and res[0].info["flags"] & BAD_CODE and res[0].dib_hash == answer(harness, oracle, dam).cks
    assert (res[1].dib_hash, res[3].dib_hash) == (res0[0].dib_hash, res0[1].dib_hash)
    assert res[1].dib_hash == answer(harness, oracle, good_p).cks and res[1].info["flags"] == 0 and res[3].info["flags"] == 0


# ------------------------------------------------------------------------------------------------------------ parser refusals
def _refusal_names():
    return [n for n, _f, _t in DC.refusals()[1]]


@pytest.mark.parametrize("name", _refusal_names())
def test_the_parser_refuses_and_leaves_the_batch_as_it_was(harness, oracle, name):
    """One file per refusal branch of the progressive parser: jsnoop_batch_add_progressive returns -1, jsnoop_last_error names the
    reason, the batch holds what it held, and a good file added behind decodes exactly."""
    import jpegsnoop_amd as J
    good, files = DC.refusals()
    f, text = [(f, t) for n, f, t in files if n == name][0]
    lib = J.load()
    by = PC.built("geometry_2x2_2x1_1x1")
    b = J.JpegBatch()
    try:
        assert b.add_jpeg(by.file) == 0
        buf = (C.c_uint8 * len(f)).from_buffer_copy(f)
        assert lib.jsnoop_batch_add_progressive(b._h, C.cast(buf, C.c_void_p), len(f)) == -1
        assert text in J.last_error(), J.last_error()
        if name not in ("sof0", "sos_before_sof", "truncated_segment"):        # (a first frame header that is SOF2: add_jpeg routes the file the same way)
            with pytest.raises(RuntimeError, match="batch_add_jpeg failed"):
                b.add_jpeg(f)
            assert text in J.last_error(), J.last_error()
        assert len(b) == 1
        assert b.add_jpeg(good) == 1 and len(b) == 2
        b.upload(); b.decode(); b.sync()
        fr = P.decode(good)
        for i, (frame, truth) in enumerate(((by.frame, by.truth), (fr.frame, fr.coefs))):
            assert b.info(i)["path"] == 3 and b.info(i)["flags"] == 0
            assert np.array_equal(b.coefs(i), P.arena(frame, truth)), "image %d after the refusal of %s" % (i, name)
        assert int(b.dib_checksums()[0]) == answer(harness, oracle, by).cks
    finally:
        b.close()
