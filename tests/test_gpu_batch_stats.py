"""-m gpu: jsnoop_batch_pack_stats / jsnoop_batch_read_stats (k_stats_batch, k_stats_order in jsnoop_stats.hip), JpegBatch.stats_to_torch / stats_all,
CJPEGsnoopCoreGpu::BatchPackStats and JobFileResult.stats_to_torch on the 58 files of tests/stats_cases.py plus the catalogue of
tests/batch_stats_cases.py: unit seams, sampling layouts, the order and budget of the range events, about 200 pictures of a unit or a few.

All of them are decoded in ONE batch and read in ONE call.  Everything is compared exactly: every row equals the oracle's 2482 words after the decode
(bHistoEn; with histo_en=False the words under bStatClipEn alone), equals what the per-image door JpegBatch.color_stats gives, and `totals` equal the
model's range events by kind.  tests/test_stats_cases.py and tests/test_batch_stats_cases.py prove on the CPU that the files hold what their names say,
that the model equals the oracle and the oracle the compiled reference.  A failure names the first differing word by meaning (stats_cases_util.explain).
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import batch_stats_cases as BC
import deal_cases as D
import stats_cases as SC
import stats_model as SM
from stats_cases_util import OPTION_SETS, explain, run_passes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 2482


class Answer:
    """What the oracle and the model say about one file after the decode alone: words[key], the model on the oracle's planes per key, totals by kind."""

    def __init__(self, harness, oracle, case):
        self.case = case
        once = SimpleNamespace(name=case.name, file=case.file, rerenders=[])             # (the decode alone: this door makes no re-render)
        self.words, self.planes = {}, {}
        for key in OPTION_SETS:
            d = run_passes(harness, oracle, once, key, keep=True)
            self.words[key] = d["words"][0]; self.planes[key] = d["planes"]

    def model(self, key):
        c = self.case
        return SM.run(self.planes[key], c.img_x, c.img_y, c.mcu_w, c.mcu_h, c.ncomp, [(OPTION_SETS[key][1], 0, 0, 0, 0, 0)], keep_pixels=False)

    def totals(self, key):
        """Range events by kind in all, indexed like words 37..42 (Y<0, Y>255, Cb<0, Cb>255, Cr<0, Cr>255), from the model's pixels."""
        c = self.case
        q = SM.pixels(self.planes[key], c.img_x, c.img_y, c.mcu_w, c.mcu_h, c.ncomp, SM.PASS0)
        return [int((q.clipv[k // 2] < 0).sum()) if k % 2 == 0 else int((q.clipv[k // 2] > 255).sum()) for k in range(6)]


@pytest.fixture(scope="module")
def world(harness, oracle):
    cases = SC.build_all() + BC.build_all()
    assert len(SC.build_all()) == 58 and len(cases) > 280
    return [Answer(harness, oracle, c) for c in cases]


def _decoded(J, files, decode_ac=True, want_planes=True):
    b = J.JpegBatch(decode_ac=decode_ac, want_planes=want_planes)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


@pytest.fixture(scope="module")
def full(gpu, world):
    """Every file in one batch, Full IDCT, and ONE stats_to_torch per histo_en: (batch, rows, totals, rows under bStatClipEn alone)."""
    import jpegsnoop_amd as J
    b = _decoded(J, [a.case.file for a in world])
    form = b.last_form()
    rows, tot = b.stats_to_torch(totals=True)
    clip = b.stats_to_torch(histo_en=False)
    assert b.last_form() == form == 1
    yield b, rows.cpu().numpy().view(np.uint32), tot.cpu().numpy(), clip.cpu().numpy().view(np.uint32)
    b.close()


def _compare(world, picks, rows, hk, errs, what):
    for k, i in enumerate(picks):
        a = world[i]
        if not np.array_equal(rows[k][:WORDS], a.words[hk]):
            errs.append("%s row %d (image %d): %s" % (what, k, i, explain(a.case, hk, 0, rows[k][:WORDS], a.model(hk))))


def test_one_batch_one_call_equals_the_oracle(world, full):
    b, rows, tot, clip = full
    assert rows.shape == (len(world), WORDS) and clip.shape == rows.shape and tot.shape == (len(world), 6)
    errs = []
    _compare(world, range(len(world)), rows, "histo", errs, "histo")
    _compare(world, range(len(world)), clip, "clip", errs, "clip")
    for i, a in enumerate(world):
        want = a.totals("histo")
        if tot[i].tolist() != want:
            errs.append("image %d (%s): totals %s, the model's events by kind %s" % (i, a.case.name, tot[i].tolist(), want))
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
    assert not clip[:, :37].any() and not clip[:, 49:].any(), "histo_en = 0 leaves only the clip counters"
    assert np.array_equal(clip[:, 37:49], rows[:, 37:49])
    above = tot.sum(1) > 10
    assert above.sum() > 40 and (~above & (tot.sum(1) > 0)).sum() >= 3, "both arms of k_stats_order"
    assert np.array_equal(rows[:, 37:43][~above], tot[~above].astype(np.uint32)) and (rows[:, 37:43][above].sum(1) == 10).all()


def test_every_row_equals_the_per_image_door(world, full):
    b, rows, _tot, clip = full
    errs = []
    for i, a in enumerate(world):
        for got, histo_en, key in ((rows[i], True, "histo"), (clip[i], False, "clip")):
            one = b.color_stats(i, histo_en=histo_en)
            if not np.array_equal(got, one):
                k, name, g, e = SM.first_difference(got, one)
                errs.append("image %d (%s) [%s]: %s is %d, color_stats says %d (word %d)" % (i, a.case.name, key, name, g, e, k))
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))


def test_the_host_door(world, full):
    b, rows, _tot, clip = full
    assert np.array_equal(b.stats_all(), rows)
    pick = [5, len(world) - 1, 5, 70]
    assert np.array_equal(b.stats_all(images=pick, histo_en=False), clip[pick])
    assert b.stats_all(images=[]).shape == (0, WORDS)
    with pytest.raises(IndexError):
        b.stats_all(images=[len(world)])


def test_lists_pitch_sentinels_and_a_second_call(world, full):
    import torch
    import jpegsnoop_amd as J
    b, rows, tot, _clip = full
    rng = np.random.default_rng(7)
    pick = [int(x) for x in rng.permutation(len(world))[:40]] + [3, 3]                  # a permuted subset, an image listed twice
    pick[1] = pick[0]
    pitch = WORDS + 38
    block = torch.full((len(pick) + 2, pitch), -77, dtype=torch.int32, device="cuda")    # a row of sentinels in front, one behind, 38 words behind every row
    out = block[1:-1]
    for _ in range(2):                                                                   # the second call finds the first one's words there: rows are zeroed by the call
        r, t = b.stats_to_torch(images=pick, out=out, totals=True)
        assert r is out
        got = block.cpu().numpy()
        assert (got[0] == -77).all() and (got[-1] == -77).all() and (got[1:-1, WORDS:] == -77).all(), "nothing outside the rows is written"
        assert np.array_equal(got[1:-1, :WORDS].view(np.uint32), rows[pick]) and np.array_equal(t.cpu().numpy(), tot[pick])
    f = J.stats_fields(out[0][:WORDS])
    assert int(f["count"]) == world[pick[0]].case.npix and int(f["y"].sum()) == world[pick[0]].case.npix and f["records"].shape == (12, 3)
    # n = 0
    e, et = b.stats_to_torch(images=[], totals=True)
    assert tuple(e.shape) == (0, WORDS) and tuple(et.shape) == (0, 6)
    import ctypes as C
    assert b._lib.jsnoop_batch_pack_stats(b._h, 1, None, 0, None, 0, None) == 0
    # out= of the wrong kind
    for bad, word in ((block[1:-1, :100], "shape"), (block[1:-1].long(), "wanted"), (block[1:-1].cpu(), "wanted"), (block[1:3], "shape")):
        with pytest.raises(ValueError, match=word):
            b.stats_to_torch(images=pick, out=bad)
    with pytest.raises(IndexError):
        b.stats_to_torch(images=[-1])
    # the C ABI's refusals on a decoded batch: nothing is written
    ind = (C.c_int * 2)(0, len(world))
    before = block.clone()
    for args, word in (((1, ind, 2, out.data_ptr(), 0, None), "out of range"), ((1, None, 1, None, 0, None), "NULL"), ((1, None, 1, out.data_ptr() + 2, 0, None), "multiple of 4"),
                       ((1, None, 2, out.data_ptr(), WORDS - 1, None), "row_pitch_words"), ((1, None, 1, out.data_ptr(), 0, out.data_ptr() + 1), "totals")):
        assert b._lib.jsnoop_batch_pack_stats(b._h, *args) == -1 and word in J.capi.last_error(), (word, J.capi.last_error())
    b.sync()
    assert torch.equal(block, before)


def test_dc_only_fast_form_and_generic(world):
    """decode_ac = False: the fast layouts are decoded by the DC-only fast form -- last_form() == 2 before and after the call --, gray by the generic kernels."""
    import jpegsnoop_amd as J
    for fast, form in ((True, 2), (False, 1)):
        picks = [i for i, a in enumerate(world) if (a.case.layout in SC.FAST_LAYOUTS) == fast]
        assert len(picks) >= 30
        b = _decoded(J, [world[i].case.file for i in picks], decode_ac=False)
        try:
            assert b.last_form() == form
            rows, tot = b.stats_to_torch(totals=True)
            clip = b.stats_to_torch(histo_en=False)
            assert b.last_form() == form
            rows = rows.cpu().numpy().view(np.uint32); clip = clip.cpu().numpy().view(np.uint32); tot = tot.cpu().numpy()
            errs = []
            _compare(world, picks, rows, "histo_dc", errs, "histo_dc")
            _compare(world, picks, clip, "clip_dc", errs, "clip_dc")
            for k, i in enumerate(picks[::7]):
                assert tot[7 * k].tolist() == world[i].totals("histo_dc"), world[i].case.name
                assert np.array_equal(rows[7 * k], b.color_stats(7 * k))
            assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
            assert np.array_equal(b.stats_all(), rows)
        finally:
            b.close()


def test_refused_without_planes_and_before_the_decode(world):
    import torch
    import jpegsnoop_amd as J
    dst = torch.full((2, WORDS), -5, dtype=torch.int32, device="cuda")
    b = _decoded(J, [world[0].case.file, world[1].case.file], want_planes=False)
    try:
        with pytest.raises(RuntimeError, match="keeps no planes"):
            b.stats_to_torch(out=dst)
        with pytest.raises(RuntimeError, match="keeps no planes"):
            b.stats_all()
    finally:
        b.close()
    b = J.JpegBatch(want_planes=True)
    try:
        b.add_jpeg(world[0].case.file); b.add_jpeg(world[1].case.file)
        assert b._lib.jsnoop_batch_pack_stats(b._h, 1, None, 2, dst.data_ptr(), 0, None) == -1 and "has not been decoded" in J.capi.last_error()
        b.upload()
        assert b._lib.jsnoop_batch_pack_stats(b._h, 1, None, 2, dst.data_ptr(), 0, None) == -1 and "has not been decoded" in J.capi.last_error()
        host = np.full((2, WORDS), 9, np.uint32)
        assert b._lib.jsnoop_batch_read_stats(b._h, 1, None, 2, host.ctypes.data) == -1 and (host == 9).all()
    finally:
        b.close()
    torch.cuda.synchronize()
    assert bool((dst == -5).all().item()), "a refused call writes nothing"


def test_the_cpp_facade(world, full, tmp_path):
    """CJPEGsnoopCoreGpu::BatchPackStats (tests/cpp/stats_demo.cpp): files listed backwards, a pitch above the row, totals."""
    _b, rows, tot, clip = full
    exe = os.path.join(ROOT, "tests", "cpp", "stats_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stats_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    names = ["b_total_11", "s_444_520x16", "o_eleven_rows_one_event_each", "m_003_444_16", "l_420_528x16"]
    picks = [next(i for i, a in enumerate(world) if a.case.name == n) for n in names]
    paths = []
    for i in picks:
        p = tmp_path / ("%d.jpg" % i); p.write_bytes(world[i].case.file); paths.append(str(p))
    from oracle import harness as H
    for histo_en, ref in ((1, rows), (0, clip)):
        out = subprocess.check_output([exe, str(histo_en)] + paths, text=True).strip().splitlines()
        assert len(out) == len(picks)
        for k, line in enumerate(out):
            w = line.split(); j = len(picks) - 1 - k
            assert int(w[0]) == j and w[1] == "%016x" % H.fnv1a64(ref[picks[j]].tobytes()) and [int(x) for x in w[2:]] == tot[picks[j]].tolist(), (histo_en, line)


def test_job_file_result_inside_the_callback(harness, oracle, world, full):
    """A JpegJob with want_planes over baseline files and a progressive one: the rows taken inside the callback.  The progressive file carries the
    coefficients of its baseline twin (tests/golden/make_pillow_progressive.py): its row is the oracle's record of the twin."""
    import jpegsnoop_amd as J
    _b, rows, tot, _clip = full
    picks = [next(i for i, a in enumerate(world) if a.case.name == n) for n in ("o_total_10", "a_420_512x240", "m_006_gray_8")]
    prog = open(os.path.join(ROOT, "tests", "golden", "pillow", "p420_96x64_prog.jpg"), "rb").read()
    twin = SimpleNamespace(name="p420_96x64", file=open(os.path.join(ROOT, "tests", "golden", "pillow", "p420_96x64_base.jpg"), "rb").read(), rerenders=[])
    job = J.JpegJob(devices=[0], want_planes=True)
    seen = {}
    try:
        for i in picks:
            job.add(world[i].case.file)
        job.add(prog); job.add(b"not a jpeg")

        def on_file(r):
            if r.status == "ok":
                t, n = r.stats_to_torch(totals=True)
                seen[r.index] = (t.cpu().numpy().view(np.uint32), n.cpu().numpy(), r.batch.color_stats(r.image), r.kind)
            else:
                with pytest.raises(RuntimeError):
                    r.stats_to_torch()
            return False

        job.run(on_file)
    finally:
        job.close()
    assert sorted(seen) == [0, 1, 2, 3] and seen[3][3] == "progressive"
    for k, i in enumerate(picks):
        assert seen[k][0].shape == (1, WORDS) and np.array_equal(seen[k][0][0], rows[i]) and np.array_equal(seen[k][1][0], tot[i]), world[i].case.name
    assert np.array_equal(seen[3][0][0], seen[3][2]) and int(seen[3][0][0][36]) == 96 * 64, "a progressive image: the per-image door's words"
    assert np.array_equal(seen[3][0][0], run_passes(harness, oracle, twin, "histo")["words"][0]), "... and the oracle's for its baseline twin"


# ------------------------------------------------------------------------------------------------------------------ the deal: a wave walks several units and records
def _deal_case(pic, k, long_one):
    """A picture of tests/deal_cases.py as a stats_cases.Case: every block a level of its own; range events in every second short picture (a block of
    one component) and in the LAST block of a long one -- its last picture rows, which a wave reaches at the end of a long walk through the record."""
    layout, w, h = pic
    fr = SC.frame_of(layout, w, h); rng = np.random.default_rng(7000 + k); g = SC._grids(fr)
    for c in range(fr.ncomp):
        g[c][:] = rng.integers(-1000, 1001, g[c].shape)
    if long_one or k % 2 == 0:
        c = k % fr.ncomp
        g[c][-1, -1] = SC.OVER if k % 4 < 2 else SC.UNDER
    return SC.Case("deal_%s_%dx%d" % pic, "D", layout, w, h, g)


def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records(harness, oracle, gpu, capsys):
    """The catalogue above is a few hundred units: a share of four, a unit a wave, one flush at the end.  Here both forms of k_stats_batch get a call sized
    from the device (tests/deal_cases.py, proven on the CPU by tests/test_deal_cases.py): a share of twelve units and more, a wave that carries its
    accumulators and its LDS histogram over several units of one picture, flushes them into that picture's row when the walk leaves it and goes on into
    the next picture, shares that start inside pictures and on their first row.  A record is at least eight picture rows -- two steps of a wave --, so no
    step passes over a record here; three pictures in one share is what can be had.  A dozen distinct pictures listed many times; every row, every
    total and (through k_stats_order's budget, which reads rowcnt) every event's picture row against the oracle's words."""
    import torch
    import jpegsnoop_amd as J
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lists = {form: D.stats_records(cus, form) for form in ("hist", "plain")}
    for form, recs in lists.items():
        c = D.census_of("stats", form, recs, cus)
        with capsys.disabled():
            print("\nk_stats_batch<%s>, %d compute units: %s" % (form, cus, D.summary(c)))
        assert D.missing(c, D.KERNELS["stats"]["waves"], **D.conditions("stats", form)) == [], D.summary(c)
    distinct = sorted({r.pic for recs in lists.values() for r in recs})
    longs = {r.pic for recs in lists.values() for r in recs if r.units >= 40 * D.STATS_STEP}
    answers = [Answer(harness, oracle, _deal_case(p, k, p in longs)) for k, p in enumerate(distinct)]
    for p, a in zip(distinct, answers):
        assert D.stats_sizes(p) == ([BC.UNIT] * (-(-a.case.img_x // BC.UNIT) - 1) + [a.case.img_x - BC.UNIT * (-(-a.case.img_x // BC.UNIT) - 1)]) * a.case.img_y, p
        ev = sum(a.totals("histo"))
        assert (ev > 0) == (p in longs or distinct.index(p) % 2 == 0) and (p not in longs or ev > 10), (p, ev)
    b = _decoded(J, [a.case.file for a in answers])
    try:
        errs = []
        for form, recs in lists.items():
            picks = [distinct.index(r.pic) for r in recs]
            if form == "hist":
                rows, tot = b.stats_to_torch(images=picks, totals=True)
            else:
                rows, tot = b.stats_to_torch(images=picks, histo_en=False, totals=True)
            rows = rows.cpu().numpy().view(np.uint32); tot = tot.cpu().numpy()
            assert rows.shape == (len(recs), WORDS) and tot.shape == (len(recs), 6)
            _compare(answers, picks, rows, "histo" if form == "hist" else "clip", errs, form)
            want = {i: answers[i].totals("histo") for i in set(picks)}
            errs += ["%s row %d (%s): totals %s, the model's events by kind %s" % (form, k, distinct[i], tot[k].tolist(), want[i]) for k, i in enumerate(picks) if tot[k].tolist() != want[i]]
        assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))
    finally:
        b.close()

