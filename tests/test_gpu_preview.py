"""-m gpu: the back end's general colour path -- back_end_mcus<false,1,1> -> mcu_to_dib<RGB_ONLY> -> ycc_to_bgra / channel_extract, the one every
preview mode other than RGB and every YCC shift goes through -- against the oracle, on the catalogue of tests/preview_cases.py (every layout, the
start MCUs at the edges of the picture, of a wave's MCUs and of a workgroup, magnitudes that saturate and that leave the int16 range).

  a  re-render of a decoded image (jsnoop_set_preview_mode / _ycc_offset -> JsnoopDecoder::rerender) at 1, 3 and the automatic MCUs per wave
  b  the state set BEFORE the decode (js_describe_image copies it), every case again at the same three settings: parallel path, progressive;
     a damaged golden file on the exact-mirror path and repaired on the parallel path
  c  DC-only: the fast form (k_dc_color) must give way to the generic kernels when a state arrives, and come back to the same pixels
  d  one batch that holds default-state images (fast forms) and images with a state side by side, under split, MCUs per wave, the cross-check
  e  DC-only batches: which states keep the fast form
  f  what is downstream of such a batch: the pack sees the preview rendering; planes, coefficients, histograms and the export do not

Every comparison is exact (np.array_equal / ==).  The truth is the oracle driven on the same file with the same state (computed once per
(picture, state), shared); only the progressive picture, which the oracle refuses, is compared with tests/preview_model.py on the decoder's own
planes -- the model is pinned to the oracle in tests/test_preview_cases.py."""
import ctypes as C

import numpy as np
import pytest

import backend_images as BI
import preview_cases as PC
import preview_model as PM
from test_gpu_backend_tiling import _single_tuning

pytestmark = pytest.mark.gpu

D = PM.DEFAULT
_ORC = {}


def set_state(b, st):
    b.set_preview_mode(st[0])
    b.set_preview_ycc_offset(*st[1:])


def oracle_state(H, oracle, pic, st, decode_ac=1, histo=0):
    """What the oracle makes of the picture under the state (set before its decode; tests/test_preview_cases.py shows that setting it afterwards
    gives the same): DIB, bright_avg, the planes (never shifted) and with histo the statistics record.  Once per key."""
    key = (pic.name, st, decode_ac, histo)
    if key not in _ORC:
        oracle.set_options(decode_ac=decode_ac, histo_en=histo)
        try:
            set_state(oracle, st)
            PC.oracle_drive(H, oracle, pic)
            r = {"dib": oracle.dib(), "bright_avg": oracle.bright_avg(), "planes": oracle.planes()}
            if histo:
                r["stats"] = BI.stats_words(oracle.color_stats())
            _ORC[key] = r
        finally:
            set_state(oracle, D)
            oracle.set_options()
    return _ORC[key]


def decode(H, gpu, pic):
    if pic.progressive:
        assert gpu.decode_progressive(pic.data) > 0, gpu.lib.jsnoop_last_error()
        assert gpu.lib.jsnoop_last_path(gpu.h) == 3 and gpu.lib.jsnoop_last_flags(gpu.h) == 0
    else:
        H.drive(gpu, pic.data, pic.parsed)


def truth_of(H, oracle, gpu, pic):
    """state -> (DIB, bright_avg).  The progressive picture: the model on the planes the decoder holds now."""
    if not pic.progressive:
        return lambda st: (lambda r: (r["dib"], r["bright_avg"]))(oracle_state(H, oracle, pic, st))
    planes = PM.planes_of(gpu)

    def model(st):
        dib, sum_y = PM.expect(oracle, planes, pic.mcu_w, pic.mcu_h, st, with_sum=True)
        return dib, PM.bright_avg(oracle, planes, pic.mcu_w, pic.mcu_h, sum_y)
    return model


def check(gpu, want, what):
    dib = gpu.dib()
    assert dib.shape == want[0].shape and np.array_equal(dib, want[0]), (what, "DIB differs in %d bytes" % int((dib != want[0]).sum()))
    assert gpu.bright_avg() == want[1], (what, gpu.bright_avg(), want[1])


# ------------------------------------------------------------------------------------------------ a: re-render
@pytest.mark.parametrize("mpw", [1, 3, None], ids=["mpw1", "mpw3", "mpw_auto"])
@pytest.mark.parametrize("name", list(PC.LAYOUTS))
def test_rerender_every_case(harness, oracle, gpu, name, mpw):
    """Every state of the catalogue on the decoded picture, DIB and bright_avg (brightest pixel from the unshifted Y, average from the shifted)
    after every change; back in the default state the first DIB must be there again."""
    pic = PC.picture(harness, name)
    _single_tuning(gpu.lib, gpu.h, **({} if mpw is None else dict(mcus_per_wave=mpw)))
    try:
        decode(harness, gpu, pic)
        if not pic.progressive and name not in PC.PARTIAL:
            assert gpu.lib.jsnoop_last_path(gpu.h) == 1 and gpu.lib.jsnoop_last_flags(gpu.h) == 0
        truth = truth_of(harness, oracle, gpu, pic)
        first = gpu.dib()
        check(gpu, truth(D), (name, mpw, "decode"))
        now = D
        for st in PC.cases_of(name):
            if st[0] != now[0]:
                gpu.set_preview_mode(st[0])
            if st[1:] != now[1:]:
                gpu.set_preview_ycc_offset(*st[1:])
            now = st
            check(gpu, truth(st), (name, mpw, st))
        set_state(gpu, D)
        assert np.array_equal(gpu.dib(), first), (name, mpw, "back in the default state")
        check(gpu, truth(D), (name, mpw, "back in the default state"))
    finally:
        set_state(gpu, D)
        _single_tuning(gpu.lib, gpu.h)


# ------------------------------------------------------------------------------------------------ b: the state is there before the decode
@pytest.mark.parametrize("mpw", [1, 3, None], ids=["mpw1", "mpw3", "mpw_auto"])
@pytest.mark.parametrize("name", list(PC.LAYOUTS))
def test_state_set_before_the_decode(harness, oracle, gpu, name, mpw):
    """The first decode goes straight through the general path.  Clean files: the parallel path; the progressive one: its own.  Every state of
    the catalogue, as in part a: each costs a whole decode here, a colour launch there."""
    pic = PC.picture(harness, name)
    _single_tuning(gpu.lib, gpu.h, **({} if mpw is None else dict(mcus_per_wave=mpw)))
    try:
        for st in PC.cases_of(name):
            set_state(gpu, st)
            decode(harness, gpu, pic)
            if not pic.progressive and name not in PC.PARTIAL:
                assert gpu.lib.jsnoop_last_path(gpu.h) == 1 and gpu.lib.jsnoop_last_flags(gpu.h) == 0, (name, st)
            truth = truth_of(harness, oracle, gpu, pic)
            check(gpu, truth(st), (name, st, "preset"))
            if not pic.progressive:
                for c, (pa, pb) in enumerate(zip(oracle_state(harness, oracle, pic, st)["planes"], gpu.planes())):
                    if pa is not None:
                        assert np.array_equal(pa, pb), (name, st, "plane %d: the retained samples are never shifted" % c)
            set_state(gpu, D)
            check(gpu, truth(D), (name, st, "reset after a preset decode"))
    finally:
        set_state(gpu, D)
        _single_tuning(gpu.lib, gpu.h)


@pytest.mark.parametrize("whole_mirror", [True, False], ids=["exact_mirror", "repaired_on_the_parallel_path"])
def test_state_set_before_the_decode_of_a_damaged_file(harness, oracle, gpu, whole_mirror):
    """A golden bad_* file with the state preset, then reset.  tests/golden/bad_marker_420_odd_141x93 (9 x 6 MCUs, a marker in the scan) is flagged
    by the parallel path.  Untuned, a second attempt through the markers of its scan repairs it (jsnoop_last_path stays 1, the flags say so);
    under the cross-check JSNOOP_XC_NO_TAIL the whole image goes through the exact-mirror kernel (jsnoop_last_path == 2) -- untuned, none of
    the golden bad_* files takes that path in the single-image decoder any more."""
    import jpegsnoop_amd as J
    from golden_util import load_case
    name = "bad_marker_420_odd_141x93"
    data = load_case(name)
    _single_tuning(gpu.lib, gpu.h, **(dict(cross_checks=J.capi.XC_NO_TAIL) if whole_mirror else {}))
    try:
        harness.drive(gpu, data)
        assert gpu.lib.jsnoop_last_flags(gpu.h) != 0 and gpu.lib.jsnoop_last_path(gpu.h) == (2 if whole_mirror else 1)
        xmax, ymax = gpu.geometry()[2:4]
        assert (xmax, ymax) == (9, 6)
        states = [(6, xmax // 2, ymax // 2, 160, -80, 40), (1, xmax - 1, ymax - 1, 0, 0, 8), (7, 0, ymax, 160, -80, 40),      # the middle, the last MCU, behind it
                  (2, 0, 0, -30000, 30000, -30000), (1, 3, 1, -8, 0, 0)]
        harness.drive(oracle, data)
        plain = (oracle.dib(), oracle.bright_avg())
        check(gpu, plain, (name, "plain"))
        for st in states:
            for b in (oracle, gpu):
                set_state(b, st)
                harness.drive(b, data)
            assert gpu.lib.jsnoop_last_path(gpu.h) == (2 if whole_mirror else 1), (name, st)
            check(gpu, (oracle.dib(), oracle.bright_avg()), (name, st, "preset"))
            for b in (oracle, gpu):
                set_state(b, D)
            check(gpu, plain, (name, st, "reset"))
    finally:
        for b in (oracle, gpu):
            set_state(b, D)
        _single_tuning(gpu.lib, gpu.h)


# ------------------------------------------------------------------------------------------------ c: DC-only, single image
@pytest.mark.parametrize("name", ["420", "444"])
def test_dc_only_gives_up_the_fast_form_for_a_state(harness, oracle, gpu, name):
    pic = PC.picture(harness, name)
    form = lambda: gpu.lib.jsnoop_last_form(C.c_void_p(gpu.h))
    st = (6, 5, 2, 160, -80, 40)
    try:
        gpu.set_options(decode_ac=0)
        gpu.set_log_callback(type(gpu._log_cb)(), None)            # (a log callback keeps the single-image decoder off the fast form)
        decode(harness, gpu, pic)
        assert form() == 2 and gpu.lib.jsnoop_last_path(gpu.h) == 1
        want = oracle_state(harness, oracle, pic, D, decode_ac=0)
        check(gpu, (want["dib"], want["bright_avg"]), (name, "DC-only, fast form"))
        fast = gpu.dib()
        set_state(gpu, st)
        assert form() == 1, "the re-render reads the coefficient arena: the decode must have been repeated in the generic form"
        want = oracle_state(harness, oracle, pic, st, decode_ac=0)
        check(gpu, (want["dib"], want["bright_avg"]), (name, st, "DC-only"))
        assert not np.array_equal(want["dib"], fast)
        set_state(gpu, D)
        assert np.array_equal(gpu.dib(), fast), (name, "back in the default state")
        set_state(gpu, st)                                        # ... and with the state there before the decode
        decode(harness, gpu, pic)
        assert form() == 1
        check(gpu, (want["dib"], want["bright_avg"]), (name, st, "DC-only, preset"))
    finally:
        gpu.set_log_callback(gpu._log_cb, None)
        set_state(gpu, D)
        gpu.set_options()


# ------------------------------------------------------------------------------------------------ d: one batch, mixed states
MIXED = [("420", D), ("gray", (7, 5, 2, 160, -80, 40)),
         ("444", D), ("411", (2, 0, 0, 0, 0, 8)),
         ("422", D), ("partial_311", (1, 3, 1, -30000, 30000, -30000)),
         ("440", D), ("partial_421", (6, 8, 0, 30000, 0, 0)),
         ("420", D), ("420", (1, 0, 7, 160, -80, 40)),            # starts at the index behind the last MCU: the general path, the fast form's pixels
         ("444", D), ("444", (4, 0, 0, 0, 0, 0)),
         ("422", D), ("422", (1, 9, 1, 0, 0, 8)),
         ("440", D), ("440", (8, 10, 6, 16376, -16376, 16376))]
FAST_HALF_FIRST = [("420", D)] * 8 + MIXED[:8]                   # split = 2: k_idct_color<1> beside k_idct_color<0>
SETTINGS = {"plain": {}, "mpw1": dict(mcus_per_wave=1), "mpw3": dict(mcus_per_wave=3), "xc_backend_generic": dict(cross_checks=1), "split2": dict(split=2)}


@pytest.fixture(scope="module")
def tables(harness, gpu):
    """A decoder object that never decodes: its preview setters only record what jsnoop_batch_add copies into the image."""
    t = harness.Backend(gpu.lib, "jsnoop_", "hip")
    yield t
    t.close()


def state_batch(H, tables, slots, want_planes=True, decode_ac=True, split=None, **tuning):
    import jpegsnoop_amd as J
    b = J.JpegBatch(want_planes=want_planes, decode_ac=decode_ac)
    if tuning:
        b.set_tuning(**tuning)
    try:
        tables.set_options(decode_ac=int(decode_ac))
        for k, (name, st) in enumerate(slots):
            pic = PC.picture(H, name)
            H.push_tables(tables, pic.parsed)
            set_state(tables, st)
            assert b.add(tables.h, pic.data, pic.parsed.scan_start) == k
    finally:
        set_state(tables, D)
        tables.set_options()
    if split:
        b.set_split(split)
    b.upload(); b.decode(); b.sync()
    return b


def check_state_batch(H, oracle, b, slots, what, decode_ac=1, stats=True):
    for i, (name, st) in enumerate(slots):
        pic = PC.picture(H, name)
        want = oracle_state(H, oracle, pic, st, decode_ac=decode_ac)
        dib = b.dib(i)
        assert dib.shape == want["dib"].shape and np.array_equal(dib, want["dib"]), (what, i, name, st, "DIB differs in %d bytes" % int((dib != want["dib"]).sum()))
        assert b.side_outputs(i)["bright_avg"] == want["bright_avg"], (what, i, name, st)
        for c, (pa, pb) in enumerate(zip(want["planes"], b.planes(i))):
            if pa is not None:
                assert np.array_equal(pa, pb), (what, i, name, st, "plane %d: the planes arena holds the unshifted samples" % c)
        if stats:
            assert np.array_equal(b.color_stats(i), oracle_state(H, oracle, pic, st, decode_ac=decode_ac, histo=1)["stats"]), (what, i, name, st, "colour statistics")


@pytest.mark.parametrize("slots", ["mixed", "fast_half_first"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_batch_of_mixed_states(harness, oracle, tables, slots, setting):
    """Default-state images (fast-form eligible) and images whose tables object carried a mode or a shift, in one launch: the LDS tile is the
    largest any image wants (grey, 4:1:1 and the partial layouts decide it), the kernel the any-layout one.  Per image DIB, bright_avg,
    planes and colour statistics (the statistics kernels read the planes arena and add the shift themselves: once) against the oracle, under
    every setting."""
    import jpegsnoop_amd as J
    assert J.capi.XC_BACKEND_GENERIC == 1
    which = MIXED if slots == "mixed" else FAST_HALF_FIRST
    kw = dict(SETTINGS[setting])
    b = state_batch(harness, tables, which, **kw)
    try:
        assert b.last_form() == 1 and (setting != "split2" or b.split_parts() == 2)
        check_state_batch(harness, oracle, b, which, (slots, setting))
    finally:
        b.close()


@pytest.mark.parametrize("slots", ["mixed", "fast_half_first"])
def test_every_setting_gives_the_same_dibs(harness, tables, slots):
    """The DIB checksums of the batch under every setting, side by side in one test (each setting is compared with the oracle above)."""
    which = MIXED if slots == "mixed" else FAST_HALF_FIRST
    sums = {}
    for setting, kw in SETTINGS.items():
        b = state_batch(harness, tables, which, **kw)
        try:
            sums[setting] = [int(x) for x in b.dib_checksums()]
        finally:
            b.close()
    assert all(s == sums["plain"] for s in sums.values()), {k: [i for i, (x, y) in enumerate(zip(s, sums["plain"])) if x != y] for k, s in sums.items()}


# ------------------------------------------------------------------------------------------------ e: DC-only batches
def test_dc_only_batch_keeps_the_fast_form_only_without_a_state(harness, oracle, tables):
    three = ["420"] * 3
    for states, form in (([D, D, D], 2),
                         ([D, (1, 3, 2, 0, 0, 0), D], 2),                       # a start MCU with zero magnitudes shifts nothing
                         ([D, (7, 0, 0, 0, 0, 0), D], 1),
                         ([D, D, (1, 5, 2, 0, 0, 8)], 1),
                         ([(6, 0, 7, 160, -80, 40), D, D], 1)):
        slots = list(zip(three, states))
        b = state_batch(harness, tables, slots, want_planes=True, decode_ac=False)
        try:
            assert b.last_form() == form, states
            check_state_batch(harness, oracle, b, slots, ("dc_only", states), decode_ac=0, stats=False)
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------ f: downstream of the mixed batch
def _outcome(fn):
    try:
        return ("ok", fn())
    except (RuntimeError, ValueError) as e:
        return ("error", str(e))


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if hasattr(a, "cpu"):
        return a.shape == b.shape and bool((a == b).all())
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_downstream_of_the_mixed_batch(harness, oracle, tables):
    """The pack reads the DIB: to_torch gives the preview rendering (tests/pack_model.py on the oracle's DIB of that state).  Planes, coefficient
    tensors, coefficient histograms and the export read the arenas the entropy decode and the IDCT filled: INVARIANCE checks -- the same calls on
    a batch of the same files added in the default state must give the same bytes, per image (the kernels behind them are pinned to the oracle
    in their own modules; a call that refuses an image must refuse it in both batches, with the same words)."""
    from pack_model import pack_model
    b = state_batch(harness, tables, MIXED)
    ref = state_batch(harness, tables, [(name, D) for name, _ in MIXED])
    try:
        packed = b.to_torch()
        for i, (name, st) in enumerate(MIXED):
            inf = b.info(i)
            want = pack_model(oracle_state(harness, oracle, PC.picture(harness, name), st)["dib"], inf["dim_x"], inf["dim_y"])
            assert np.array_equal(packed[i].cpu().numpy(), want), (i, name, st, "the pack must see the preview rendering")
        calls = {"planes_to_torch": lambda x, i: x.planes_to_torch(images=[i], native=True), "coefs_to_torch": lambda x, i: x.coefs_to_torch(images=[i]),
                 "coef_hist_all": lambda x, i: x.coef_hist_all(images=[i]), "export_jpeg": lambda x, i: (x.export_jpeg(images=[i]), [(e["result"], e["detail"], e["len"]) for e in x.export_results()])}
        for what, fn in calls.items():
            for i, (name, st) in enumerate(MIXED):
                got, want = _outcome(lambda: fn(b, i)), _outcome(lambda: fn(ref, i))
                assert got[0] == want[0] and _same(got[1], want[1]), (what, i, name, st, "the preview state reached an output that reads the arenas")
                if name not in PC.PARTIAL:
                    assert got[0] == "ok", (what, i, name, got[1])
        for i, (name, st) in enumerate(MIXED):                     # (against the oracle: check_state_batch of the tests above)
            for pa, pb in zip(ref.planes(i), b.planes(i)):
                assert np.array_equal(pa, pb), (i, name, st)
    finally:
        b.close(); ref.close()
