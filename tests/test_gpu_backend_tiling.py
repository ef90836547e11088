"""-m gpu: the back end (k_idct_color, jsnoop_kernels.hip) across MCUs per wave, layouts and its pixel reductions, against the oracle.

upload() gives every image max(1, ceil(nmcu / (8 * mcus_per_wave))) workgroups of 8 waves; a workgroup owns a contiguous range of
ceil(nmcu / workgroups) MCUs and its waves step through it 8 apart (back_end_pairs).  With the automatic choice and the suite's usual
sizes that is one MCU per wave, so the loop runs at most once and neither the prefetch of the next MCU, the hand vmcnt waits across the
back edge, the mx / my stepping nor the last round's re-fetch is exercised.  Here the tuning field mcus_per_wave drives the loop
through many rounds, for each one-layout kernel <1..4> (one layout per batch) and for the any-layout kernel <0> (gray, 4x4 sampling, and
every layout under JSNOOP_XC_BACKEND_GENERIC); the grid's reach is computed from the same rule and asserted, so it cannot shrink unnoticed.

Every decode is compared with the oracle: the DIB byte for byte, the int16 planes when they are kept, the ten bright_avg ints (brightest
pixel's Y / Cb / Cr, RGB and MCU, average Y; the batch API returns them where the planes are kept, or for gray) and, where noted, the
colour statistics."""
import ctypes as C

import numpy as np
import pytest

import backend_images as BI

pytestmark = pytest.mark.gpu

FAST = {"420": 1, "422": 2, "440": 3, "444": 4}                  # layout -> k_idct_color<LAYOUT> of a one-layout batch
SHAPES = [(1, 1), (1, 37), (2, 9), (3, 11), (7, 5), (8, 8), (9, 7), (41, 3)]   # (MCUs across, MCUs down)
MPW = [0, 1, 2, 3, 7, 64, 4096]


# ------------------------------------------------------------------------------------------------ the work split of upload()
def auto_mpw(total_mcus):
    return min(64, max(1, -(-total_mcus // (8 * 1024))))


def wgs_of(nmcu, mpw):
    return max(1, -(-nmcu // (8 * mpw)))


def wave_loops(nmcu, mpw):
    """Iterations of back_end_pairs' MCU loop for every wave of the image: [(workgroup range length, [loops of waves 0..7])]."""
    wgs = wgs_of(nmcu, mpw)
    per = -(-nmcu // wgs)
    out = []
    for g in range(wgs):
        b, e = g * per, min(g * per + per, nmcu)
        n = max(0, e - b)
        out.append((n, [max(0, -(-(n - w) // 8)) for w in range(8)]))
    return out


def reach(shapes_mcus, mpw):
    """What one batch of images with these (xmax, ymax) drives the loop through."""
    eff = mpw if mpw > 0 else auto_mpw(sum(x * y for x, y in shapes_mcus))
    r = {"max_loops": 0, "mid_round_end": False, "idle_waves": False, "narrow_multi": False}
    for xmax, ymax in shapes_mcus:
        for n, loops in wave_loops(xmax * ymax, eff):
            r["max_loops"] = max(r["max_loops"], max(loops))
            r["mid_round_end"] |= n > 8 and n % 8 != 0
            r["idle_waves"] |= min(loops) == 0
            r["narrow_multi"] |= xmax < 8 and max(loops) > 1
    return r


mcu_size = BI.mcu_size


def grid_images(H, layout):
    """The shapes in MCUs plus one size that is not a multiple of the MCU in pixels; (jpeg, (xmax, ymax))."""
    hs, vs, gray = BI.LAYOUTS[layout]
    mw, mh = mcu_size(layout)
    out = []
    for i, (xm, ym) in enumerate(SHAPES + [(13, 6)]):
        w, h = xm * mw, ym * mh
        if (xm, ym) == (13, 6):
            w, h = w - 5, h - 3
        out.append((H.synth_jpeg(width=w, height=h, hs=hs, vs=vs, gray=gray, quality=88, seed=300 + i), (xm, ym)))
    return out


def grid_reach():
    shapes = SHAPES + [(13, 6)]
    return {mpw: reach(shapes, mpw) for mpw in MPW}


# ------------------------------------------------------------------------------------------------ oracle and batch plumbing
_ORACLE = {}


def oracle_result(H, oracle, data, decode_ac=1):
    key = (H.hash_bytes(data), decode_ac)
    if key not in _ORACLE:
        oracle.set_options(decode_ac=decode_ac)
        try:
            H.drive(oracle, data)
            _ORACLE[key] = {"dib": oracle.dib(), "planes": oracle.planes(), "bright_avg": oracle.bright_avg()}
        finally:
            oracle.set_options()
    return _ORACLE[key]


def run_batch(files, mpw, want_planes=False, xc=0, decode_ac=True, split=None):
    import jpegsnoop_amd as J
    b = J.JpegBatch(want_planes=want_planes, decode_ac=decode_ac)
    b.set_tuning(mcus_per_wave=mpw, cross_checks=xc)
    for f in files:
        b.add_jpeg(f)
    if split:
        b.set_split(split)
    b.upload(); b.decode(); b.sync()
    return b


def check_batch(H, oracle, b, files, want_planes=False, decode_ac=1, what=""):
    import jpegsnoop_amd as J
    sums = b.dib_checksums()
    for i, data in enumerate(files):
        want = oracle_result(H, oracle, data, decode_ac)
        inf = b.info(i)
        assert inf["path"] == 1 and inf["flags"] == 0, (what, i, "the parallel path (and the back end under test) must decode it")
        dib = b.dib(i)
        assert np.array_equal(dib, want["dib"]), (what, i, "DIB differs in %d bytes" % int((dib != want["dib"]).sum()))
        assert int(sums[i]) == J.dib_checksum_numpy(want["dib"]), (what, i)
        if want_planes:
            for c, (pa, pb) in enumerate(zip(want["planes"], b.planes(i))):
                if pa is not None:
                    assert np.array_equal(pa, pb), (what, i, "plane %d differs" % c)
        if want_planes or inf["ncomp"] == 1:                      # (the brightest pixel's Cb / Cr / RGB are read from the planes)
            got = b.side_outputs(i)["bright_avg"]
            assert got == want["bright_avg"], (what, i, got, want["bright_avg"])


# ------------------------------------------------------------------------------------------------ a / b: the grid
@pytest.mark.parametrize("xc", [0, 1], ids=["own_kernel", "xc_backend_generic"])
@pytest.mark.parametrize("layout", list(BI.LAYOUTS))
def test_grid_over_the_mcu_loop(harness, oracle, layout, xc):
    """Each layout's shapes in one batch, at every mcus_per_wave, with and without the planes; xc = 1 runs the same through the any-layout
    kernel (JSNOOP_XC_BACKEND_GENERIC).  Plus DC-only decodes (decode_ac = 0) at 3 and 4096 MCUs per wave."""
    import jpegsnoop_amd as J
    assert J.capi.XC_BACKEND_GENERIC == 1
    imgs = grid_images(harness, layout)
    files = [d for d, _ in imgs]
    for d, (xm, ym) in imgs:                                      # the shapes are what the reach computation assumes
        p = harness.parse_jpeg(d)
        mw, mh = mcu_size(layout)
        assert (-(-p.x // mw), -(-p.y // mh)) == (xm, ym)
    for mpw in MPW:
        for want_planes in (False, True):
            b = run_batch(files, mpw, want_planes=want_planes, xc=xc)
            try:
                check_batch(harness, oracle, b, files, want_planes=want_planes, what=(layout, mpw, want_planes, xc))
            finally:
                b.close()
    for mpw in (3, 4096):
        b = run_batch(files, mpw, want_planes=True, xc=xc, decode_ac=False)
        try:
            check_batch(harness, oracle, b, files, want_planes=True, decode_ac=0, what=(layout, mpw, "dc_only", xc))
        finally:
            b.close()
    if layout in FAST:
        r = grid_reach()
        assert max(v["max_loops"] for v in r.values()) >= 3, r          # a wave that runs its loop three times or more
        assert any(v["mid_round_end"] for v in r.values()), r           # a range that ends in the middle of a round of 8 waves
        assert any(v["idle_waves"] for v in r.values()), r              # waves with nothing to do
        assert any(v["narrow_multi"] for v in r.values()), r            # fewer than 8 MCUs across and more than one iteration (mx / my wrap)
        assert r[1]["max_loops"] == 1 and r[4096]["max_loops"] >= 16, r


def _single_tuning(lib, h, **kw):
    import jpegsnoop_amd as J
    t = J.capi.Tuning()
    lib.jsnoop_tuning_defaults(C.byref(t))
    for k, v in kw.items():
        setattr(t, k, v)
    assert lib.jsnoop_set_tuning(C.c_void_p(h), C.byref(t)) == 0, J.last_error()


@pytest.mark.parametrize("mpw", [1, 3, 4096])
def test_preview_modes_and_shift_through_the_mcu_loop(harness, oracle, gpu, mpw):
    """Preview modes 2..4 and a YCC shift whose first shifted MCU lies inside a wave's range of MCUs -- the general colour path of k_idct_color<0>
    (the single-image decoder, jsnoop_set_tuning) -- at one, three and 4096 MCUs per wave."""
    data = harness.synth_jpeg(width=176, height=112, seed=41)     # 11 x 7 MCUs of 4:2:0
    _single_tuning(gpu.lib, gpu.h, mcus_per_wave=mpw, cross_checks=1)
    try:
        for b in (oracle, gpu):
            harness.drive(b, data)
        assert gpu.lib.jsnoop_last_path(gpu.h) == 1
        assert np.array_equal(gpu.dib(), oracle.dib()) and gpu.bright_avg() == oracle.bright_avg()
        for mode in (2, 3, 4):
            for b in (oracle, gpu):
                b.set_preview_mode(mode)
            assert np.array_equal(gpu.dib(), oracle.dib()), (mpw, mode)
        for b in (oracle, gpu):
            b.set_preview_mode(1)
            b.set_preview_ycc_offset(5, 2, 160, -80, 40)          # MCU 27: the fourth of wave 3's at one workgroup, mid-range at any
        assert np.array_equal(gpu.dib(), oracle.dib()), mpw
    finally:
        for b in (oracle, gpu):
            b.set_preview_ycc_offset(0, 0, 0, 0, 0)
            b.set_preview_mode(1)
        _single_tuning(gpu.lib, gpu.h)


# ------------------------------------------------------------------------------------------------ c: two halves, two layouts
def test_split_halves_with_different_layouts(harness, oracle):
    """k x 4:4:4, then k x 4:2:2 with split = 2: the halves run k_idct_color<4> and <2> on two streams.  One 4:2:2 image spreads over more than
    64 workgroups at one MCU per wave, so only the second half folds per-workgroup records (k_status_reduce); the first keeps the atomics."""
    k = 4
    first = [harness.synth_jpeg(width=160, height=120, hs=1, vs=1, seed=60 + i) for i in range(k)]          # 20 x 15 = 300 MCUs: 38 workgroups
    second = [harness.synth_jpeg(width=200 + 16 * i, height=72, hs=2, vs=1, seed=70 + i) for i in range(k - 1)]
    second.append(harness.synth_jpeg(width=640, height=480, hs=2, vs=1, seed=79))                           # 40 x 60 MCUs: 300 workgroups
    files = first + second
    assert max(wgs_of(20 * 15, 1) for _ in first) <= 64 and wgs_of(40 * 60, 1) > 64
    b = run_batch(files, 1, want_planes=True, split=2)
    try:
        assert b.split_parts() == 2
        check_batch(harness, oracle, b, files, want_planes=True, what="split")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ d: brightest pixel and average Y
def _fold(nmcu, mpw):
    return wgs_of(nmcu, mpw) > 64


def _nmcu(data, layout, H):
    p = H.parse_jpeg(data)
    mw, mh = mcu_size(layout)
    return -(-p.x // mw) * -(-p.y // mh)


@pytest.mark.parametrize("mpw", [1, 4096])
def test_flat_images_tie_everywhere(harness, oracle, mpw):
    """White, black and mid-grey fields in every layout: every pixel ties for the brightest, which must be the first in raster order, MCU (0,0).
    One MCU per wave takes the per-workgroup records and the fold, 4096 the atomics."""
    for layout in BI.LAYOUTS:
        files = [BI.flat(harness, layout, c) for c in BI.COLOURS]
        assert _fold(_nmcu(files[0], layout, harness), mpw) == (mpw == 1)
        b = run_batch(files, mpw, want_planes=True)
        try:
            check_batch(harness, oracle, b, files, want_planes=True, what=("flat", layout, mpw))
            for i in range(len(files)):
                assert b.side_outputs(i)["bright_avg"][7:9] == [0, 0]
        finally:
            b.close()


@pytest.mark.parametrize("mpw", [1, 4096])
def test_raster_order_beats_decode_order(harness, oracle, mpw):
    """MCU (0,0) is bright only in its lower luma blocks, MCU (9,0) -- another workgroup at one MCU per wave, another wave at 4096 -- only in
    its upper-left one: the first maximum in raster order is in MCU (9,0)."""
    for layout in ("420", "440"):
        files = [BI.raster_tie(harness, layout)]
        assert _fold(_nmcu(files[0], layout, harness), mpw) == (mpw == 1)
        assert oracle_result(harness, oracle, files[0])["bright_avg"][7:9] == [9, 0]
        b = run_batch(files, mpw, want_planes=True)
        try:
            check_batch(harness, oracle, b, files, want_planes=True, what=("raster", layout, mpw))
        finally:
            b.close()


@pytest.mark.parametrize("mpw", [1, 4096])
def test_average_y_sum_wraps(harness, oracle, mpw):
    """Flat white of 4160 x 4096 pixels (Y = 255 each) in 4:2:0 and gray: the reference's unsigned luminance sum wraps past 2^32."""
    w, h = BI.WRAP_SIZE
    for layout in ("420", "gray"):
        files = [BI.flat(harness, layout, "white", BI.WRAP_SIZE)]
        assert _fold(_nmcu(files[0], layout, harness), mpw) == (mpw == 1)
        want = oracle_result(harness, oracle, files[0])["bright_avg"]
        assert want[9] < 255 and want[9] == (w * h * 255 % 2 ** 32) // ((w + 1) * (h + 1)), want
        b = run_batch(files, mpw, want_planes=True)
        try:
            check_batch(harness, oracle, b, files, want_planes=True, what=("wrap", layout, mpw))
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------ e: colour statistics
@pytest.mark.parametrize("layout", ["420", "444", "gray"])
def test_color_stats_of_saturated_fields(harness, oracle, gpu, layout):
    """Fields of pure R, G, B, white, black and magenta over several workgroups: the DIB and the colour statistics with bHistoEn on, and with
    bStatClipEn alone, through the single-image decoder and the batch, against the oracle."""
    data = BI.fields(harness, layout)
    for mpw in (1, 4096):
        _single_tuning(gpu.lib, gpu.h, mcus_per_wave=mpw)
        try:
            for opt in (dict(histo_en=1), dict(stat_clip_en=1)):
                for b in (oracle, gpu):
                    b.set_options(**opt)
                    harness.drive(b, data)
                assert np.array_equal(gpu.dib(), oracle.dib()), (layout, mpw, opt)
                assert np.array_equal(BI.stats_words(gpu.color_stats()), BI.stats_words(oracle.color_stats())), (layout, mpw, opt)
                assert gpu.bright_avg() == oracle.bright_avg(), (layout, mpw, opt)
        finally:
            for b in (oracle, gpu):
                b.set_options()
            _single_tuning(gpu.lib, gpu.h)
        batch = run_batch([data], mpw, want_planes=True)
        try:
            check_batch(harness, oracle, batch, [data], want_planes=True, what=("fields", layout, mpw))
            for histo_en in (1, 0):
                oracle.set_options(histo_en=histo_en, stat_clip_en=1 - histo_en)
                try:
                    harness.drive(oracle, data)
                    want = BI.stats_words(oracle.color_stats())
                finally:
                    oracle.set_options()
                assert np.array_equal(batch.color_stats(0, histo_en=bool(histo_en)), want), (layout, mpw, histo_en)
        finally:
            batch.close()
