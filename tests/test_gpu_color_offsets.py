"""-m gpu: the offset form of the 4:2:0 colour phase (k_idct_color<1>: chroma_offsets / mcu_to_dib_offs, jsnoop_kernels.hip) against the oracle.

The back end evaluates ConvertYCCtoRGBFastFloat's chain once per chroma sample and forms a pixel as sat_u8(Y + offset); on the triples listed in
jsnoop_color_exc.h (G one lower, three chroma pairs) a wave votes and the affected pixels look their bit up.  Two things are checked:

* the device functions over all 2^24 clamped triples (jsnoop_color_offsets_sweep) -- 0 differing triples;
* the kernel itself, through JpegBatch and the single-image decoder, on small 4:2:0 pictures that reach what synthetic pictures never do: gray
  (Cb = Cr = 0 everywhere), flat chroma at the two other listed pairs, and a mix in which only some MCUs, and only some samples of an MCU,
  hold a listed pair.  Each picture first proves on the oracle's own planes that it holds triples from the exception set and triples of
  the same chroma pairs outside it.

The pictures come from an encoder fed YCbCr planes directly (Pillow, quality 100: every quantiser is 1, a flat chroma block keeps its value
exactly)."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_color_exc.h")


def exception_set():
    """{(cb, cr): [8 mask words over Y + 128]} as the kernel reads it."""
    txt = open(HDR).read()
    pairs = [tuple(int(v) for v in m) for m in re.findall(r"\{ (-?\d+), (-?\d+) \}", re.search(r"#define JS_COLOR_EXC_CBCR (.*)", txt).group(1))]
    rows = [[int(w, 16) for w in re.findall(r"0x([0-9A-F]{8})u", l)] for l in txt.split("#define JS_COLOR_EXC_MASKS")[1].split("\n") if "0x" in l]
    assert len(pairs) == len(rows) and pairs
    return dict(zip(pairs, rows))


# ------------------------------------------------------------------------------------------------ the device functions, exhaustively
def test_offsets_sweep_equals_the_oracle_on_all_triples(harness, oracle, gpu):
    """All 2^24 clamped (Y, Cb, Cr) triples through chroma_offsets + the pixel of mcu_to_dib_offs (vote, tag and table included) against the
    oracle's ConvertYCCtoRGBFastFloat, one Y plane at a time like test_gpu_parity.py::test_color_sweep: 0 differing triples."""
    out = np.zeros(1 << 24, np.uint32)
    gpu.lib.jsnoop_color_offsets_sweep.restype = C.c_int
    gpu.lib.jsnoop_color_offsets_sweep.argtypes = [C.c_void_p, C.c_void_p]
    assert gpu.lib.jsnoop_color_offsets_sweep(gpu.h, out.ctypes.data_as(C.c_void_p)) == 0
    cb, cr = np.meshgrid(np.arange(-128, 128, dtype=np.int32), np.arange(-128, 128, dtype=np.int32), indexing="ij")
    differing = 0
    for y in range(-128, 128):
        ycc = np.stack([np.full(cb.size, y * 8, np.int32), cb.ravel() * 8, cr.ravel() * 8], -1).copy()
        rgb = np.zeros((ycc.shape[0], 3), np.uint8)
        oracle.lib.orc_color_fast(ycc.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), C.c_size_t(ycc.shape[0]))
        want = rgb[:, 2].astype(np.uint32) | (rgb[:, 1].astype(np.uint32) << 8) | (rgb[:, 0].astype(np.uint32) << 16)
        differing += int((out[(y + 128) << 16:(y + 129) << 16] != want).sum())
    print("differing triples:", differing)
    assert differing == 0


# ------------------------------------------------------------------------------------------------ the pictures
def encode_ycc(y, cb8, cr8):
    """Baseline 4:2:0 JPEG of the given planes (Y 0..255, chroma as Cb8 / Cr8 offsets from 128), no colour conversion, every quantiser 1."""
    from PIL import Image
    a = np.stack([y, 128 + cb8, 128 + cr8], -1).astype(np.uint8)
    f = io.BytesIO()
    Image.fromarray(a, "YCbCr").save(f, "JPEG", quality=100, subsampling=2)
    return f.getvalue()


def ramp(w, h):
    """All 256 luma levels in raster order over w x h pixels."""
    return (np.arange(w * h).reshape(h, w) * 256) // (w * h)


def flat_chroma(w, h, cb8, cr8):
    return encode_ycc(ramp(w, h), np.full((h, w), cb8), np.full((h, w), cr8))


def mixed():
    """4 x 4 MCUs over two ramps; by (mx + my) % 4 an MCU is: all (0, 0) -- none listed (37, 12) -- chroma columns alternating between (0, 0)
    and (20, -20), so that a lane's two chroma samples differ -- upper half (100, -100), lower half (-100, 100)."""
    w = h = 64
    y = np.concatenate([ramp(64, 32), ramp(64, 32)[:, ::-1]])
    cb, cr = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    alt = np.where((np.arange(16) // 2) % 2 == 1, 20, 0)[None, :]
    for my in range(4):
        for mx in range(4):
            k, ys, xs = (my + mx) % 4, slice(my * 16, my * 16 + 16), slice(mx * 16, mx * 16 + 16)
            if k == 1:
                cb[ys, xs], cr[ys, xs] = 37, 12
            elif k == 2:
                cb[ys, xs], cr[ys, xs] = alt, -alt
            elif k == 3:
                cb[my * 16:my * 16 + 8, xs], cr[my * 16:my * 16 + 8, xs] = 100, -100
                cb[my * 16 + 8:my * 16 + 16, xs], cr[my * 16 + 8:my * 16 + 16, xs] = -100, 100
    return encode_ycc(y, cb, cr)


# name -> (builder, the listed pairs the picture must hold)
PICTURES = {
    # (the ramp up, then down again: the decoder truncates, and a single ramp comes back four levels short of 256)
    "gray": (lambda: encode_ycc(np.concatenate([ramp(64, 16), ramp(64, 16)[::-1, ::-1]]), np.zeros((32, 64), np.int64), np.zeros((32, 64), np.int64)), [(0, 0)]),
    "cb+100_cr-100": (lambda: flat_chroma(32, 16, 100, -100), [(100, -100)]),
    "cb-100_cr+100": (lambda: flat_chroma(32, 16, -100, 100), [(-100, 100)]),
    "mixed": (mixed, [(0, 0), (100, -100), (-100, 100)]),
}
_CASES = {}


def census(planes, exc):
    """Per listed pair: (pixels whose triple is in the exception set, pixels of the same pair whose triple is not), and per MCU the listed pixels."""
    py, pcb, pcr = [np.clip(p.astype(np.int32) >> 3, -128, 127) for p in planes]
    out, listed = {}, np.zeros(py.shape, bool)
    for (cb, cr), ws in exc.items():
        sel = (pcb == cb) & (pcr == cr)
        words = np.array(ws, np.uint64)
        yi = (py[sel] + 128).astype(np.uint64)
        bit = (words[yi >> np.uint64(5)] >> (yi & np.uint64(31))) & np.uint64(1)
        out[(cb, cr)] = (int(bit.sum()), int(sel.sum()) - int(bit.sum()))
        listed |= sel
    h, w = py.shape
    per_mcu = listed.reshape(h // 16, 16, w // 16, 16).sum((1, 3))
    return out, per_mcu


def case(H, oracle, name):
    """The picture, what the oracle makes of it, and the proof that it cannot pass vacuously."""
    if name not in _CASES:
        build, pairs = PICTURES[name]
        data = build()
        p = H.parse_jpeg(data)
        assert [(h, v) for _i, h, v, _t in p.comps] == [(2, 2), (1, 1), (1, 1)] and p.sof == 0xC0, "baseline 4:2:0"
        H.drive(oracle, data)
        want = {"dib": oracle.dib(), "planes": oracle.planes(), "bright_avg": oracle.bright_avg()}
        counts, per_mcu = census(want["planes"], exception_set())
        for pair in pairs:
            inside, outside = counts[pair]
            assert inside > 0 and outside > 0, (name, pair, counts)
        if name == "gray":
            assert len(np.unique(np.clip(want["planes"][0] >> 3, -128, 127))) == 256       # Y covers all 256 levels
            assert (per_mcu == 256).all()
        if name == "mixed":                                      # MCUs with no listed sample, with all, and with only some
            assert (per_mcu == 0).any() and (per_mcu == 256).any() and ((per_mcu > 0) & (per_mcu < 256)).any(), per_mcu
            py, pcb, pcr = [np.clip(q.astype(np.int32) >> 3, -128, 127) for q in want["planes"]]
            zero = (pcb == 0) & (pcr == 0)
            quad = zero.reshape(zero.shape[0], -1, 4)           # a lane's four pixels: its two chroma samples must differ somewhere
            assert (quad[..., 0] != quad[..., 2]).any()
        _CASES[name] = (data, want)
    return _CASES[name]


def run_batch(files, want_planes, mpw=0):
    import jpegsnoop_amd as J
    b = J.JpegBatch(want_planes=want_planes)
    b.set_tuning(mcus_per_wave=mpw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


# ------------------------------------------------------------------------------------------------ inside the kernel
@pytest.mark.parametrize("name", list(PICTURES))
def test_single_image_decode(harness, oracle, gpu, name):
    """DIB, brightest pixel and average Y (the luminance sum over the pixel count) of the single-image decoder."""
    data, want = case(harness, oracle, name)
    harness.drive(gpu, data)
    assert gpu.lib.jsnoop_last_path(gpu.h) == 1
    dib = gpu.dib()
    assert np.array_equal(dib, want["dib"]), (name, "DIB differs in %d bytes" % int((dib != want["dib"]).sum()))
    assert gpu.bright_avg() == want["bright_avg"], name
    for pa, pb in zip(want["planes"], gpu.planes()):
        assert np.array_equal(pa, pb), name


@pytest.mark.parametrize("mpw", [0, 3], ids=["one_mcu_per_wave", "three_mcus_per_wave"])
@pytest.mark.parametrize("want_planes", [False, True], ids=["dib_only", "with_planes"])
def test_batch_decode(harness, oracle, want_planes, mpw):
    """All pictures in one batch of k_idct_color<1>, without and with the planes (which must be unchanged: the chroma blocks stay in the tile for
    them), at one MCU per wave and with waves that loop: a vote must not outlive its MCU."""
    import jpegsnoop_amd as J
    names = list(PICTURES)
    cases = [case(harness, oracle, n) for n in names]
    b = run_batch([d for d, _ in cases], want_planes, mpw)
    try:
        sums = b.dib_checksums()
        for i, (name, (_data, want)) in enumerate(zip(names, cases)):
            inf = b.info(i)
            assert inf["path"] == 1 and inf["flags"] == 0, (name, inf)
            dib = b.dib(i)
            assert np.array_equal(dib, want["dib"]), (name, "DIB differs in %d bytes" % int((dib != want["dib"]).sum()))
            assert int(sums[i]) == J.dib_checksum_numpy(want["dib"]), name
            if want_planes:
                for pa, pb in zip(want["planes"], b.planes(i)):
                    assert np.array_equal(pa, pb), (name, "plane differs")
                assert b.side_outputs(i)["bright_avg"] == want["bright_avg"], name          # brightest pixel, and the luminance sum as the average Y
    finally:
        b.close()
