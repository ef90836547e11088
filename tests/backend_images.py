"""Pictures with chosen pixels for the back end's reductions (brightest pixel, average Y, colour statistics), shared by
tests/test_gpu_backend_tiling.py, tests/test_backend_reductions_golden.py and tests/golden/make_backend_reductions.py.

Flat 8x8 luma blocks carry only a DC coefficient, so every sample of such a block decodes to the same value: identical flat
bright blocks tie exactly, whatever the quantisation."""
import numpy as np

# sampling of each layout: (hs, vs, gray); the four one-layout kernels k_idct_color<1..4> and two of the any-layout kernel's
LAYOUTS = {"420": (2, 2, 0), "422": (2, 1, 0), "440": (1, 2, 0), "444": (1, 1, 0), "gray": (1, 1, 1), "h4v4": (4, 4, 0)}
FLAT_MCUS = (24, 23)            # MCUs across, down of the flat fields: 552 > 512 (the fold at one MCU per wave needs 65 workgroups)
WRAP_SIZE = (4160, 4096)        # 17 039 360 pixels at Y = 254: the unsigned luminance sum wraps (:4635)
COLOURS = {"white": (255, 255, 255), "black": (0, 0, 0), "grey": (128, 128, 128)}
FIELDS = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0), (255, 0, 255)]


def encode(H, rgb, layout, quality=90):
    hs, vs, gray = LAYOUTS[layout]
    return H.encode_rgb(rgb, hs=hs, vs=vs, quality=quality, gray=gray)


def mcu_size(layout):
    hs, vs, gray = LAYOUTS[layout]
    return (8, 8) if gray else (8 * hs, 8 * vs)


def flat(H, layout, colour, size=None):
    mw, mh = mcu_size(layout)
    w, h = size or (FLAT_MCUS[0] * mw, FLAT_MCUS[1] * mh)
    return encode(H, np.broadcast_to(np.array(COLOURS[colour], np.uint8), (h, w, 3)), layout)


def raster_tie(H, layout, k=9):
    """MCU (0,0) bright only in its lower luma blocks, MCU (k,0) only in its upper-left one: both white, the rest black.  The reference scans
    in raster order and keeps the first maximum (strict >, :4724), so MCU (k,0) wins although MCU (0,0) is decoded first.  (Vertical layouts:
    4:2:0, 4:4:0.)"""
    hs, vs, _ = LAYOUTS[layout]
    assert vs == 2
    mw, mh = 8 * hs, 16
    w, h = 32 * mw, 18 * mh                                       # 576 MCUs
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[8:16, 0:mw] = 255
    rgb[0:8, k * mw:k * mw + 8] = 255
    return encode(H, rgb, layout)


def fields(H, layout, band=64, height=256):
    """Six vertical bands of saturated colours, MCU-aligned, 384 x 256 pixels: several workgroups at one MCU per wave."""
    rgb = np.zeros((height, band * len(FIELDS), 3), np.uint8)
    for i, c in enumerate(FIELDS):
        rgb[:, i * band:(i + 1) * band] = c
    return encode(H, rgb, layout)


def golden_cases(H):
    """name -> JPEG bytes of every picture tests/golden/backend_reductions.json pins to the compiled reference."""
    out = {}
    for layout in LAYOUTS:
        for colour in COLOURS:
            out["flat_%s_%s" % (layout, colour)] = flat(H, layout, colour)
    for layout in ("420", "440"):
        out["raster_tie_%s" % layout] = raster_tie(H, layout)
    for layout in ("420", "gray"):
        out["wrap_%s_white" % layout] = flat(H, layout, "white", WRAP_SIZE)
    for layout in ("420", "444", "gray"):
        out["fields_%s" % layout] = fields(H, layout)
    return out


def stats_words(st):
    """The colour-statistics dict of harness.Backend.color_stats as the JSNOOP_STATS_WORDS record."""
    return np.concatenate([st["histo"].view(np.uint32), np.array([st["count"]], np.uint32), st["clip"], st["rgb"].ravel(), st["yfull"]])


def record(H, b, data):
    """What the JSON keeps of one picture decoded by backend b: bright_avg under the plain decode, then bright_avg and the colour statistics
    with bHistoEn, and with bStatClipEn alone."""
    r = {"sha256": H.hash_bytes(data)}
    try:
        b.set_options(decode_ac=1)
        H.drive(b, data)
        r["bright_avg"] = [int(v) for v in b.bright_avg()]
        for key, opt in (("histo", dict(histo_en=1)), ("clip", dict(stat_clip_en=1))):
            b.set_options(decode_ac=1, **opt)
            H.drive(b, data)
            r["bright_avg_" + key] = [int(v) for v in b.bright_avg()]
            r["stats_" + key] = H.hash_bytes(stats_words(b.color_stats()))
    finally:
        b.set_options(decode_ac=1)
    return r
