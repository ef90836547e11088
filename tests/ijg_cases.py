"""The files tests/test_ijg_model.py and tests/test_gpu_pack_ijg.py render -- TEST INFRASTRUCTURE.  Pictures are seeded noise (every block holds every frequency)
or the extremes a quantiser clips hardest; files are Pillow's (libjpeg-turbo's) own, so its decode of them is the second opinion on every byte."""
import io

import numpy as np

import base_stream as BS
import prog_codec as P

MODES = ("grey", "444", "422", "420")
HV = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}
_SUB = {"444": 0, "422": 1, "420": 2}
SIZES = [(1, 1), (2, 2), (3, 3), (4, 5), (5, 4), (8, 8), (16, 16), (17, 9), (9, 17), (33, 31), (50, 70), (130, 21), (64, 48), (6, 40), (40, 6)]      # (width, height)
QUALITIES = (10, 50, 85, 100)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def extremes(w=24, h=20):
    """[(name, pixels)]: random 0 / 255 pixels, a one-pixel checkerboard, saturated stripes."""
    y, x = np.mgrid[0:h, 0:w]
    bits = np.random.default_rng(99).integers(0, 2, (h, w, 3), dtype=np.uint8) * 255
    board = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    stripes = np.stack([((x & 1) * 255), (((x >> 1) & 1) * 255), ((y & 1) * 255)], -1).astype(np.uint8)
    return [("bits", bits), ("board", board), ("stripes", stripes)]


def pillow_file(pixels, mode, quality, progressive=False, **kw):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(pixels[..., 0])) if mode == "grey" else Image.fromarray(pixels)
    buf = io.BytesIO()
    if mode != "grey":
        kw["subsampling"] = _SUB[mode]
    im.save(buf, "JPEG", quality=quality, progressive=progressive, **kw)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def wild_file(w=40, h=24, seed=5):
    """A 4:2:0 baseline file whose every coefficient is the largest level its code allows (AC +-1023, DC +-1023: differences of category 11) at quantiser 255:
    the dequantised int16 values wrap, the IDCT's sums wrap.  No decoder's pixels mean anything here; the render must still be the model's."""
    frame = P.Frame(w, h, [(2, 2, 0), (1, 1, 0), (1, 1, 0)], {0: [255] * 64})
    ac = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    tabs = {(0, 0): P.flat_table(list(range(12)), 4), (1, 0): P.flat_table(ac, 8)}
    n = frame.mcu_x * frame.mcu_y * 6
    sign = np.random.default_rng(seed).integers(0, 2, (n, 64)) * 2 - 1
    blocks = [[int(v) for v in row] for row in sign * 1023]
    return BS.write(frame, tabs, [(0, 0)] * 3, blocks).file
