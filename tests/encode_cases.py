"""Pictures and sizes the encoder tests share (CPU model tests and GPU tests): deterministic, small, and the same everywhere."""
import numpy as np

SIZES = [(1, 1), (8, 8), (17, 9), (9, 17), (33, 31), (50, 70), (130, 21), (64, 48)]          # (width, height)
QUALITIES = [1, 10, 24, 25, 50, 75, 85, 95, 100]
LAYOUTS = ["grey", "4:4:4", "4:2:2", "4:2:0"]
# a custom table pair, natural order: every value 1..255 occurs somewhere, luma and chroma differ
CUSTOM = ([1 + (37 * k) % 255 for k in range(64)], [255 - (53 * k) % 255 for k in range(64)])


def picture(width, height, seed, grey=False):
    """Noise over sinusoids, uint8 [H][W][3] (or [H][W])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = np.stack([128 + 100 * np.sin(xx / 7. + seed), 128 + 100 * np.cos(yy / 5.), 128 + 90 * np.sin((xx + yy) / 9.)], -1)
    rgb = np.clip(base + rng.normal(0, 20, (height, width, 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(rgb[..., 1]) if grey else rgb


def extremes(width=33, height=31):
    """name -> uint8 [H][W][3]: all 0, all 255, a one-pixel checkerboard of 0 / 255, saturated colour stripes of period 1 and 2."""
    yy, xx = np.mgrid[0:height, 0:width]
    out = {"zeros": np.zeros((height, width, 3), np.uint8), "ones": np.full((height, width, 3), 255, np.uint8)}
    out["checker"] = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    sat = np.array([[255, 0, 0], [0, 255, 255], [0, 0, 255], [255, 255, 0]], np.uint8)
    out["stripes1"] = sat[xx % 4]
    out["stripes2"] = sat[(yy // 2) % 4]
    return out
