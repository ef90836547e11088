"""The plain definition of the preview rendering (CalcChannelPreview, reference :4619-4821; SetPreviewMode :633, SetPreviewYccOffset :650),
in numpy on int64: what a DIB looks like under a preview state, from the three sample planes.

A state is (mode, shift_mcu_x, shift_mcu_y, shift_y, shift_cb, shift_cr).  A pixel (px, py) is shifted when

    (py // mcu_h) * across + px // mcu_w >= shift_mcu_y * across + shift_mcu_x,        across = MCU-rounded width // mcu_w

-- a LINEAR MCU index on both sides, so shift_mcu_x >= across spills into the next MCU row and an index at or past the number of MCUs
shifts nothing.  The shift is added to the raw samples (three fractional bits) before `>> 3` and the clamp to [-128, 127]; the RGB triple is
the oracle's ConvertYCCtoRGBFastFloat (orc_color_fast) of the shifted samples, ChannelExtract (:4832-4872) picks what a mode shows.  The
brightest pixel is searched on the UNSHIFTED Y (:4722-4730 run before :4735-4739), the average on the shifted, clamped one (:4751).

Shared by tests/test_gpu_parity.py, tests/test_preview_cases.py (where the model itself is pinned to the oracle) and tests/test_gpu_preview.py."""
import ctypes as C

import numpy as np

DEFAULT = (1, 0, 0, 0, 0, 0)
MODES = range(1, 9)                  # PREVIEW_RGB, YCC, R, G, B, Y, CB, CR


def planes_of(backend):
    """The three int64 planes of a backend's last decode, chroma as planes() hands it out (replicated), all zero for grey (:4709-4715)."""
    p = backend.planes()
    y = p[0].astype(np.int64)
    return [y] + [q.astype(np.int64) if q is not None else np.zeros_like(y) for q in p[1:]]


def shifted_mask(shape, mcu_w, mcu_h, smx, smy):
    H, W = shape
    across = W // mcu_w
    mi = (np.arange(H)[:, None] // mcu_h) * across + (np.arange(W)[None, :] // mcu_w)
    return mi >= smy * across + smx


def color_fast(oracle, ycc):
    """orc_color_fast on an (n, 3) array of raw samples: (n, 3) uint8 R, G, B."""
    ycc = np.ascontiguousarray(ycc, np.int32)
    rgb = np.zeros((ycc.shape[0], 3), np.uint8)
    oracle.lib.orc_color_fast(ycc.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), C.c_size_t(ycc.shape[0]))
    return rgb


def shifted_samples(planes, mcu_w, mcu_h, state):
    """(H, W, 3) int64: sample + shift where the MCU index rule says so."""
    _mode, smx, smy, sy, scb, scr = state
    py, pcb, pcr = [np.asarray(p).astype(np.int64) for p in planes]
    sel = shifted_mask(py.shape, mcu_w, mcu_h, smx, smy).astype(np.int64)
    return np.stack([py + sel * sy, pcb + sel * scb, pcr + sel * scr], -1)


def expect(oracle, planes, mcu_w, mcu_h, state=DEFAULT, with_sum=False):
    """The bottom-up BGRA DIB of the planes under the state; with_sum: (DIB, sum of the final Y mod 2^32)."""
    mode = state[0]
    ycc = shifted_samples(planes, mcu_w, mcu_h, state)
    H8, W8 = ycc.shape[:2]
    assert int(np.abs(ycc).max()) < 2 ** 31
    flat = ycc.reshape(-1, 3)
    rgb = color_fast(oracle, flat)
    fin = np.clip(flat >> 3, -128, 127) + 128
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    fy, fcb, fcr = fin[:, 0], fin[:, 1], fin[:, 2]
    R, G, B = {1: (r, g, b), 2: (fcr, fy, fcb), 3: (r, r, r), 4: (g, g, g), 5: (b, b, b), 6: (fy, fy, fy), 7: (fcb, fcb, fcb), 8: (fcr, fcr, fcr)}[mode]
    out = np.zeros((H8, W8, 4), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = B.reshape(H8, W8), G.reshape(H8, W8), R.reshape(H8, W8)
    dib = out[::-1].copy()
    return (dib, int(fy.sum()) % 2 ** 32) if with_sum else dib


def bright_avg(oracle, planes, mcu_w, mcu_h, sum_y):
    """The ten ints of bright_avg(): valid, the brightest pixel's Y, Cb, Cr (unshifted; the first maximum in raster order, strict > :4724), its
    R, G, B and MCU, and the average Y: the 32-bit sum over (H + 1) * (W + 1), as the oracle's calc_channel_preview divides."""
    py, pcb, pcr = [np.asarray(p).astype(np.int64) for p in planes]
    H8, W8 = py.shape
    k = int(np.argmax(py))                                        # (numpy's argmax returns the first maximum in raster order)
    y, x = divmod(k, W8)
    ycc = [int(py[y, x]), int(pcb[y, x]), int(pcr[y, x])]
    rgb = color_fast(oracle, np.array([ycc]))[0]
    return [1] + ycc + [int(v) for v in rgb] + [x // mcu_w, y // mcu_h, (sum_y % 2 ** 32) // ((H8 + 1) * (W8 + 1))]
