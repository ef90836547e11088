"""Sources and helpers the transform tests share (CPU: test_transform_model.py; GPU: test_gpu_transform.py) -- TEST INFRASTRUCTURE.

A source is what the library holds for one decoded image: (arena, dccum, geo, dim_x, dim_y, qnat).  `noise` makes one of coefficient noise under
tables that are NOT symmetric (a table left un-transposed shows) with every cell occupied; `planes` is the float64 orthonormal IDCT of every block
of one component, dequantised values in, samples out (no level shift, no rounding: the transform is linear and is held to 1e-6)."""
import numpy as np

import coef_model as CM
import prog_codec as PC

LAYOUTS = {"grey": [(1, 1)], "4:4:4": [(1, 1)] * 3, "4:2:2": [(2, 1), (1, 1), (1, 1)], "4:4:0": [(1, 2), (1, 1), (1, 1)], "4:2:0": [(2, 2), (1, 1), (1, 1)],
           "4:1:1": [(4, 1), (1, 1), (1, 1)]}
SIZES = [(8, 8), (17, 9), (33, 31), (48, 32), (50, 70)]
CROPS = [None, (0, 0, 16, 16), (16, 16, 16, 8), (5, 3, 20, 11), (9, 17, 1000, 1000), (32, 0, 7, 9)]   # on and off the MCU grid; reaching the edge and not


def table(c):
    """64 multipliers, natural order, not symmetric under transposition, 1..7."""
    return [1 + (3 * (n & 7) + 5 * (n >> 3) + c) % 7 for n in range(64)]


def noise(layout, w, h, seed, levels=40):
    hv = LAYOUTS[layout]; hmax = max(a for a, _ in hv); vmax = max(b for _, b in hv)
    geo = CM.Geometry(hv, -(-w // (8 * hmax)), -(-h // (8 * vmax)))
    rng = np.random.default_rng(seed)
    qnat = [table(c) for c in range(geo.ncomp)]
    comp = geo.comp_of_block()
    lev = rng.integers(1, levels + 1, (geo.nblocks, 64)) * rng.choice([-1, 1], (geo.nblocks, 64))          # never 0: every cell is occupied
    q = np.array(qnat)[comp]
    arena = (lev * q).astype(np.int16)
    dccum = (rng.integers(-levels, levels + 1, geo.nblocks) * q[:, 0]).astype(np.int16)
    return arena, dccum, geo, w, h, qnat


_K = np.arange(8)
_C = np.sqrt(np.where(_K == 0, 1.0, 2.0) / 8.0)[:, None] * np.cos((2 * _K[None, :] + 1) * _K[:, None] * np.pi / 16.0)      # C[k][n], orthonormal


def planes(arena, dccum, geo, c):
    """Component c -> float64 [bh * 8][bw * 8]: x = C^T F C per block, F[v][u] the arena row with the cumulative DC in cell 0."""
    at = geo.arena_index(c); bh, bw = at.shape
    F = arena[at].astype(np.float64).reshape(bh, bw, 8, 8); F[..., 0, 0] = dccum[at]
    X = np.einsum("vy,abvu,ux->abyx", _C, F, _C)
    return X.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def numpy_op(P, op):
    """What the op does to a plane of samples, in numpy's own words (jpegtran's meaning: ROT_90 is clockwise)."""
    import transform_model as M
    return {M.NONE: lambda: P, M.FLIP_H: lambda: P[:, ::-1], M.FLIP_V: lambda: P[::-1], M.ROT_180: lambda: np.rot90(P, 2), M.TRANSPOSE: lambda: P.T,
            M.ROT_90: lambda: np.rot90(P, -1), M.ROT_270: lambda: np.rot90(P, 1), M.TRANSVERSE: lambda: np.rot90(P, 2).T}[op]()


def levels_of(arena, dccum, geo, qnat):
    """Per component [bh][bw][64] in ZIG-ZAG order: the levels a decoder of the exported file holds (prog_codec.decode's form), DC from dccum."""
    out = []
    for c in range(geo.ncomp):
        at = geo.arena_index(c); q = np.array(qnat[c], np.int64)
        v = arena[at].astype(np.int64); v[..., 0] = dccum[at]
        assert not (v % q).any()
        out.append((v // q)[..., np.array(PC.ZIGZAG)].astype(np.int16))
    return out


def jpeg_file(layout, w, h, seed, shift=0, script=None):
    """A w x h file of `layout` whose every coefficient (padding blocks included) is noise, under the tables table(c + shift): baseline, or progressive
    along `script` (prog_codec's scan tuples).  -> (bytes, prog_codec.Frame)."""
    hv = LAYOUTS[layout]
    qtabs = {c: [table(c + shift)[PC.ZIGZAG[z]] for z in range(64)] for c in range(len(hv))}
    frame = PC.Frame(w, h, [(a, b, c) for c, (a, b) in enumerate(hv)], qtabs)
    rng = np.random.default_rng(seed)
    coefs = []
    for c in range(frame.ncomp):
        by, bx = frame.grid(c)
        lev = rng.integers(1, 16, (by, bx, 64)) * rng.choice([-1, 1], (by, bx, 64))
        lev[..., 0] = rng.integers(-60, 61, (by, bx))
        coefs.append(lev.astype(np.int16))
    data = PC.encode_baseline(frame, coefs) if script is None else PC.encode_progressive(frame, coefs, script)
    return data, frame


def geometry(frame):
    return CM.Geometry(frame.hv, frame.mcu_x, frame.mcu_y)
