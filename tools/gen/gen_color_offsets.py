#!/usr/bin/env python3
"""Generates jpegsnoop_amd/csrc/jsnoop_color_exc.h: where the offset form of the 4:2:0 colour phase (k_idct_color, back_end_pairs<2, 2, .>)
needs a correction.

The offset form: a chroma sample (Cb, Cr) is run ONCE through ConvertYCCtoRGBFastFloat's fp32 chain at Y = 0, uncapped --

    Roff = floor(RN(RN(Cr * (2 - 2*0.299f)) + 128))      Boff = floor(RN(RN(Cb * (2 - 2*0.114f)) + 128))
    Goff = floor(RN(RN(RN(RN(0 - RN(0.114f * b)) - RN(0.299f * r)) / 0.587f) + 128))          with r, b the two chroma terms

-- and each of the pixels that share the sample is sat_u8(Y + off) per channel.  That is NOT the reference's arithmetic (which rounds
after adding Y), so it is proven here, not argued: all 2^24 clamped triples (Y, Cb, Cr) in [-128, 127]^3 go through the oracle's
orc_color_fast (the way tests/test_gpu_parity.py::test_color_sweep calls it) and are compared with the model.  R and B must agree
everywhere.  G may be ONE LOWER than the model on a set of triples that a few chroma pairs cover: those pairs, each with a 256-bit mask
over Y + 128, are the header.  Anything else (another channel, another delta, more than MAX_PAIRS pairs) is an error: the kernel's
exception path rests on that shape.

Usage: gen_color_offsets.py [out.h]        (default: the committed header)
       gen_color_offsets.py --check        (also asserts model + masks == oracle on all 2^24 triples; what the CPU test runs)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HDR = os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_color_exc.h")
MAX_PAIRS = 3            # the kernel tags a sample with its pair in two bits (0: none); each pair costs every chroma sample a compare

f32 = np.float32


def offsets():
    """(Roff[cr], Boff[cb], Goff[cb, cr]) as int32: the uncapped pipeline at Y = 0, every operation rounded to fp32 in the oracle's order."""
    kr, kg, kb = f32(0.299), f32(0.587), f32(0.114)
    c = np.arange(-128, 128, dtype=np.int32).astype(f32)
    crm = c * (f32(2) - f32(2) * kr)                             # r = cr * (2 - 2 kr) + 0
    cbm = c * (f32(2) - f32(2) * kb)
    assert crm.dtype == f32 and cbm.dtype == f32
    b, r = cbm[:, None], crm[None, :]
    g = ((f32(0) - kb * b) - kr * r) / kg                        # (y - kb b - kr r) / kg at y = 0
    assert g.dtype == f32
    fl = lambda v: np.floor(v + f32(128)).astype(np.int32)
    return fl(crm), fl(cbm), fl(g)


def oracle_lib():
    sys.path.insert(0, ROOT)
    try:
        from oracle import harness as H
    finally:
        sys.path.pop(0)
    H.build(["oracle"])
    return C.CDLL(H.ORC_SO)


def oracle_plane(lib, y, cb, cr):
    """orc_color_fast on one Y plane: (65536, 3) uint8 R, G, B, index cb * 256 + cr (both + 128)."""
    ycc = np.stack([np.full(cb.size, y * 8, np.int32), cb.ravel() * 8, cr.ravel() * 8], -1).copy()
    rgb = np.zeros((ycc.shape[0], 3), np.uint8)
    lib.orc_color_fast(ycc.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), C.c_size_t(ycc.shape[0]))
    return rgb


def model_plane(y, off, exc=None):
    """sat_u8(Y + off) per channel, (256, 256, 3) indexed [cb + 128, cr + 128]; exc: {(cb, cr): [8 words]} lowers G by one where the bit of Y + 128 is set."""
    roff, boff, goff = off
    m = np.empty((256, 256, 3), np.int32)
    m[..., 0] = y + roff[None, :]
    m[..., 1] = y + goff
    m[..., 2] = y + boff[:, None]
    for (cb, cr), words in (exc or {}).items():
        m[cb + 128, cr + 128, 1] -= (words[(y + 128) >> 5] >> ((y + 128) & 31)) & 1
    return np.clip(m, 0, 255).astype(np.uint8)


def sweep(lib, off, exc=None):
    """Differences between the model (with exc applied) and the oracle over all 2^24 triples: {(cb, cr): {y: (channel, oracle - model)}}."""
    cb, cr = np.meshgrid(np.arange(-128, 128, dtype=np.int32), np.arange(-128, 128, dtype=np.int32), indexing="ij")
    diffs = {}
    for y in range(-128, 128):
        want = oracle_plane(lib, y, cb, cr).reshape(256, 256, 3)
        got = model_plane(y, off, exc)
        for i, j, ch in zip(*np.nonzero(want != got)):
            diffs.setdefault((int(i) - 128, int(j) - 128), {})[y] = (int(ch), int(want[i, j, ch]) - int(got[i, j, ch]))
    return diffs


def exceptions(diffs):
    if len(diffs) > MAX_PAIRS:
        raise SystemExit("the model misses the oracle at %d chroma pairs (at most %d can be listed): %s ..." % (len(diffs), MAX_PAIRS, sorted(diffs)[:8]))
    exc = {}
    for pair, ys in sorted(diffs.items(), key=lambda kv: (abs(kv[0][0]), -kv[0][0])):
        words = [0] * 8
        for y, (ch, delta) in ys.items():
            if ch != 1 or delta != -1:
                raise SystemExit("pair %s, Y = %d: channel %d differs by %d -- only G one lower can be listed" % (pair, y, ch, delta))
            words[(y + 128) >> 5] |= 1 << ((y + 128) & 31)
        exc[pair] = words
    return exc


def header(exc):
    n = sum(bin(w).count("1") for ws in exc.values() for w in ws)
    o = ["// Generated by tools/gen/gen_color_offsets.py -- do not edit (tests/test_color_offsets_gen.py regenerates it byte for byte).",
         "// The offset form of the 4:2:0 colour phase, sat_u8(Y + off(Cb, Cr)) per channel, equals the reference's ConvertYCCtoRGBFastFloat on",
         "// every clamped triple (Y, Cb, Cr) in [-128, 127]^3 except %d: there G is ONE LOWER.  They lie in the %d chroma pairs below; bit" % (n, len(exc)),
         "// (Y + 128) & 31 of word (Y + 128) >> 5 of a pair's mask says so.  R and B have no exception.",
         "#pragma once",
         "#define JS_COLOR_EXC_PAIRS %d" % len(exc),
         "#define JS_COLOR_EXC_TRIPLES %d" % n,
         "// { Cb, Cr } after the clamp to [-128, 127]",
         "#define JS_COLOR_EXC_CBCR { %s }" % ", ".join("{ %d, %d }" % p for p in exc),
         "// per pair: 256 bits over Y + 128, word 0 first",
         "#define JS_COLOR_EXC_MASKS { \\"]
    for i, (p, ws) in enumerate(exc.items()):
        o.append("    { %s }%s    /* (%d, %d): %d values of Y */ \\" % (", ".join("0x%08Xu" % w for w in ws), "," if i + 1 < len(exc) else " ", p[0], p[1], sum(bin(w).count("1") for w in ws)))
    o.append("}")
    return "\n".join(o) + "\n"


def main(argv):
    check = "--check" in argv
    args = [a for a in argv if a != "--check"]
    lib, off = oracle_lib(), offsets()
    exc = exceptions(sweep(lib, off))
    if check:
        left = sweep(lib, off, exc)
        if left:
            raise SystemExit("model + masks still differ from the oracle at %s" % sorted(left)[:8])
        print("model + masks == oracle on all %d triples; %d exception triples in %d pairs" % (1 << 24, sum(bin(w).count("1") for ws in exc.values() for w in ws), len(exc)))
    with open(args[0] if args else HDR, "w") as f:
        f.write(header(exc))


if __name__ == "__main__":
    main(sys.argv[1:])
