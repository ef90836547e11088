"""The definition of jsnoop_batch_export_jpeg's file -- TEST INFRASTRUCTURE and the authority the kernels are compared with, byte for byte.

Input is what the library holds for one image after a decode: the coefficient arena [blocks][64] (int16, natural order, decode order: MCU after
MCU, the components interleaved inside the MCU), the cumulative DC of every block (dccum), the geometry (coef_model.Geometry plus the SOF
dimensions) and the multipliers of jsnoop_batch_image_dqt per component (natural order).  Output is (result, detail, file bytes or None).

Deliberately sequential: one block, one symbol, one bit group at a time through prog_codec's bit writer.  Nothing of the kernels' structure
(no lengths pass, no prefix sum, no separate stuffing pass).

Levels.  AC: level = arena[b][n] / q_c[n] with C division (truncating toward zero), n >= 1.  DC: d = (int16)(dccum[b] - dccum[p]), p the block of
the same component before b in decode order (dccum[p] = 0 for the component's first block), level = d / q_c[0]; slot 0 of the arena is not read.
Result.  OK 0; INEXACT 1: a value above leaves a remainder; UNCODABLE 2: |DC difference level| > 2047 or |AC level| > 1023; UNSUPPORTED 3: the SOF
precision is not 8.  The result of an image is the largest of its blocks'; detail is the lowest block index (counted inside the image, decode order)
whose own result is the image's.  A block that is uncodable is not also counted as inexact.  A non-OK image has no file."""
import numpy as np

import prog_codec as PC

OK, INEXACT, UNCODABLE, UNSUPPORTED = 0, 1, 2, 3

# ITU-T T.81 Annex K.3.3, Tables K.3 - K.6: (counts per code length 1..16, symbols in code order)
_AC_LUM = ("01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 A1 08 23 42 B1 C1 15 52 D1 F0 24 33 62 72 82 09 0A 16 17 18 19 1A 25 26 27 28 "
           "29 2A 34 35 36 37 38 39 3A 43 44 45 46 47 48 49 4A 53 54 55 56 57 58 59 5A 63 64 65 66 67 68 69 6A 73 74 75 76 77 78 79 7A 83 84 85 86 87 88 89 "
           "8A 92 93 94 95 96 97 98 99 9A A2 A3 A4 A5 A6 A7 A8 A9 AA B2 B3 B4 B5 B6 B7 B8 B9 BA C2 C3 C4 C5 C6 C7 C8 C9 CA D2 D3 D4 D5 D6 D7 D8 D9 DA E1 E2 "
           "E3 E4 E5 E6 E7 E8 E9 EA F1 F2 F3 F4 F5 F6 F7 F8 F9 FA")
_AC_CHR = ("00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 A1 B1 C1 09 23 33 52 F0 15 62 72 D1 0A 16 24 34 E1 25 F1 17 18 19 1A 26 "
           "27 28 29 2A 35 36 37 38 39 3A 43 44 45 46 47 48 49 4A 53 54 55 56 57 58 59 5A 63 64 65 66 67 68 69 6A 73 74 75 76 77 78 79 7A 82 83 84 85 86 87 "
           "88 89 8A 92 93 94 95 96 97 98 99 9A A2 A3 A4 A5 A6 A7 A8 A9 AA B2 B3 B4 B5 B6 B7 B8 B9 BA C2 C3 C4 C5 C6 C7 C8 C9 CA D2 D3 D4 D5 D6 D7 D8 D9 DA "
           "E2 E3 E4 E5 E6 E7 E8 E9 EA F2 F3 F4 F5 F6 F7 F8 F9 FA")
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [int(x, 16) for x in _AC_LUM.split()])
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [int(x, 16) for x in _AC_CHR.split()])
ANNEX_K = [DC_LUM, AC_LUM, DC_CHR, AC_CHR]          # slots: 2 * table id + class


def _tdiv(a, b):
    """C division of Python ints: (quotient truncated toward zero, remainder with the sign of a).  A multiplier of 0 divides nothing: level 0, the value left over."""
    if b == 0:
        return 0, a
    q = abs(a) // b
    q = -q if a < 0 else q
    return q, a - q * b


def _i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


_POS = [0] * 64                                       # zig-zag position of a natural index
for _z, _n in enumerate(PC.ZIGZAG):
    _POS[_n] = _z


def levels(arena, dccum, geo, qnat):
    """-> (lev [blocks][64] int64 in ZIG-ZAG order with the DC difference level at 0, result, detail).  qnat[c] = 64 multipliers, natural order."""
    arena = np.asarray(arena); dccum = np.asarray(dccum)
    assert arena.shape == (geo.nblocks, 64) and dccum.shape == (geo.nblocks,), (arena.shape, dccum.shape, geo.nblocks)
    comp = geo.comp_of_block()
    lev = np.zeros((geo.nblocks, 64), np.int64); status = np.zeros(geo.nblocks, np.int64)
    last = [0] * geo.ncomp
    for b in range(geo.nblocks):
        c = int(comp[b]); q = qnat[c]; inexact = uncodable = False
        d = _i16(int(dccum[b]) - last[c]); last[c] = int(dccum[b])
        lv, rem = _tdiv(d, int(q[0]))
        lev[b, 0] = lv; inexact |= rem != 0; uncodable |= abs(lv) > 2047
        for n in np.flatnonzero(arena[b]):             # (a zero value has level 0 and no remainder under every multiplier)
            n = int(n)
            if n == 0:
                continue                               # slot 0 is not read
            lv, rem = _tdiv(int(arena[b, n]), int(q[n]))
            lev[b, _POS[n]] = lv; inexact |= rem != 0; uncodable |= abs(lv) > 1023
        status[b] = UNCODABLE if uncodable else (INEXACT if inexact else OK)
    result = int(status.max()) if geo.nblocks else OK
    detail = int(np.flatnonzero(status == result)[0]) if result else 0
    return lev, result, detail


def tokens(lev, geo):
    """Annex F symbols of every block in decode order, in prog_codec's token form: (0, slot, symbol) | (1, value bits, count).
    Slot = 2 * table id + class, table id 0 for the first component and 1 for the others."""
    comp = geo.comp_of_block(); T = []
    for b in range(lev.shape[0]):
        t = 0 if comp[b] == 0 else 1; blk = lev[b]
        d = int(blk[0]); n = abs(d).bit_length()
        T.append((0, 2 * t, n))
        if n:
            T.append((1, d if d >= 0 else d - 1, n))
        last = 0
        for z in np.flatnonzero(blk[1:]):
            z = int(z) + 1; r = z - last - 1; last = z
            while r > 15:
                T.append((0, 2 * t + 1, 0xF0)); r -= 16
            v = int(blk[z]); n = abs(v).bit_length()
            T.append((0, 2 * t + 1, (r << 4) | n)); T.append((1, v if v >= 0 else v - 1, n))
        if last != 63:
            T.append((0, 2 * t + 1, 0))
    return T


def unstuffed(T, tables):
    """(bytes before stuffing with the final padding of ones, number of bits before the padding)."""
    codes = [PC._codes(t) for t in tables]
    out = bytearray(); acc = 0; have = 0; n = 0
    for kind, a, b in T:
        v, k = codes[a][b] if kind == 0 else (a & ((1 << b) - 1), b)
        acc = (acc << k) | v; have += k; n += k
        while have >= 8:
            out.append((acc >> (have - 8)) & 255); have -= 8
        acc &= (1 << have) - 1
    if have:
        out.append(((acc << (8 - have)) | ((1 << (8 - have)) - 1)) & 255)
    return bytes(out), n


def block_ends(T, tables):
    """Bit position behind every block (a block begins with the one token of a DC slot)."""
    codes = [PC._codes(t) for t in tables]
    ends = []; n = 0
    for kind, a, b in T:
        if kind == 0 and a % 2 == 0 and n:
            ends.append(n)
        n += codes[a][b][1] if kind == 0 else b
    ends.append(n)
    return ends


def entropy_bytes(T, tables):
    """The entropy-coded segment: MSB first, padded with ones, every FF followed by 00 (also a padded last byte)."""
    return PC._emit(T, tables)


def header(geo, dim_x, dim_y, qnat, jfif=True):
    out = bytearray(b"\xFF\xD8")
    if jfif:
        out += PC._seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    big = []
    for c in range(geo.ncomp):
        qz = [int(qnat[c][PC.ZIGZAG[z]]) for z in range(64)]
        big.append(max(qz) > 255)
        out += PC._seg(0xDB, bytes([(16 if big[c] else 0) | c]) + (b"".join(x.to_bytes(2, "big") for x in qz) if big[c] else bytes(qz)))
    p = bytes([8]) + int(dim_y).to_bytes(2, "big") + int(dim_x).to_bytes(2, "big") + bytes([geo.ncomp])
    for c in range(geo.ncomp):
        h, v = geo.hv[c] if geo.ncomp > 1 else (1, 1)
        p += bytes([c + 1, h << 4 | v, c])
    out += PC._seg(0xC1 if any(big) else 0xC0, p)
    for t in range(1 if geo.ncomp == 1 else 2):
        out += PC._dht(0, t, ANNEX_K[2 * t]) + PC._dht(1, t, ANNEX_K[2 * t + 1])
    p = bytes([geo.ncomp])
    for c in range(geo.ncomp):
        t = 0 if c == 0 else 1
        p += bytes([c + 1, t << 4 | t])
    return bytes(out + PC._seg(0xDA, p + bytes([0, 63, 0])))


def export_file(arena, dccum, geo, dim_x, dim_y, qnat, jfif=True, precision=8):
    """-> (result, detail, file bytes or None)."""
    if precision != 8:
        return UNSUPPORTED, 0, None
    lev, result, detail = levels(arena, dccum, geo, qnat)
    if result:
        return result, detail, None
    return OK, 0, header(geo, dim_x, dim_y, qnat, jfif) + entropy_bytes(tokens(lev, geo), ANNEX_K) + b"\xFF\xD9"


def frame_inputs(frame, coefs):
    """What the library holds after decoding a clean file of prog_codec's `frame` / `coefs`: (arena, dccum, geometry, qnat)."""
    import coef_model as M
    geo = M.Geometry(frame.hv, frame.mcu_x, frame.mcu_y)
    arena = PC.arena(frame, coefs, clear_dc=True)
    qnat = []
    for c in range(frame.ncomp):
        qz = frame.qtabs[frame.comps[c][2]]; qn = [0] * 64
        for z in range(64):
            qn[PC.ZIGZAG[z]] = qz[z]
        qnat.append(qn)
    dccum = np.zeros(geo.nblocks, np.int16)
    for c in range(frame.ncomp):
        idx = geo.arena_index(c)
        dccum[idx] = ((coefs[c][..., 0].astype(np.int64) * qnat[c][0]) & 0xFFFF).astype(np.uint16).view(np.int16)
    return arena, dccum, geo, qnat
