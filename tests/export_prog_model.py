"""The definition of the progressive export (jsnoop_batch_export_jpeg_prog) -- TEST INFRASTRUCTURE and the authority the kernels are compared with, byte
for byte.  Sequential, built from export_model / export_rst_model / prog_codec, never from the kernels.

Inputs are export_rst_model.export_file's (arena, dccum, geometry, SOF dimensions, multipliers) plus a script and a restart spec.
A script is a list of scans (components, Ss, Se, Ah, Al), components ascending indices; validate() holds the rules, DEFAULT the built-in scripts.

Geometry (T.81 A.2.3).  A scan of more than one component walks the MCU-padded grid in decode order (arena order; a unit is an MCU of the scan's components).
A scan of one component walks the coded(c) part of the component's grid in raster order, one block a unit (for a one-component image that is the arena).
Levels.  DC: v[b] = (int16)dccum[b] / q_c[0], C division; a remainder, or a multiplier of 0 under a value, is INEXACT.  DC first scan: s = v >> Al
(arithmetic), coded as s[b] - s[p], p the previous block of the component in the scan's order inside the restart interval (0 where none); beyond +-2047:
UNCODABLE.  DC refinement: the bit (v >> Al) & 1.  AC first scan over Ss..Se (zig-zag): export_model's levels (arena / q; remainder INEXACT, beyond
+-1023 UNCODABLE), run/size symbols, ZRL.  End-of-band runs: a block whose band ends in zeros, or is all zeros, joins the pending run; the run is
flushed before the first symbol of the next block that has one, when it reaches 32767, at an interval end and at the scan end, as symbol n << 4 with
n = floor(log2(run)) and n extra bits.  Result word and detail: export_model's rule over the blocks and bands the script codes, detail the lowest
block in the image's decode order.
Tables: prog_codec.optimal_table of the scan's counts: a DC first scan one per scan component (class 0, id = position), an AC scan one (class 1, id 0).
Restart: NONE; MCUS n: Ri = n in every scan, in the scan's units; ROWS r: Ri = r x units per row (mcu_x, or coded(c)'s width); SOURCE: the recorded
interval as MCUS.  An Ri above 65535 in any scan: UNSUPPORTED.
File: SOI, APP0, DQTs, FF C2 with export_model's SOF fields; per scan its DHTs, DRI where Ri differs from the one in force, SOS, data; EOI."""
import numpy as np

import export_model as EM
import export_rst_model as RM
import prog_codec as PC

OK, INEXACT, UNCODABLE, UNSUPPORTED = EM.OK, EM.INEXACT, EM.UNCODABLE, EM.UNSUPPORTED
NONE, MCUS, ROWS, SOURCE = RM.NONE, RM.MCUS, RM.ROWS, RM.SOURCE
MAX_SCANS = 256
MAX_BLOCKS = 1 << 26
DEFAULT = {3: [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((0,), 6, 63, 0, 0), ((0, 1, 2), 0, 0, 1, 0)],
           1: [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 0), ((0,), 6, 63, 0, 0), ((0,), 0, 0, 1, 0)]}


def validate(script):
    """The rules of a script; returns the component count (1 or 3) it writes, raises ValueError naming the rule."""
    if not 1 <= len(script) <= MAX_SCANS:
        raise ValueError("1 .. %d scans" % MAX_SCANS)
    for i, (comps, ss, se, ah, al) in enumerate(script):
        comps = list(comps)
        if not comps or comps != sorted(set(comps)) or comps[0] < 0 or comps[-1] > 2:
            raise ValueError("scan %d: components" % i)
        if not ss <= se <= 63:
            raise ValueError("scan %d: Ss <= Se <= 63" % i)
        if not 0 <= al <= 13:
            raise ValueError("scan %d: Al <= 13" % i)
        if ss == 0 and se != 0:
            raise ValueError("scan %d: a DC scan has Ss = Se = 0" % i)
        if ss and (len(comps) != 1 or ah or al):
            raise ValueError("scan %d: an AC scan names one component and has Ah = Al = 0" % i)
        if ss == 0 and ah and al != ah - 1:
            raise ValueError("scan %d: a DC refinement has Al = Ah - 1" % i)
    named = sorted({c for s in script for c in s[0]})
    if named not in ([0], [0, 1, 2]):
        raise ValueError("the script names components %r" % (named,))
    al_of = {}; seen = {c: set() for c in named}
    for i, (comps, ss, se, ah, al) in enumerate(script):
        for c in comps:
            if ss == 0:
                if (ah != 0) if c not in al_of else (al_of[c] == 0 or ah != al_of[c]):
                    raise ValueError("scan %d: component %d's DC progression" % (i, c))
                al_of[c] = al
            else:
                if c not in al_of:
                    raise ValueError("scan %d: AC in front of the first DC scan" % i)
                band = set(range(ss, se + 1))
                if seen[c] & band:
                    raise ValueError("scan %d: a band coded twice" % i)
                seen[c] |= band
    for c in named:
        if al_of.get(c) != 0:
            raise ValueError("component %d's DC does not end at Al 0" % c)
        if seen[c] != set(range(1, 64)):
            raise ValueError("component %d's AC indices are not all coded" % c)
    return len(named)


def coded(geo, dim_x, dim_y, c):
    """(nby, nbx) of the part of component c's grid a one-component scan codes."""
    h, v = geo.hv[c]
    return -(-(-(-dim_y * v // geo.vmax)) // 8), -(-(-(-dim_x * h // geo.hmax)) // 8)


def scan_units(geo, dim_x, dim_y, comps):
    """-> (units, units per row): a unit is a list of (slot, component, arena block)."""
    comps = list(comps)
    if len(comps) > 1:
        first = [sum(a * b for a, b in geo.hv[:c]) for c in range(geo.ncomp)]
        units = []
        for m in range(geo.mcu_x * geo.mcu_y):
            units.append([(slot, c, m * geo.bpm + first[c] + k) for slot, c in enumerate(comps) for k in range(geo.hv[c][0] * geo.hv[c][1])])
        return units, geo.mcu_x
    c = comps[0]; nby, nbx = coded(geo, dim_x, dim_y, c); idx = geo.arena_index(c)
    return [[(0, c, int(idx[by, bx]))] for by in range(nby) for bx in range(nbx)], nbx


def scan_ri(mode, interval, per_row, source_ri=0):
    return {NONE: 0, MCUS: interval, ROWS: interval * per_row, SOURCE: source_ri}[mode]


def all_levels(arena, dccum, geo, qnat):
    """-> (dcv [blocks], dc inexact [blocks], AC levels [blocks][64] zig-zag, AC inexact, AC uncodable), every block of the arena."""
    arena = np.asarray(arena).astype(np.int64); comp = geo.comp_of_block()
    Q = np.asarray(qnat, np.int64)[comp]                                         # [blocks][64], natural order
    mag = np.where(Q > 0, np.abs(arena) // np.maximum(Q, 1), 0); lev = np.where(arena < 0, -mag, mag); rem = arena - lev * Q
    zz = np.array(PC.ZIGZAG)
    levz = lev[:, zz]; ixz = (rem != 0)[:, zz]; ucz = np.abs(levz) > 1023
    d = np.asarray(dccum).astype(np.int16).astype(np.int64); q0 = Q[:, 0]
    dmag = np.where(q0 > 0, np.abs(d) // np.maximum(q0, 1), 0); dcv = np.where(d < 0, -dmag, dmag)
    return dcv, (d - dcv * q0) != 0, levz, ixz, ucz


def _shift(v, al, arithmetic=True):
    return (v >> al) if arithmetic else (-((-v) >> al) if v < 0 else v >> al)


def scan_tokens(units, scan, ri, L, status, arithmetic=True):
    """The tokens of one scan in prog_codec's form (slots: a DC scan's components by position, an AC scan 0), sequentially; status[b] is raised to
    what the scan finds wrong with block b."""
    _comps, ss, se, ah, al = scan
    dcv, dcix, levz, ixz, ucz = L
    T = []; pred = {}; run = 0; nrst = 0

    def flush():
        nonlocal run
        if run:
            n = run.bit_length() - 1
            T.append((0, 0, n << 4))
            if n:
                T.append((1, run - (1 << n), n))
            run = 0

    for u, blocks in enumerate(units):
        if ri and u and u % ri == 0:
            flush(); T.append((2, nrst & 7, 0)); nrst += 1; pred = {}
        for slot, c, b in blocks:
            if ss == 0:
                bad = INEXACT if dcix[b] else OK
                s = _shift(int(dcv[b]), al, arithmetic)
                if ah:
                    T.append((1, s & 1, 1))
                else:
                    d = s - pred.get(slot, 0); pred[slot] = s
                    n = abs(d).bit_length()
                    if abs(d) > 2047:
                        bad = UNCODABLE; n = min(n, 15)
                    T.append((0, slot, n))
                    if n:
                        T.append((1, d if d >= 0 else d - 1, n))
                status[b] = max(status[b], bad)
                continue
            band = levz[b, ss:se + 1]
            status[b] = max(status[b], UNCODABLE if ucz[b, ss:se + 1].any() else (INEXACT if ixz[b, ss:se + 1].any() else OK))
            nz = np.flatnonzero(band)
            if len(nz) == 0:
                run += 1
                if run == 32767:
                    flush()
                continue
            flush()
            last = -1
            for i in nz:
                i = int(i); r = i - last - 1; last = i
                while r > 15:
                    T.append((0, 0, 0xF0)); r -= 16
                v = int(band[i]); n = min(abs(v).bit_length(), 15)
                T.append((0, 0, (r << 4) | n)); T.append((1, v if v >= 0 else v - 1, n))
            if last != se - ss:
                run = 1
    flush()
    return T


def head(geo, dim_x, dim_y, qnat, jfif=True):
    """export_model's header up to its SOF, the marker FF C2."""
    h = bytearray(EM.header(geo, dim_x, dim_y, qnat, jfif))
    h = h[:h.index(b"\xFF\xC4")]
    sof = len(h) - (10 + 3 * geo.ncomp)
    assert h[sof] == 0xFF and h[sof + 1] in (0xC0, 0xC1)
    h[sof + 1] = 0xC2
    return bytes(h)


def export_parts(arena, dccum, geo, dim_x, dim_y, qnat, script, restart=(NONE, 0), source_ri=0, jfif=True, precision=8, arithmetic=True):
    """-> (result, detail, file bytes or None, scans or None): scans = one dict per scan with ri, intervals, dht (the DHT segments), ecs (the
    entropy-coded data), tables, freq, sos_offset."""
    script = [(tuple(c), ss, se, ah, al) for c, ss, se, ah, al in script]
    ncomp = validate(script)
    mode, interval = restart
    per = [scan_units(geo, dim_x, dim_y, s[0]) if ncomp == geo.ncomp else (None, 0) for s in script]
    ris = [scan_ri(mode, interval, row, source_ri) for _u, row in per]
    if precision != 8 or ncomp != geo.ncomp or geo.nblocks >= MAX_BLOCKS or any(r > 65535 for r in ris):
        return UNSUPPORTED, 0, None, None
    L = all_levels(arena, dccum, geo, qnat)
    status = np.zeros(geo.nblocks, np.int64)
    toks = [scan_tokens(units, s, ri, L, status, arithmetic) for s, (units, _row), ri in zip(script, per, ris)]
    result = int(status.max()) if geo.nblocks else OK
    if result:
        return result, int(np.flatnonzero(status == result)[0]), None, None
    out = bytearray(head(geo, dim_x, dim_y, qnat, jfif)); scans = []; in_force = 0
    for (comps, ss, se, ah, al), (units, _row), ri, T in zip(script, per, ris, toks):
        ns = len(comps)
        if ss == 0 and ah == 0:
            freq = PC._freq(T, ns); tabs = [PC.optimal_table(f) for f in freq]
            dht = b"".join(PC._dht(0, i, t) for i, t in enumerate(tabs))
        elif ss:
            freq = PC._freq(T, 1); tabs = [PC.optimal_table(freq[0])]
            dht = PC._dht(1, 0, tabs[0])
        else:
            freq = []; tabs = [None] * ns; dht = b""
        out += dht
        if ri != in_force:
            out += PC._seg(0xDD, int(ri).to_bytes(2, "big")); in_force = ri
        p = bytes([ns])
        for i, c in enumerate(comps):
            p += bytes([c + 1, (i << 4) if (ss == 0 and ah == 0) else 0])
        ecs = PC._emit(T, tabs)
        scans.append(dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, ri=ri, intervals=(-(-len(units) // ri) if ri else 1), dht=dht, ecs=ecs, tables=tabs, freq=freq,
                          sos_offset=len(out), tokens=T))
        out += PC._seg(0xDA, p + bytes([ss, se, ah << 4 | al])) + ecs
    return OK, 0, bytes(out + b"\xFF\xD9"), scans


def export_file(arena, dccum, geo, dim_x, dim_y, qnat, script, restart=(NONE, 0), source_ri=0, jfif=True, precision=8, optimal=False):
    """-> (result, detail, file bytes or None).  script None is mode OFF: export_rst_model's file (optimal: its Huffman mode, which a script ignores)."""
    if script is None:
        return RM.export_file(arena, dccum, geo, dim_x, dim_y, qnat, RM.effective_ri(restart[0], restart[1], geo.mcu_x, source_ri), optimal, jfif, precision)
    return export_parts(arena, dccum, geo, dim_x, dim_y, qnat, script, restart, source_ri, jfif, precision)[:3]
