"""The definition of the export with restart intervals (jsnoop_batch_export_jpeg_rst) -- TEST INFRASTRUCTURE and the authority the kernels are
compared with, byte for byte.  Sequential, built from export_model / export_opt_model / prog_codec, never from the kernels.

Ri is the entry's restart interval in MCUs, nmcu = nblocks / blocks per MCU.  Ri = 0 is export_model.export_file / export_opt_model.export_file.
For Ri in 1 .. 65535 interval r holds MCUs [r Ri, min((r + 1) Ri, nmcu)) in decode order, NI = ceil(nmcu / Ri) of them.

DC.  The predecessor of every component is 0 at the start of every interval: for the first block of a component in an interval d = (int16)dccum[b],
otherwise d = (int16)(dccum[b] - dccum[p]) as in export_model.levels.  AC levels, result words and detail follow export_model's rules on these levels.
Bytes.  export_model's header with FF DD 00 04 Ri_hi Ri_lo directly in front of SOS (behind the last DHT; also when NI = 1); every interval coded
on its own (MSB first, padded with ones, 00 behind every FF); FF D0+(r & 7) between interval r and r + 1, never stuffed; EOI.  In prog_codec's terms:
_emit over the tokens with a (2, r & 7, 0) token at every boundary.  Optimal tables: prog_codec.optimal_table of the counts of those tokens.
An effective Ri above 65535 is UNSUPPORTED (host arithmetic)."""
import numpy as np

import export_model as EM
import export_opt_model as OM
import prog_codec as PC

OK, INEXACT, UNCODABLE, UNSUPPORTED = EM.OK, EM.INEXACT, EM.UNCODABLE, EM.UNSUPPORTED
NONE, MCUS, ROWS, SOURCE = 0, 1, 2, 3                 # JSNOOP_RESTART_*


def effective_ri(mode, interval, mcu_x, source_ri=0):
    """The Ri an entry is written with; above 65535: the entry is UNSUPPORTED."""
    return {NONE: 0, MCUS: interval, ROWS: interval * mcu_x, SOURCE: source_ri}[mode]


def intervals(geo, ri):
    nmcu = geo.nblocks // geo.bpm
    return -(-nmcu // ri) if ri else 1


def levels(arena, dccum, geo, qnat, ri):
    """export_model.levels with the predictors set to 0 at every interval start."""
    if not ri:
        return EM.levels(arena, dccum, geo, qnat)
    arena = np.asarray(arena); dccum = np.asarray(dccum)
    assert arena.shape == (geo.nblocks, 64) and dccum.shape == (geo.nblocks,)
    comp = geo.comp_of_block(); per = ri * geo.bpm
    lev = np.zeros((geo.nblocks, 64), np.int64); status = np.zeros(geo.nblocks, np.int64)
    last = [0] * geo.ncomp
    for b in range(geo.nblocks):
        if b % per == 0:
            last = [0] * geo.ncomp
        c = int(comp[b]); q = qnat[c]
        d = EM._i16(int(dccum[b]) - last[c]); last[c] = int(dccum[b])
        lv, rem = EM._tdiv(d, int(q[0]))
        lev[b, 0] = lv; inexact = rem != 0; uncodable = abs(lv) > 2047
        for n in np.flatnonzero(arena[b]):
            n = int(n)
            if n == 0:
                continue
            lv, rem = EM._tdiv(int(arena[b, n]), int(q[n]))
            lev[b, EM._POS[n]] = lv; inexact |= rem != 0; uncodable |= abs(lv) > 1023
        status[b] = UNCODABLE if uncodable else (INEXACT if inexact else OK)
    result = int(status.max()) if geo.nblocks else OK
    detail = int(np.flatnonzero(status == result)[0]) if result else 0
    return lev, result, detail


def tokens(lev, geo, ri):
    """export_model.tokens with a (2, r & 7, 0) token between interval r and r + 1."""
    if not ri:
        return EM.tokens(lev, geo)
    per = ri * geo.bpm; T = []; r = 0
    for b0 in range(0, geo.nblocks, per):
        if b0:
            T.append((2, r & 7, 0)); r += 1
        T += _tokens_from(lev, geo, b0, min(b0 + per, geo.nblocks))
    return T


def _tokens_from(lev, geo, b0, b1):
    comp = geo.comp_of_block()

    class Part:                                       # export_model.tokens reads comp_of_block and the rows it is handed, nothing else
        def comp_of_block(self):
            return comp[b0:b1]
    return EM.tokens(lev[b0:b1], Part())


def with_dri(header, ri):
    """The header with the DRI segment directly in front of SOS."""
    sos = header.rindex(b"\xFF\xDA")
    return header[:sos] + PC._seg(0xDD, int(ri).to_bytes(2, "big")) + header[sos:]


def export_parts(arena, dccum, geo, dim_x, dim_y, qnat, ri, optimal=False, jfif=True, precision=8):
    """-> (result, detail, file bytes or None, freq or None, tables or None)."""
    if not ri:
        if optimal:
            return OM.export_parts(arena, dccum, geo, dim_x, dim_y, qnat, jfif, precision)
        return EM.export_file(arena, dccum, geo, dim_x, dim_y, qnat, jfif, precision) + (None, None)
    if precision != 8 or ri > 65535 or (optimal and geo.nblocks >= OM.MAX_BLOCKS):
        return UNSUPPORTED, 0, None, None, None
    lev, result, detail = levels(arena, dccum, geo, qnat, ri)
    if result:
        return result, detail, None, None, None
    T = tokens(lev, geo, ri)
    if optimal:
        freq = OM.frequencies(T, 2 if geo.ncomp == 1 else 4); tabs = OM.tables(freq)
        head = OM.header(geo, dim_x, dim_y, qnat, tabs, jfif)
    else:
        freq = None; tabs = EM.ANNEX_K
        head = EM.header(geo, dim_x, dim_y, qnat, jfif)
    return OK, 0, with_dri(head, ri) + PC._emit(T, tabs) + b"\xFF\xD9", freq, (tabs if optimal else None)


def export_file(arena, dccum, geo, dim_x, dim_y, qnat, ri, optimal=False, jfif=True, precision=8):
    """-> (result, detail, file bytes or None)."""
    return export_parts(arena, dccum, geo, dim_x, dim_y, qnat, ri, optimal, jfif, precision)[:3]
