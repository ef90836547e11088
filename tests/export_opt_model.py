"""The definition of jsnoop_batch_export_jpeg_coded's file with huffman = optimal -- TEST INFRASTRUCTURE and the authority the kernels are
compared with, byte for byte.  Built from export_model.levels / tokens and prog_codec.optimal_table / _dht / _emit.

Levels, result words, detail and UNSUPPORTED are export_model's, unchanged.  For an OK image freq[slot][symbol] is the number of times tokens() emits
that symbol in that slot (slot = 2 * table id + class; ZRL and EOB count); the table of a slot is prog_codec.optimal_table(freq[slot]): T.81 K.2 with
the reserved 257th symbol of frequency 1, on equal frequencies the largest symbol value first, Adjust_BITS of Figure K.3, the reserved code point
taken off the longest length, symbols sorted by (code size before the adjustment, symbol value).  The file is export_model's with the DHT segments
replaced by these tables (DC0, AC0, DC1, AC1; one segment each) and the entropy-coded segment written with them.

group_k2 is K.2 as k_export_huff runs it: no OTHERS chains but a group id per symbol; tests/test_export_opt_model.py proves the two equal."""
import numpy as np

import export_model as EM
import prog_codec as PC

OK, INEXACT, UNCODABLE, UNSUPPORTED = EM.OK, EM.INEXACT, EM.UNCODABLE, EM.UNSUPPORTED
MAX_BLOCKS = 1 << 26                                  # an image with this many blocks or more is UNSUPPORTED in this mode (uint32 counters: 63 a block)


def frequencies(T, nslots):
    """[slot] -> {symbol: count} of the tokens of export_model.tokens."""
    return PC._freq(T, nslots)


def tables(freq):
    return [PC.optimal_table(f) for f in freq]


def header(geo, dim_x, dim_y, qnat, tabs, jfif=True):
    """export_model.header with its DHT segments replaced by `tabs` (2 or 4 tables, by slot)."""
    h = EM.header(geo, dim_x, dim_y, qnat, jfif)
    first = h.index(b"\xFF\xC4"); sos = h.rindex(b"\xFF\xDA")
    assert h[first:sos] == b"".join(PC._dht(s & 1, s >> 1, EM.ANNEX_K[s]) for s in range(len(tabs)))
    return h[:first] + b"".join(PC._dht(s & 1, s >> 1, tabs[s]) for s in range(len(tabs))) + h[sos:]


def export_parts(arena, dccum, geo, dim_x, dim_y, qnat, jfif=True, precision=8):
    """-> (result, detail, file bytes or None, freq or None, tables or None)."""
    if precision != 8 or geo.nblocks >= MAX_BLOCKS:
        return UNSUPPORTED, 0, None, None, None
    lev, result, detail = EM.levels(arena, dccum, geo, qnat)
    if result:
        return result, detail, None, None, None
    T = EM.tokens(lev, geo)
    freq = frequencies(T, 2 if geo.ncomp == 1 else 4)
    tabs = tables(freq)
    return OK, 0, header(geo, dim_x, dim_y, qnat, tabs, jfif) + PC._emit(T, tabs) + b"\xFF\xD9", freq, tabs


def export_file(arena, dccum, geo, dim_x, dim_y, qnat, jfif=True, precision=8):
    """-> (result, detail, file bytes or None)."""
    return export_parts(arena, dccum, geo, dim_x, dim_y, qnat, jfif, precision)[:3]


# ----------------------------------------------------------------------------------------------------------- K.2 the kernel's way
def group_codesizes(freq, ties_largest_first=True, reserve=True):
    """Code sizes (before Adjust_BITS) of the symbols with a count, and of the reserved symbol 256: every symbol carries the id of its group (the head
    that keeps the group's frequency); a merge of c1 and c2 -- two minima over the key (frequency, 511 - symbol) of the live heads, as the kernel packs
    it into one word -- gives every symbol of either group one more bit and the id c1."""
    f = {int(s): int(n) for s, n in freq.items() if n > 0}
    if not f:
        f = {0: 1}
    if reserve:
        f[256] = 1
    syms = np.array(sorted(f), np.int64); cnt = np.array([f[int(s)] for s in syms], np.int64)
    if len(syms) == 1:
        return {int(syms[0]): 1}
    DEAD = np.int64(1) << 62
    key = cnt * 512 + ((511 - syms) if ties_largest_first else syms)
    size = np.zeros(len(syms), np.int64); group = syms.copy()
    for _ in range(len(syms) - 1):
        i1 = int(np.argmin(key)); k1 = key[i1]; key[i1] = DEAD
        i2 = int(np.argmin(key)); k2 = key[i2]; key[i2] = DEAD
        key[i1] = ((k1 >> 9) + (k2 >> 9)) * 512 + (k1 & 511)
        m = (group == syms[i1]) | (group == syms[i2])
        size[m] += 1; group[m] = syms[i1]
    return {int(s): int(n) for s, n in zip(syms, size)}


def group_k2(freq, ties_largest_first=True, reserve=True, adjust=True, order_by_final=False):
    """(counts[16], symbols) the kernel's way.  The keyword arguments are the four WRONG readings of the definition (each refused by a named case of
    tests/export_opt_cases.py): ties smallest symbol first, no reserved code point, Adjust_BITS skipped (lengths clamped to 16), symbols in the
    order of their final length (which differs from the code-size order once Adjust_BITS has moved symbols)."""
    size = group_codesizes(freq, ties_largest_first, reserve)
    bits = [0] * 300
    for n in size.values():
        bits[n] += 1
    i = max(k for k in range(300) if bits[k])
    if adjust:
        while i > 16:
            while bits[i] > 0:
                j = i - 2
                while bits[j] == 0:
                    j -= 1
                bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1
            i -= 1
    else:
        for k in range(17, 300):
            bits[16] += bits[k]; bits[k] = 0
        i = min(i, 16)
    if reserve:
        while bits[i] == 0:
            i -= 1
        bits[i] -= 1
    order = sorted((size[s], s) for s in size if s != 256)
    syms = [s for _n, s in order]
    if order_by_final:
        final = []
        for ln in range(1, 17):
            final += [ln] * bits[ln]
        # the k-th symbol of the code-size order has the k-th final length; a reading that sorts by (final length, symbol) differs where lengths tie anew
        syms = [s for _l, s in sorted(zip(final, syms))]
    return bits[1:17], syms
