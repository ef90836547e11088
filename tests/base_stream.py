"""A token-level writer of baseline (SOF0) files -- TEST INFRASTRUCTURE, the sibling of prog_codec.encode_baseline.

encode_baseline codes coefficient arrays with optimal tables and asserts away what a conforming encoder never writes.  `write`
takes the Huffman tables as they are handed in and, per block, either 64 coefficients (zig-zag order, absolute DC) or the block's
tokens themselves: [(DC category, difference), (AC symbol, value), ...].  The token form may hold DC categories 12..15, AC sizes
11..15, `run/0` symbols with run 1..14, ZRL anywhere, runs that carry the index past 63 and blocks that end without EOB.  A token
(BITS, (value, n)) writes n literal bits -- a code that matches nothing, value bits that are cut off: what no table can express.

Besides the file `write` returns a CENSUS: one record per Huffman symbol with the bit position of its code in the un-stuffed entropy
data (restart markers removed, the pad bits in front of them kept: the layout the parallel path cuts into sub-sequences), the
restart interval, the block (decode order), the coefficient index before the symbol (0: the DC symbol), the table ((class, id)), the
code length, the size (value bits) and the symbol.  The helpers below answer from it where a symbol lies relative to a
sub-sequence, whether two symbols share one first-level window of the decode tables, and how many second-level entries a table set
needs (the rule of js_build_parallel_luts, restated).
"""
from __future__ import annotations

from collections import namedtuple

import prog_codec as P

L1_BITS = 9            # JS_L1_BITS   (jpegsnoop_amd/csrc/jsnoop_types.h)
LUT2_MAX = 2048        # JS_LUT2_MAX

Rec = namedtuple("Rec", "pos iv blk k tab len size sym")
BITS = "bits"          # the symbol of a literal-bits token; its census record: tab None, len 0, size n


class Stream:
    """file: the JPEG; raw: the un-stuffed entropy data; census: [Rec]; bits: un-stuffed entropy data in bits (pad bits included); iv_ends: per restart interval the
    bit position behind its last data bit (before padding); coefs: per block the 64 intended coefficients (zig-zag, absolute DC) or
    None where the block's tokens are not what a conforming decoder reads; frame / tabs / comp_ids as handed in."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def value_bits(v, s):
    """The s bits that code value v (F.1.2.1.1)."""
    v = int(v)
    assert s and abs(v).bit_length() == s, (v, s)
    return v if v >= 0 else v + (1 << s) - 1


def tokens_of(vec, pred):
    """Coefficient vector (zig-zag, absolute DC) -> tokens; sizes up to 15 are written as they come."""
    d = int(vec[0]) - pred
    T = [(abs(d).bit_length(), d)]
    last = 0
    for k in range(1, 64):
        t = int(vec[k])
        if not t:
            continue
        r = k - last - 1; last = k
        while r > 15:
            T.append((0xF0, 0)); r -= 16
        T.append(((r << 4) | abs(t).bit_length(), t))
    if last != 63:
        T.append((0x00, 0))
    return T


def coefs_of(tokens, pred):
    """What a conforming decoder makes of a block's tokens, or None when the tokens are not conforming (run/0, overshoot, ...)."""
    out = [0] * 64
    if any(t[0] == BITS for t in tokens):
        return None
    s, d = tokens[0]
    if s > 11:
        return None
    out[0] = pred + (d if s else 0)
    k = 1
    for i, (sym, v) in enumerate(tokens[1:]):
        if k > 63:
            return None
        r, s = sym >> 4, sym & 15
        if s == 0:
            if r == 15:
                k += 16; continue
            if r:
                return None
            return out if i == len(tokens) - 2 else None
        k += r
        if k > 63:
            return None
        out[k] = int(v); k += 1
    return out if k == 64 else None


def write(frame, tabs, comp_ids, blocks, dri=0, rst_before=()):
    """frame: prog_codec.Frame; tabs: {(class, id): (counts, symbols)} (class 0 DC, 1 AC; ids 0..3); comp_ids: per component
    (DC id, AC id); blocks: one entry per block in decode order -- a sequence of 64 numbers (coefficients) or a list of tokens.
    rst_before: block indices (decode order) in front of which the interval is closed and the next RSTn written besides those the
    restart interval asks for -- a marker inside an MCU, or a second one on an MCU boundary that already has one."""
    bpm = frame.mcu_blocks(); units = frame.mcu_x * frame.mcu_y
    assert len(blocks) == units * len(bpm), (len(blocks), units, len(bpm))
    codes = {key: P._codes(t) for key, t in tabs.items()}
    census = []; coefs = []; iv_ends = []; body = bytearray(); raw = bytearray()
    w = P._Bits(); nb = 0; base = 0; iv = 0; pred = [0] * frame.ncomp; extra = frozenset(int(b) for b in rst_before)
    assert all(0 < b < len(blocks) for b in extra), "a marker lies between two blocks"

    def close_interval(marker):
        nonlocal w, nb, base, iv
        iv_ends.append(base + nb)
        w.flush(); body.extend(w.out); raw.extend(bytes(w.out).replace(b"\xFF\x00", b"\xFF"))
        if marker is not None:
            body.extend(bytes([0xFF, 0xD0 + (marker & 7)]))
        base += (nb + 7) // 8 * 8; w = P._Bits(); nb = 0; iv += 1

    for u in range(units):
        if dri and u and u % dri == 0:
            close_interval(iv); pred = [0] * frame.ncomp             # (RSTn counts the markers written: iv == u // dri - 1 without rst_before)
        for j, (c, _y, _x) in enumerate(bpm):
            blk = blocks[u * len(bpm) + j]; bi = u * len(bpm) + j
            if bi in extra:
                close_interval(iv); pred = [0] * frame.ncomp
            is_tokens = len(blk) != 64 or isinstance(blk[0], tuple)
            T = list(blk) if is_tokens else tokens_of(blk, pred[c])
            want = coefs_of(T, pred[c])
            coefs.append(want)
            pred[c] += int(T[0][1]) if T[0][0] and T[0][0] != BITS else 0
            k = 0
            for n, (sym, v) in enumerate(T):
                if sym == BITS:
                    census.append(Rec(base + nb, iv, bi, k, None, 0, int(v[1]), BITS))
                    w.put(int(v[0]), int(v[1])); nb += int(v[1])
                    continue
                key = (0 if n == 0 else 1, comp_ids[c][0 if n == 0 else 1])
                code, ln = codes[key][sym]
                size = sym & 15
                census.append(Rec(base + nb, iv, bi, k, key, ln, size, sym))
                w.put(code, ln); nb += ln
                if size:
                    w.put(value_bits(v, size), size); nb += size
                k = 1 if n == 0 else k + (16 if sym == 0xF0 else 64 if sym == 0 else (sym >> 4) + 1)
    close_interval(None)
    out = bytearray(P._head(frame, 0xC0, None))
    if dri:
        out += P._seg(0xDD, int(dri).to_bytes(2, "big"))
    for (cls, ident), t in sorted(tabs.items()):
        out += P._dht(cls, ident, t)
    p = bytes([frame.ncomp])
    for c in range(frame.ncomp):
        p += bytes([c + 1, comp_ids[c][0] << 4 | comp_ids[c][1]])
    out += P._seg(0xDA, p + bytes([0, 63, 0])) + body + b"\xFF\xD9"
    return Stream(file=bytes(out), raw=bytes(raw), census=census, bits=base, iv_ends=iv_ends, coefs=coefs, frame=frame, tabs=tabs, comp_ids=comp_ids,
                  dri=dri, rst_before=sorted(extra))


# ------------------------------------------------------------------------------------------------------- census helpers
def sub_bits(wl):
    """Bits of one sub-sequence under JsnoopTuning.sub_wl = wl (4: 64 B ... 8: 1 KiB)."""
    return 32 << wl


def subseq(rec, wl=4):
    """Index of the sub-sequence the symbol's code starts in."""
    return rec.pos // sub_bits(wl)


def n_subseq(stream, wl=4):
    return -(-stream.bits // sub_bits(wl))


def to_sub_end(rec, wl=4):
    """Bits from the start of the symbol to the end of its sub-sequence (1 = it starts on the last bit)."""
    return sub_bits(wl) - rec.pos % sub_bits(wl)


def pair_visible(census, i):
    """Symbol i and symbol i + 1 are AC symbols of one block and the whole CODE of i + 1 lies inside the L1_BITS window that starts
    at symbol i -- the condition under which the pair rows (lutp, lutw) may describe both (whether a walk may then take the pair
    is the kernels' business: the index, the end of the block)."""
    if i + 1 >= len(census):
        return False
    a, b = census[i], census[i + 1]
    if a.blk != b.blk or a.k == 0 or a.sym == 0 or a.len > L1_BITS:
        return False
    used = a.len + a.size
    return used < L1_BITS and b.len <= L1_BITS - used


def window(stream, pos, n):
    """n bits of the un-stuffed entropy data from bit position pos (zeros behind the end)."""
    v = int.from_bytes(stream.raw[pos >> 3:(pos >> 3) + 8].ljust(8, b"\0"), "big")
    return (v >> (64 - (pos & 7) - n)) & ((1 << n) - 1)


def code_at(stream, table, pos, maxlen):
    """(symbol, length) of the code of `table` that the bits at pos spell within maxlen bits, or None."""
    for sym, (code, ln) in P._codes(table).items():
        if ln <= maxlen and window(stream, pos, ln) == code:
            return sym, ln
    return None


def distinct_tables(tabs, comp_ids, ncomp):
    """The distinct (class, table) pairs among the slots a scan of ncomp components uses: slots of one class with identical code lists
    share a row (slot_row), a DC and an AC table never do."""
    seen = []
    for c in range(ncomp):
        for cls in (0, 1):
            t = tabs[(cls, comp_ids[c][cls])]
            key = (cls, tuple(t[0]), tuple(t[1]))
            if key not in seen:
                seen.append(key)
    return seen


def lut2_need(tabs, comp_ids, ncomp):
    """Second-level entries the table set needs: per distinct table and per distinct L1_BITS-bit prefix of its codes longer than
    L1_BITS bits, 2 ** (longest code under that prefix - L1_BITS).  The set fits the LUT form while this is <= LUT2_MAX."""
    need = 0
    for cls, counts, syms in distinct_tables(tabs, comp_ids, ncomp):
        longest = {}
        for code, ln in P._codes((list(counts), list(syms))).values():
            if ln > L1_BITS:
                pre = code >> (ln - L1_BITS)
                longest[pre] = max(longest.get(pre, 0), ln)
        need += sum(1 << (ln - L1_BITS) for ln in longest.values())
    return need


def l2_groups(table):
    """{extra index bits: number of second-level groups} of one table."""
    longest = {}
    for code, ln in P._codes(table).values():
        if ln > L1_BITS:
            pre = code >> (ln - L1_BITS)
            longest[pre] = max(longest.get(pre, 0), ln)
    out = {}
    for ln in longest.values():
        out[ln - L1_BITS] = out.get(ln - L1_BITS, 0) + 1
    return out
