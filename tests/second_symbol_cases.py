"""The catalogue behind tests/test_second_symbol_cases.py (CPU) and tests/test_gpu_second_symbol.py (GPU): baseline files written symbol by
symbol (tests/base_stream.py) around the SECOND symbol of a write-pass step (k_write2, k_write_dc: DESIGN.md §4.1).

A step takes the symbol at the window and, when nothing out of the ordinary can happen on the way, the AC symbol behind it.  The pair
rows of the tables (lutw) show that second symbol only when its code lies inside the 9-bit window behind the first symbol's code AND value
bits; every other second symbol comes from a table read of its own, at the bits that follow the first symbol.  Each case here holds pairs
the pair rows cannot show (`hidden`: len1 + size1 + len2 > 9) in a named situation, and carries a `check` that proves it from the
writer's census.  The truth is the oracle's decode.
"""
from __future__ import annotations

import numpy as np

import base_cases as BC
import base_stream as BS
import prog_codec as P

STEP_BITS = 32         # JS_STEP_BITS (jsnoop_kernels.hip): what one step may consume -- the window of the cursor, one update of its shift

# One code of every length 1..9, then 16-bit codes.  Bits per symbol (code + value):
#   0x01: 2   EOB: 2   ZRL: 3   0x21: 5   0x05: 10   0x0A: 16   0x09: 16   0x19: 17   0x04: 13   0x0F: 31   0x51: 17   0x31: 17   0x0B: 27
AC_W = P.ladder_table([0x01, 0x00, 0xF0, 0x21, 0x05, 0x0A, 0x09, 0x19, 0x04, 0x0F, 0x51, 0x31, 0x0B], 1, 9)
BITS = {0x01: 2, 0x00: 2, 0xF0: 3, 0x21: 5, 0x05: 10, 0x0A: 16, 0x09: 16, 0x19: 17, 0x04: 13, 0x0F: 31, 0x51: 17, 0x31: 17, 0x0B: 27}
TABS = {(0, 0): BC.DC2, (1, 0): AC_W}
val, tok = BC.val, BC.tok


def adv(sym):
    return 64 if sym == 0 else 16 if sym == 0xF0 else (sym >> 4) + 1


def hidden(cs, i):
    """Symbols i and i + 1 are a pair a step may take (one block, the first neither EOB nor the block's last by its index) that the pair
    rows cannot show: the first is a DC symbol, or the code of the second leaves the 9-bit window."""
    if i + 1 >= len(cs):
        return False
    a, b = cs[i], cs[i + 1]
    if a.blk != b.blk or b.k >= 64 or (a.k and a.sym == 0):
        return False
    return a.k == 0 or a.len + a.size + b.len > BS.L1_BITS


def taken(cs, i):
    """... and the step takes it: both codes within the first level, all four fields within STEP_BITS, the index stays inside the block."""
    a, b = cs[i], cs[i + 1]
    return hidden(cs, i) and a.len <= BS.L1_BITS and b.len <= BS.L1_BITS and a.len + a.size + b.len + b.size <= STEP_BITS and b.k + adv(b.sym) - (63 if b.sym == 0 else 0) <= 64


def up_to(rng, k):
    """Tokens that carry the coefficient index from 1 to k."""
    t = []; cur = 1
    while k - cur >= 16:
        t.append((0xF0, 0)); cur += 16
    return t + tok(rng, *([0x01] * (k - cur)))


def filler(bits, rng):
    """Blocks over TABS (DC category 0) that take exactly `bits` bits: 4 + 2 n + 5 m each."""
    out = []
    assert bits == 0 or bits >= 4 and bits not in (5, 7), bits
    while bits:
        take = bits if bits <= 124 else 100
        m = take & 1
        n = (take - 4 - 5 * m) // 2
        assert 0 <= n and n + 3 * m <= 62, (bits, take)
        out.append([(0, 0)] + tok(rng, *([0x01] * n)) + tok(rng, *([0x21] * m)) + [(0x00, 0)])
        bits -= take
    return out


def block_bits(t):
    return 2 + t[0][0] + sum(BITS[s] for s, _ in t[1:])


def pairs_in(cs, first, second):
    return [i for i in range(len(cs) - 1) if cs[i].k > 0 and cs[i].sym == first and cs[i + 1].sym == second and cs[i].blk == cs[i + 1].blk]


CASES = []


def case(fn):
    CASES.append(fn)
    return fn


_COLOUR = False        # build_all(colour=True): the gray cases written as 4:4:4 pictures (the DC-only fast form takes three components only)


def one_row(blocks, name, check, dri=0, **kw):
    """A gray picture of the blocks in decode order, at most 16 blocks wide (padded with empty blocks to whole rows) -- or, re-framed, the
    same blocks with the same tables for all three components of a 4:4:4 picture: the bit stream, and so the place of every symbol, is the same."""
    blocks = list(blocks); per = 3 if _COLOUR else 1; w = min(16, -(-len(blocks) // per))
    while len(blocks) % (w * per):
        blocks.append([(0, 0), (0, 0)])
    if _COLOUR:
        assert dri == 0
        return BC.Case(name + "_444", BS.write(BC.color(w, len(blocks) // (3 * w), 1, 1, BC.QV, BC.QV), TABS, [(0, 0)] * 3, blocks), check, **kw)
    return BC.Case(name, BS.write(BC.gray(w, len(blocks) // w), TABS, [(0, 0)], blocks, dri), check, **kw)


@case
def second_is_eob_or_zrl():
    """Hidden pairs whose second symbol is EOB (ends the block inside the step) or ZRL (stores nothing, advances 16)."""
    rng = np.random.default_rng(901)
    blocks = []
    for rep in range(3):
        for first in (0x05, 0x04, 0x0A, 0x19):
            d = rep % 3
            blocks.append([(d, val(rng, d))] + tok(rng, *([0x01] * rep)) + tok(rng, first) + [(0x00, 0)])
            blocks.append([(d, val(rng, d))] + tok(rng, *([0x01] * rep)) + tok(rng, first, 0xF0, 0x01, first, 0xF0, 0xF0, 0x21) + [(0x00, 0)])
    def check(c):
        cs = c.stream.census
        for first in (0x05, 0x04, 0x0A, 0x19):
            for second in (0x00, 0xF0):
                hits = pairs_in(cs, first, second)
                assert len(hits) >= 3 and all(taken(cs, i) and not BS.pair_visible(cs, i) for i in hits), (hex(first), hex(second))
        assert all(x is not None for x in c.stream.coefs)
    return one_row(blocks, "second_is_eob_or_zrl", check)


@case
def second_reaches_index_64():
    """Hidden pairs whose second symbol ends the block at index 64 exactly, by its run (0x21 from 61, 0x19 from 62, ZRL from 48) or by
    its place (0x05 at 63); no EOB follows."""
    rng = np.random.default_rng(902)
    blocks = []
    for rep in range(3):
        for first, second in ((0x05, 0x21), (0x04, 0x19), (0x05, 0xF0), (0x0A, 0x05), (0x19, 0x05)):
            blocks.append([(rep, val(rng, rep))] + up_to(rng, 64 - adv(first) - adv(second)) + tok(rng, first, second))
    blocks.append([(0, 0), (0, 0)])
    def check(c):
        cs = c.stream.census
        n = [i for i in range(len(cs) - 1) if taken(cs, i) and cs[i].k and cs[i + 1].k + adv(cs[i + 1].sym) == 64]
        assert len(n) == 15 and {cs[i + 1].sym for i in n} == {0x21, 0x19, 0xF0, 0x05}
        assert all(x is not None for x in c.stream.coefs)
    return one_row(blocks, "second_reaches_index_64", check)


def _overshoot(where):
    name = "second_run_passes_index_64_%s" % where
    def build():
        rng = np.random.default_rng(903)
        fr = BC.color(2, 2); n = 4 * 6
        at = {"first_block_of_an_mcu": 6, "last_block_of_an_mcu": 11, "last_block_of_the_image": n - 1}[where]
        blocks = []
        for i in range(n):
            d = int(rng.integers(3))
            if i == at:                               # 0x05 leaves index 62; 0x21 (hidden behind its ten bits) asks for 65
                blocks.append([(d, val(rng, d))] + up_to(rng, 61) + tok(rng, 0x05, 0x21)); continue
            blocks.append([(d, val(rng, d))] + tok(rng, *[[0x01, 0x05, 0x21, 0x04][int(x)] for x in rng.integers(0, 4, int(rng.integers(0, 9)))]) + [(0, 0)])
        def check(c):
            cs = c.stream.census
            last = [r for r in cs if r.blk == at][-1]; i = cs.index(last)
            assert last.sym == 0x21 and last.k + adv(last.sym) == 65 and hidden(cs, i - 1) and not taken(cs, i - 1) and c.stream.coefs[at] is None
        tabs = {(0, 0): BC.DC2, (1, 0): AC_W, (0, 1): BC.DC2, (1, 1): AC_W}
        return BC.Case(name, BS.write(fr, tabs, [(0, 0), (1, 1), (1, 1)], blocks), check, group="overshoot")
    build.__name__ = name
    return build


for _w in ("first_block_of_an_mcu", "last_block_of_an_mcu", "last_block_of_the_image"):
    CASES.append(_overshoot(_w))


@case
def second_code_longer_than_the_first_level():
    """The symbol behind the first one has a 16-bit code: the step stays single (the second read finds an escape)."""
    rng = np.random.default_rng(904)
    blocks = []
    for rep in range(3):
        for first in (0x01, 0x05, 0x04, 0x0A, 0xF0):
            for second in (0x0F, 0x51, 0x0B):
                d = rep % 3
                blocks.append([(d, val(rng, d))] + tok(rng, *([0x01] * rep)) + tok(rng, first, second, 0x01, first) + [(0x00, 0)])
    def check(c):
        cs = c.stream.census
        n = [i for i in range(len(cs) - 1) if cs[i].k and cs[i].blk == cs[i + 1].blk and cs[i + 1].len == 16]
        assert len(n) >= 45 and not any(taken(cs, i) or BS.pair_visible(cs, i) for i in n)
        assert all(hidden(cs, i + 1) and not taken(cs, i + 1) for i in n), "and the long code as the first symbol: an escape takes nothing along"
    return one_row(blocks, "second_code_longer_than_the_first_level", check)


@case
def pair_of_exactly_the_step_bound_and_one_over():
    """Two symbols of 16 + 16 = 32 bits (taken: the whole window, one cursor update of 32) and of 16 + 17 / 17 + 16 = 33 (not taken),
    at every phase of the cursor's words."""
    rng = np.random.default_rng(905)
    blocks = []
    for rep in range(68):
        pre = tok(rng, *([0x01] * (rep % 17))) + tok(rng, *([0xF0] * (rep % 2))) + tok(rng, *([0x21] * (rep // 2 % 2)))      # 2, 3 and 5 bits: every phase modulo 32
        blocks.append([(0, 0)] + pre + tok(rng, 0x0A, 0x09, 0x09, 0x0A, 0x09, 0x19, 0x19, 0x0A, 0x0A, 0x0A, 0x19, 0x19) + [(0x00, 0)])
    def check(c):
        cs = c.stream.census
        tot = lambda i: cs[i].len + cs[i].size + cs[i + 1].len + cs[i + 1].size
        at = [i for i in range(len(cs) - 1) if hidden(cs, i) and cs[i].k and cs[i + 1].sym]
        assert {tot(i) for i in at if taken(cs, i)} >= {STEP_BITS} and {tot(i) for i in at if not taken(cs, i)} == {STEP_BITS + 1, STEP_BITS + 2}
        assert {cs[i].pos % 32 for i in at if tot(i) == STEP_BITS} == set(range(32)), "a pair of 32 bits at every phase"
        assert {cs[i].pos % 32 for i in at if tot(i) == STEP_BITS + 1} == set(range(32))
    return one_row(blocks, "pair_of_exactly_the_step_bound_and_one_over", check)


PLACES = BC.PLACES           # the ends of the sub-sequences of sub_wl 4..8 and their middles


def _sweep(first, second, d, seed):
    """The hidden pair (first, second), moved so that the SECOND symbol starts d bits behind each of PLACES (d = -bits of it: it ends on
    the last bit of a lane's range; one more: it crosses; -1 / 0 / +1: the first symbol ends the range or not)."""
    name = "sweep_hidden_pair_%02x_%02x_second_at_%+d" % (first, second, d)
    def build():
        rng = np.random.default_rng(seed)
        blocks = []; cur = 0
        for place in PLACES:
            lead = place + d - 2 - BITS[first] - cur
            blocks += filler(lead, rng)
            t = [(0, 0)] + tok(rng, first, second) + ([(0, 0)] if second else [])
            blocks.append(t); cur = place + d - BITS[first] - 2 + block_bits(t)
        blocks += filler(64, rng)
        def check(c):
            cs = c.stream.census
            hits = [i for i in pairs_in(cs, first, second) if hidden(cs, i) and cs[i + 1].pos - d in PLACES]
            assert [cs[i + 1].pos - d for i in hits] == list(PLACES)
            for wl in range(4, 9):
                assert any(cs[i + 1].pos - d == BS.sub_bits(wl) for i in hits) and any(cs[i + 1].pos - d == BS.sub_bits(wl) // 2 for i in hits)
        return one_row(blocks, name, check)
    build.__name__ = name
    return build


for _j, _d in enumerate((-BITS[0x21], -BITS[0x21] + 1, -1, 0, 1)):
    CASES.append(_sweep(0x05, 0x21, _d, 910 + _j))
for _j, _d in enumerate((-2, -1, 0, 1)):
    CASES.append(_sweep(0x04, 0x00, _d, 920 + _j))


def _cut_interval(name, second, keep_bits, seed):
    """Restart intervals whose last block ends with a hidden pair, then cut: the bytes in front of the marker are removed so that the
    interval's data ends `keep_bits` bits into the second symbol (inside its code, or inside its value bits)."""
    def build():
        rng = np.random.default_rng(seed)
        first = 0x05; blocks = []; cuts = []
        for iv in range(6):
            if iv % 2 == 0:
                blocks += [filler(20, rng)[0], filler(12, rng)[0]]; continue
            # the second symbol starts at a byte boundary less keep_bits % 8 ... so that whole bytes can be removed behind keep_bits of it
            tail = [(0, 0), (first, 16)] + tok(rng, second) + [(0x00, 0)]             # (value bits 10000: the last byte that stays is not FF)
            lead = (-(2 + BITS[first] + keep_bits)) % 8
            while lead < 4 or lead in (5, 7):
                lead += 8
            blocks += [filler(lead, rng)[0], tail]
            cuts.append((lead + 2 + BITS[first] + keep_bits) // 8)        # bytes of the interval that stay
        s = BS.write(BC.gray(4, len(blocks) // 4), TABS, [(0, 0)], blocks, dri=2)
        # remove the bytes between `stay` and the marker of every odd interval
        f = bytearray(s.file); sos = f.index(b"\xFF\xDA"); body = sos + 2 + int.from_bytes(f[sos + 2:sos + 4], "big")
        out = bytearray(f[:body]); p = body; iv = 0; start = body
        while p < len(f):
            if f[p] == 0xFF and f[p + 1] != 0:
                if iv % 2 == 1:
                    stay = cuts[iv // 2]
                    seg = bytes(f[start:p]); raw = seg.replace(b"\xFF\x00", b"\xFF")           # (the interval's bytes, un-stuffed)
                    assert stay < len(raw) and raw[stay - 1] != 0xFF, (raw.hex(), stay)
                    del out[len(out) - len(seg):]
                    out += raw[:stay].replace(b"\xFF", b"\xFF\x00")
                out += f[p:p + 2]; p += 2; iv += 1; start = p
                continue
            out.append(f[p]); p += 1
        s.file = bytes(out); s.cut_intervals = len(cuts)
        def check(c):
            cs = c.stream.census
            hits = [i for i in pairs_in(cs, first, second) if hidden(cs, i)]
            assert len(hits) == 3 == c.stream.cut_intervals and len(c.stream.file) < len(f)
            assert (keep_bits < cs[hits[0] + 1].len) == ("code_bits" in name) and keep_bits < cs[hits[0] + 1].len + cs[hits[0] + 1].size
        return BC.Case(name, s, check, group="cut_interval")
    build.__name__ = name
    return build


CASES.append(_cut_interval("pair_crosses_interval_end_in_code_bits", 0x04, 5, 930))
CASES.append(_cut_interval("pair_crosses_interval_end_in_value_bits", 0x04, 11, 931))
CASES.append(_cut_interval("pair_crosses_interval_end_in_the_value_bit_of_a_short_symbol", 0x21, 4, 932))


def _dc_first(name, h, v, seed):
    """Every block opens with its DC symbol and an AC symbol right behind it: at the first block of an MCU, behind a change of component
    (other rows of the tables), with an EOB as the second symbol (the block ends in the step that began with its DC symbol)."""
    def build():
        rng = np.random.default_rng(seed)
        fr = BC.color(3, 2, h, v); bpm = fr.mcu_blocks(); blocks = []
        dcy = P.ladder_table([0, 1, 2, 3, 4, 5, 6], 2, 7); dcc = P.flat_table([0, 1, 2, 3], 3)
        acc = P.ladder_table([0x00, 0x01, 0x21, 0x05, 0x04, 0xF0, 0x31], 1, 6)
        tabs = {(0, 0): dcy, (1, 0): AC_W, (0, 1): dcc, (1, 1): acc}
        seconds = [0x00, 0x01, 0x05, 0x04, 0xF0, 0x21]
        for u in range(fr.mcu_x * fr.mcu_y):
            for j, (c, _y, _x) in enumerate(bpm):
                d = int(rng.integers(7 if c == 0 else 4)); s2 = seconds[(u + j) % len(seconds)]
                t = [(d, val(rng, d))] + tok(rng, s2)
                if s2:
                    t += tok(rng, *[[0x01, 0x05, 0x21][int(x)] for x in rng.integers(0, 3, int(rng.integers(0, 5)))]) + [(0, 0)]
                blocks.append(t)
        def check(c):
            cs = c.stream.census; nb = len(bpm)
            dc = [i for i, r in enumerate(cs) if r.k == 0]
            assert all(hidden(cs, i) and taken(cs, i) for i in dc)
            for j in (0, nb - 2, nb - 1):             # first block of an MCU; first Cb block (behind Y); Cr
                assert {cs[i + 1].sym for i in dc if cs[i].blk % nb == j} >= {0x00, 0x01, 0x05}, j
        return BC.Case(name, BS.write(fr, tabs, [(0, 0), (1, 1), (1, 1)], blocks), check)
    build.__name__ = name
    return build


CASES.append(_dc_first("dc_first_ac_second_420", 2, 2, 940))
CASES.append(_dc_first("dc_first_ac_second_444", 1, 1, 941))


@case
def two_workgroups_of_the_write_pass():
    """64 x 64 4:4:4, 63 coefficients of 16 bits per block in pairs of exactly 32 bits: 24 KB of entropy data -- 379 sub-sequences of
    64 bytes, two workgroups of 256 lanes."""
    rng = np.random.default_rng(950)
    fr = BC.color(8, 8, 1, 1)
    blocks = [[(i % 3, val(rng, i % 3))] + tok(rng, *([0x0A, 0x09] * 31 + [0x0A])) for i in range(192)]
    def check(c):
        cs = c.stream.census
        assert BS.n_subseq(c.stream, 4) > 256 and sum(1 for i in range(len(cs) - 1) if taken(cs, i)) > 5000
    tabs = {(0, 0): BC.DC2, (1, 0): AC_W}
    return BC.Case("two_workgroups_of_the_write_pass", BS.write(fr, tabs, [(0, 0)] * 3, blocks), check)


_BUILT = {}


def build_all(colour=False):
    """Every case, built once per process; colour: the well-formed ones, three components each."""
    global _COLOUR
    if colour not in _BUILT:
        _COLOUR = colour
        try:
            out = [fn() for fn in CASES]
        finally:
            _COLOUR = False
        if colour:
            out = [c for c in out if c.wellformed]
            assert all(c.stream.frame.ncomp == 3 for c in out)
        assert len({c.name for c in out}) == len(out)
        _BUILT[colour] = out
    return _BUILT[colour]


def last_block_read(coefs):
    """The last row of a coefficient record that holds anything."""
    return max(i for i in range(coefs.shape[0]) if coefs[i].any())


def with_precision(data, prec):
    """The file with another sample precision in its frame header (the reference divides every decoded value by 1 << (P - 8))."""
    f = bytearray(data); i = f.index(b"\xFF\xC0")
    assert f[i + 4] == 8
    f[i + 4] = prec
    return bytes(f)
