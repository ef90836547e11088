"""The catalogue of baseline (SOF0) files behind tests/test_base_cases.py (CPU) and tests/test_gpu_base_walks.py (GPU).

Every case is written SYMBOL BY SYMBOL with tests/base_stream.py so that a named event of the parallel entropy path (walk_sync, the
candidate kernels, k_write / k_write2, walk_slow; the table forms lut1 / lut2, lutp / lut2p, lutw of js_build_parallel_luts) is in
the stream, and carries a `check` that proves the event from the writer's census -- a change to a generator that loses the coverage
fails on the CPU, not silently on the GPU.  The truth is the oracle's decode, pinned per case to the compiled reference's recorded
digests (tests/golden/base_cases.json).

Groups.  `wellformed` cases are those the reference decodes without raising its error state (scan_bad = 0, no warning); the GPU must
decode them on the parallel path without a flag.  Three groups assert outputs only: "over_limit" (a table set that needs more
second-level entries than the LUT form has), "nosync" (streams in which a speculative walk never synchronises) and "overshoot"
(blocks whose run carries the coefficient index past 63: the reference ends the block there and sets scan_bad).  One case beyond
them, "pad_is_code" (a complete code under restart markers), is outputs-only for the same reason as the overshoots: the reference
itself reports scan_bad.
"""
from __future__ import annotations

import numpy as np

import base_stream as BS
import prog_codec as P

SYNC_WG_SUBSEQ = 256 - 2        # sub-sequences one k_sync workgroup holds: JS_SY_THREADS - JS_SY_HALO (jpegsnoop_amd/csrc/jsnoop_launch.h)

QV = [1 + k // 4 for k in range(64)]              # zig-zag order
QC = [2 + k // 3 for k in range(64)]


def gray(nbx, nby=1, q=QV):
    return P.Frame(8 * nbx, 8 * nby, [(1, 1, 0)], {0: q})


def color(mx, my, h=2, v=2, q0=QV, q1=QC):
    return P.Frame(8 * h * mx, 8 * v * my, [(h, v, 0), (1, 1, 1), (1, 1, 1)], {0: q0, 1: q1})


def table(lengths_symbols):
    """[(length, [symbols])] -> (counts, symbols)."""
    counts = [0] * 16; syms = []
    for ln, ss in sorted(lengths_symbols, key=lambda x: x[0]):
        counts[ln - 1] += len(ss); syms += list(ss)
    assert len(set(syms)) == len(syms)
    P._codes((counts, syms))                      # (asserts the code is not over-subscribed)
    return counts, syms


# The work-horse tables.  AC_PAIR: one code of every length 1..9, then 16-bit codes.  Bits per symbol (code + value):
#   0x01: 2   EOB: 2   0x21: 4   ZRL: 4   0x11: 6   0x02: 8   0x12: 9   0x03: 11   0x04: 13, sizes 10..15 and run 5: 16 + size
AC_PAIR = P.ladder_table([0x01, 0x00, 0x21, 0xF0, 0x11, 0x02, 0x12, 0x03, 0x04, 0x0F, 0x0E, 0x0D, 0x0C, 0x0B, 0x0A, 0x51, 0x05, 0x31], 1, 9)
DC2 = P.flat_table([0, 1, 2], 2)                  # category 0: '00', 1: '01', 2: '10'
DC_LADDER = P.ladder_table(list(range(16)), 1, 16)               # category n: a code of n + 1 bits
PAIR_TABS = {(0, 0): DC2, (1, 0): AC_PAIR}
BITS = {0x01: 2, 0x00: 2, 0x21: 4, 0xF0: 4, 0x11: 6, 0x02: 8, 0x12: 9, 0x03: 11, 0x04: 13}


def val(rng, size):
    """A random value of exactly `size` bits, either sign."""
    if not size:
        return 0
    m = int(rng.integers(1 << (size - 1), 1 << size))
    return m if rng.integers(2) else -m


def tok(rng, *syms):
    return [(s, val(rng, s & 15)) for s in syms]


def filler(bits, rng):
    """Blocks over PAIR_TABS (DC category 0) whose codes and values take exactly `bits` bits: 4 + 2 n + 9 m bits each."""
    out = []
    assert bits == 0 or bits >= 4 and bits not in (5, 7, 9, 11), bits
    while bits:
        take = bits if bits <= 124 else 124 if bits - 124 >= 14 else bits - 14 - (bits & 1)      # (what is left stays writable)
        m = take & 1
        n = (take - 4 - 9 * m) // 2
        assert n >= 0 and n + 2 * m <= 62, (bits, take)
        t = [(0, 0)] + tok(rng, *([0x01] * n)) + tok(rng, *([0x12] * m)) + [(0x00, 0)]
        out.append(t); bits -= take
    return out


def block_bits(t):
    return 2 + sum(BITS[s] for s, _ in t[1:])


class Case:
    def __init__(self, name, stream, check, group=None):
        self.name, self.stream, self.check, self.group = name, stream, check, group
        self.wellformed = group is None
        self.file = stream.file
        self.standard = all(c is not None for c in stream.coefs)         # a conforming decoder reads what was intended


CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def one_row(tabs, blocks, name, check, comp_ids=((0, 0),), q=QV, dri=0, **kw):
    """A gray picture of len(blocks) x 1 blocks."""
    return Case(name, BS.write(gray(len(blocks), 1, q), tabs, list(comp_ids), blocks, dri), check, **kw)


def cover_blocks(rng, dc_syms, ac_syms):
    """Blocks that use every DC symbol and every AC symbol at least once, with EOB / index 63 ends as they come."""
    blocks = []; cur = None; k = 1
    dcs = list(dc_syms)

    def open_block():
        nonlocal cur, k
        s = dcs[len(blocks) % len(dcs)]
        cur = [(s, val(rng, s))]; k = 1
    open_block()
    for sym in ac_syms:
        if sym == 0:
            continue
        adv = 16 if sym == 0xF0 else (sym >> 4) + 1
        if k + adv > 64:
            cur.append((0, 0)); blocks.append(cur); open_block()
        cur.append((sym, val(rng, sym & 15))); k += adv
        if k == 64:
            blocks.append(cur); open_block()
    cur.append((0, 0)); blocks.append(cur)
    while len(blocks) < len(dcs):
        open_block(); cur.append((0, 0)); blocks.append(cur)
    return blocks


def lens_used(census, cls):
    return {r.len for r in census if r.tab[0] == cls}


# ================================================================================================================ tables
AC_LADDER = P.ladder_table([0x01, 0x00, 0x11, 0x02, 0x21, 0xF0, 0x03, 0x31, 0x12, 0x41, 0x04, 0x51, 0x22, 0x61, 0x05, 0x13], 1, 16)


@case
def tab_ladder_every_length():
    """One code of every length 1..16 in the DC and in the AC table (9 / 10 bits: the seam of the two levels; one second-level group
    of seven extra index bits that holds the codes of 10..16 bits)."""
    rng = np.random.default_rng(101)
    blocks = []
    for rep in range(3):
        blocks += cover_blocks(rng, list(range(12)), AC_LADDER[1] * 2)
    def check(c):
        cs = c.stream.census
        assert lens_used(cs, 1) == set(range(1, 17)) and lens_used(cs, 0) == set(range(1, 13))
        assert BS.l2_groups(AC_LADDER) == {7: 1} and BS.l2_groups(DC_LADDER) == {7: 1}
    return one_row({(0, 0): DC_LADDER, (1, 0): AC_LADDER}, blocks, "tab_ladder_every_length", check)


def _ac_groups_table():
    """Short codes of 1..6 bits and one of 9, then seven second-level groups whose longest codes have 10, 11, ... 16 bits."""
    syms = [0x00, 0xF0] + [r << 4 | s for s in range(1, 16) for r in range(16)]
    cnt = [1, 1, 1, 1, 1, 1, 0, 0, 1, 2, 4, 8, 16, 32, 64, 100]
    order = [0x01, 0x00, 0x11, 0x02, 0xF0, 0x21, 0x12] + [s for s in syms if s not in (0x01, 0x00, 0x11, 0x02, 0xF0, 0x21, 0x12)]
    return cnt, order[:sum(cnt)]


AC_GROUPS = _ac_groups_table()
DC_FLAT4 = P.flat_table(list(range(12)), 4)


@case
def tab_second_level_groups_1_to_7_bits():
    """Second-level groups with 1..7 extra index bits, every symbol of every group in the stream (first and last entries included);
    DC: flat 4-bit codes; AC sizes up to 15 with 16-bit codes."""
    rng = np.random.default_rng(102)
    blocks = cover_blocks(rng, list(range(12)), AC_GROUPS[1])
    def check(c):
        assert BS.l2_groups(AC_GROUPS) == {n: 1 for n in range(1, 8)}
        used = {r.sym for r in c.stream.census if r.tab[0] == 1}
        assert used == set(AC_GROUPS[1]), "every symbol of the table"
        assert lens_used(c.stream.census, 1) == {1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16}
    return one_row({(0, 0): DC_FLAT4, (1, 0): AC_GROUPS}, blocks, "tab_second_level_groups_1_to_7_bits", check)


def _flat_case(lens, seed):
    """Flat tables: per component a DC and an AC table whose codes all have ONE length; three lengths per file."""
    name = "tab_flat_%d_%d_%d" % lens
    def build():
        rng = np.random.default_rng(seed)
        fr = color(4, 3, 1, 1)
        tabs = {}; ids = []
        acs = [0x00, 0x01, 0x02, 0x11, 0xF0, 0x23, 0x31]
        for i, L in enumerate(lens):
            n_dc = min(12, (1 << L) - 1); n_ac = min(len(acs), (1 << L) - 1)
            tabs[(0, i)] = P.flat_table(list(range(n_dc)), L); tabs[(1, i)] = P.flat_table(acs[:n_ac], L); ids.append((i, i))
        per = []
        for i, L in enumerate(lens):
            b = []
            while len(b) < 12:
                b += cover_blocks(rng, tabs[(0, i)][1], tabs[(1, i)][1] * 2)
            per.append(b[:12])
        blocks = [per[c][u] for u in range(12) for c in range(3)]
        def check(c):
            for i, L in enumerate(lens):
                assert {r.len for r in c.stream.census if r.tab[1] == i} == {L}
        return Case(name, BS.write(fr, tabs, ids, blocks), check)
    build.__name__ = name
    return build


for _i, _l in enumerate([(1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12), (13, 14, 15), (16, 9, 10)]):
    CASES.append(_flat_case(_l, 110 + _i))


@case
def tab_one_code_only_gray():
    """DC symbol 0 alone and EOB alone, one bit each: every block is the two bits 00."""
    blocks = [[(0, 0), (0, 0)]] * 40
    def check(c):
        assert c.stream.bits == 80 and all(r.len == 1 for r in c.stream.census)
        assert c.stream.tabs[(0, 0)][1] == [0] and c.stream.tabs[(1, 0)][1] == [0]
    return one_row({(0, 0): table([(1, [0])]), (1, 0): table([(1, [0])])}, blocks, "tab_one_code_only_gray", check)


def _complete_code(name, dri, group):
    """Complete codes: DC '0' / '1' for categories 0 / 1, AC '0' EOB, '10' 0x01, '11' 0x11 -- the all-ones word is a code.  With
    restart markers the pad bits in front of a marker are codes too: the reference, whose restart is driven by "no code fits", reads
    them as symbols (scan_bad) -- outputs only."""
    def build():
        rng = np.random.default_rng(104)
        blocks = []
        for i in range(60):
            n = int(rng.integers(0, 20))
            t = [(1, val(rng, 1)) if i % 3 else (0, 0)] + tok(rng, *[(0x11 if rng.integers(2) else 0x01) for _ in range(n)]) + [(0, 0)]
            blocks.append(t)
        def check(c):
            assert c.stream.tabs[(1, 0)][0][:2] == [1, 2] and c.stream.tabs[(0, 0)][0][0] == 2
            assert any(r.sym == 0x11 for r in c.stream.census) and len(c.stream.iv_ends) == (20 if dri else 1)
            if dri:
                assert {(-e) % 8 for e in c.stream.iv_ends} >= {1, 2, 3, 4, 5, 6, 7}, "pad bits of every length, all of them codes"
        return one_row({(0, 0): table([(1, [0, 1])]), (1, 0): table([(1, [0]), (2, [0x01, 0x11])])}, blocks, name, check, dri=dri, group=group)
    build.__name__ = name
    return build


CASES.append(_complete_code("tab_complete_code_all_ones_is_a_code", 0, None))
CASES.append(_complete_code("tab_complete_code_pad_bits_are_codes_dri_3", 3, "pad_is_code"))


def _sharing(name, ids, tabs, seed, rows):
    def build():
        rng = np.random.default_rng(seed)
        fr = color(5, 4)
        bpm = fr.mcu_blocks(); blocks = []
        for u in range(20):
            for c, _y, _x in bpm:
                dc = tabs[(0, ids[c][0])][1]; ac = [s for s in tabs[(1, ids[c][1])][1] if s and s & 15]
                n = int(rng.integers(0, 12)); d = int(dc[int(rng.integers(len(dc)))])
                t = [(d, val(rng, d))] + tok(rng, *[int(ac[int(rng.integers(len(ac)))]) for _ in range(n)])
                k = 1 + sum((s >> 4) + 1 for s, _ in t[1:])
                assert k <= 64
                blocks.append(t + ([(0, 0)] if k < 64 else []))
        def check(c):
            assert len(BS.distinct_tables(tabs, ids, 3)) == rows
            assert {r.tab for r in c.stream.census} == {(cls, ids[k][cls]) for k in range(3) for cls in (0, 1)}
        return Case(name, BS.write(fr, tabs, ids, blocks), check)
    build.__name__ = name
    return build


_SH = P.ladder_table([0, 1, 2, 3, 4, 5, 6], 2, 7)                 # as a DC table: categories; as an AC table: EOB and run 0 sizes 1..6
_SH2 = P.ladder_table([2, 0, 1, 3, 4, 6, 5], 1, 7)
CASES.append(_sharing("share_all_slots_identical", [(0, 0), (1, 1), (2, 2)], {(cls, i): _SH for cls in (0, 1) for i in range(3)}, 120, 2))
CASES.append(_sharing("share_luma_chroma_distinct", [(0, 0), (1, 1), (1, 1)], {(0, 0): _SH, (1, 0): _SH2, (0, 1): _SH2, (1, 1): AC_PAIR}, 121, 4))
CASES.append(_sharing("share_six_distinct_tables", [(0, 0), (1, 1), (2, 2)],
                      {(0, 0): _SH, (1, 0): _SH2, (0, 1): _SH2, (1, 1): AC_PAIR, (0, 2): P.flat_table(list(range(7)), 3), (1, 2): AC_LADDER}, 122, 6))


def _big_ac(p, rot):
    """An AC table that needs 2 p + 384 second-level entries: codes of 1..3 bits, p full prefixes of 10-bit codes, one prefix that
    holds codes of 10, 11, ... 16 bits, one prefix full of 16-bit codes and one 16-bit code under a last prefix."""
    syms = [0x01, 0x00, 0x11] + [r << 4 | s for r in range(16) for s in range(1, 16) if (r << 4 | s) not in (0x01, 0x11)] + [0xF0]
    body = syms[3:]; body = body[rot:] + body[:rot]
    cnt = [1, 1, 1, 0, 0, 0, 0, 0, 0, 2 * p + 1, 1, 1, 1, 1, 1, 2 + 128 + 1]
    return cnt, (syms[:3] + body)[:sum(cnt)]


def _big_dc(rot):
    """A DC table (16 categories) that needs 256 second-level entries: codes of 1..7 bits, a prefix with codes of 10..16 bits, and one
    16-bit code under the next prefix."""
    s = list(range(16)); s = s[rot:] + s[:rot]
    return [1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 3], s


def _limit_case(name, ps, want, group):
    def build():
        rng = np.random.default_rng(130)
        tabs = {}
        for i in range(3):
            tabs[(0, i)] = _big_dc(4 + i); tabs[(1, i)] = _big_ac(ps[i], 7 * i)
        ids = [(0, 0), (1, 1), (2, 2)]
        fr = color(6, 4, 1, 1); blocks = []
        per = []
        for i in range(3):
            # the longest codes of every table (its last symbols) and a mix of the rest, categories <= 11 and no run/0 symbols
            ac = [s for s in tabs[(1, i)][1] if s in (0, 0xF0) or s & 15]
            pick = ac[-6:] + ac[:8] + [ac[int(j)] for j in rng.integers(0, len(ac), 120)]
            b = cover_blocks(rng, [d for d in tabs[(0, i)][1] if d <= 11], pick)
            assert len(b) <= 24
            while len(b) < 24:
                b.append([(0, 0), (0, 0)])
            per.append(b)
        blocks = [per[c][u] for u in range(24) for c in range(3)]
        def check(c):
            need = BS.lut2_need(tabs, ids, 3)
            assert need == want and (need <= BS.LUT2_MAX) == (group is None), need
            assert len(BS.distinct_tables(tabs, ids, 3)) == 6
            assert {r.tab for r in c.stream.census if r.len == 16} == set(tabs), "a 16-bit code of every table"
        return Case(name, BS.write(fr, tabs, ids, blocks), check, group=group)
    build.__name__ = name
    return build


CASES.append(_limit_case("lut2_need_exactly_2048", (20, 21, 23), 2048, None))
CASES.append(_limit_case("lut2_need_2050_over_the_limit", (20, 21, 24), 2050, "over_limit"))


def _wide_values(name, qv, seed):
    def build():
        rng = np.random.default_rng(seed)
        q = [qv] * 64
        fr = color(4, 3, 2, 1, q, q)
        ac = P.flat_table([0x00, 0xF0] + list(range(1, 16)) + [0x10 | s for s in range(10, 16)], 8)
        tabs = {(0, 0): DC_LADDER, (1, 0): ac}; ids = [(0, 0)] * 3
        blocks = []
        ext = lambda s, sign, top: sign * ((1 << s) - 1 if top else 1 << (s - 1))
        i = 0
        for u in range(12):
            for c, _y, _x in fr.mcu_blocks():
                s = 12 + i % 4 if i % 3 else int(rng.integers(0, 12))
                t = [(s, ext(s, 1 if i % 2 else -1, i % 5 < 3) if s else 0)]
                k = 1
                for j in range(int(rng.integers(3, 20))):
                    sz = 11 + (i + j) % 5 if j % 2 else int(rng.integers(1, 16))
                    sym = (0x10 | sz) if (sz >= 10 and (i + j) % 3 == 0) else sz
                    if k + (sym >> 4) + 1 > 63:
                        break
                    t.append((sym, ext(sz, 1 if (i + j) % 2 else -1, (i + j) % 3 != 1) if j % 4 else val(rng, sz))); k += (sym >> 4) + 1
                blocks.append(t + [(0, 0)]); i += 1
        def check(c):
            cs = c.stream.census
            assert {r.sym for r in cs if r.tab[0] == 0} >= {12, 13, 14, 15}
            assert {r.size for r in cs if r.tab[0] == 1} >= {11, 12, 13, 14, 15}
            assert set(c.stream.frame.qtabs[0]) == {qv}
        return Case(name, BS.write(fr, tabs, ids, blocks), check)
    build.__name__ = name
    return build


CASES.append(_wide_values("wide_values_q1", 1, 140))
CASES.append(_wide_values("wide_values_q255", 255, 141))


@case
def run_zero_symbols_run_1_to_14():
    """AC symbols run/0 with run 1..14: the reference stores a zero and advances run + 1."""
    rng = np.random.default_rng(150)
    ac = P.ladder_table([0x01, 0x00, 0x10, 0x20, 0x30, 0x02, 0x40, 0x50] + [r << 4 for r in range(6, 15)] + [0xF0, 0x11], 1, 8)
    blocks = []
    for i in range(48):
        t = [(i % 3, val(rng, i % 3))]; k = 1
        while True:
            sym = int([0x01, 0x02, 0x11, 0xF0][int(rng.integers(4))]) if rng.integers(3) == 0 else int(rng.integers(1, 15)) << 4
            adv = 16 if sym == 0xF0 else (sym >> 4) + 1
            if k + adv > 64:
                break
            t.append((sym, val(rng, sym & 15))); k += adv
            if k == 64 or rng.integers(12) == 0:
                break
        blocks.append(t + ([(0, 0)] if k < 64 else []))
    def check(c):
        cs = c.stream.census
        assert {r.sym for r in cs} >= {r << 4 for r in range(1, 15)}
        assert any(r.sym & 15 == 0 and 0 < r.sym < 0xF0 and r.k + (r.sym >> 4) + 1 == 64 for r in cs), "a run/0 symbol that ends its block at 64"
        assert any(BS.pair_visible(cs, i) and cs[i + 1].sym in (0x10, 0x20, 0x30) for i in range(len(cs))), "run/0 as the second symbol of a pair"
    return one_row({(0, 0): DC2, (1, 0): ac}, blocks, "run_zero_symbols_run_1_to_14", check)


# ================================================================================================================ pair entries
def up_to(rng, k):
    """Tokens that carry the coefficient index from 1 to k (ZRLs, then single coefficients)."""
    t = []; cur = 1
    while k - cur >= 16:
        t.append((0xF0, 0)); cur += 16
    return t + tok(rng, *([0x01] * (k - cur)))


def pairs_in(census, first, second, **kw):
    """Indices i with census[i].sym == first, census[i + 1].sym == second in one block (+ conditions on census[i])."""
    return [i for i in range(len(census) - 1) if census[i].sym == first and census[i + 1].sym == second and census[i].blk == census[i + 1].blk
            and census[i].k > 0 and all(getattr(census[i], a) == v for a, v in kw.items())]


@case
def pair_visibility_edges():
    """Two symbols in one 9-bit window: taken (8 bits + a 1-bit code; 6 bits + a 3-bit code whose value bit is outside), not taken
    (first symbol of 9 bits; second code one bit longer than what is left), second symbol EOB / ZRL."""
    rng = np.random.default_rng(201)
    combos = [(0x02, 0x01), (0x12, 0x01), (0x02, 0x00), (0x11, 0x21), (0x11, 0xF0), (0x01, 0x00), (0x01, 0xF0), (0x01, 0x01), (0x21, 0x11), (0x01, 0x12),
              (0x21, 0x21), (0x11, 0x01), (0xF0, 0x01), (0xF0, 0xF0), (0xF0, 0x00), (0x03, 0x01),
              (0x02, 0x21), (0x02, 0xF0), (0x11, 0x11), (0x11, 0x02), (0x21, 0x12), (0x01, 0x03)]      # (the last six: a code that leaves the window, and is not the one its visible bits padded with zeros would spell)
    blocks = []
    for a, b in combos * 3:
        pre = tok(rng, *([0x01] * int(rng.integers(0, 5))))
        d = int(rng.integers(3)); t = [(d, val(rng, d))] + pre + tok(rng, a, b)
        blocks.append(t + ([(0, 0)] if b else []))
    def check(c):
        cs = c.stream.census
        vis = lambda a, b: [BS.pair_visible(cs, i) for i in pairs_in(cs, a, b)]
        for a, b, want in [(0x02, 0x01, True), (0x12, 0x01, False), (0x02, 0x00, False), (0x11, 0x21, True), (0x11, 0xF0, False), (0x01, 0x00, True),
                           (0x01, 0xF0, True), (0x21, 0x11, True), (0x01, 0x12, True), (0x03, 0x01, False), (0xF0, 0x00, True),
                           (0x02, 0x21, False), (0x02, 0xF0, False), (0x11, 0x11, False), (0x11, 0x02, False), (0x21, 0x12, False), (0x01, 0x03, False)]:
            v = vis(a, b)
            assert len(v) >= 3 and all(x == want for x in v), (hex(a), hex(b), v)
    return one_row(PAIR_TABS, blocks, "pair_visibility_edges", check)


@case
def pair_first_symbol_leaves_index_62_63_64():
    """Visible pairs whose first symbol leaves the coefficient index at 62, 63 and 64.  At 64 the block is over: what the window shows
    behind it is the next block's DC code ('00' / '01' read through the AC table: 0x01), and the pair must not be taken."""
    rng = np.random.default_rng(202)
    blocks = []
    for rep in range(6):
        for k_after in (62, 63, 64):
            for first in (0x01, 0x21, 0x11):
                adv = (first >> 4) + 1
                t = [(rep % 2, val(rng, rep % 2))] + up_to(rng, k_after - adv) + tok(rng, first)
                if k_after < 64:
                    t += tok(rng, 0x01) if k_after == 63 or rep % 2 else [(0x00, 0)]
                    if k_after == 62 and rep % 2:
                        t += tok(rng, 0x01)
                blocks.append(t)
    blocks.append([(0, 0), (0, 0)])
    def check(c):
        s = c.stream; cs = s.census
        for first in (0x01, 0x21, 0x11):
            adv = (first >> 4) + 1
            for k_after in (62, 63):
                assert any(BS.pair_visible(cs, i) for i in range(len(cs) - 1) if cs[i].sym == first and cs[i].k + adv == k_after), (hex(first), k_after)
            ends = [i for i in range(len(cs) - 1) if cs[i].sym == first and cs[i].k + adv == 64]
            assert len(ends) >= 6
            for i in ends:                          # the window behind the block's last symbol spells a whole AC code
                a = cs[i]; assert cs[i + 1].k == 0
                assert BS.code_at(s, AC_PAIR, a.pos + a.len + a.size, BS.L1_BITS - a.len - a.size) is not None
    return one_row(PAIR_TABS, blocks, "pair_first_symbol_leaves_index_62_63_64", check)


@case
def pair_second_symbol_reaches_index_64():
    """Visible pairs whose second symbol ends the block exactly at index 64 by its run (0x21 from 61, 0x11 from 62, ZRL from 48)."""
    rng = np.random.default_rng(203)
    blocks = []
    for rep in range(4):
        for first, second in ((0x01, 0x21), (0x01, 0x11), (0x21, 0x11), (0x01, 0xF0), (0x11, 0x21)):
            a1 = (first >> 4) + 1; a2 = 16 if second == 0xF0 else (second >> 4) + 1
            blocks.append([(rep % 3, val(rng, rep % 3))] + up_to(rng, 64 - a1 - a2) + tok(rng, first, second))
    blocks.append([(0, 0), (0, 0)])
    def check(c):
        cs = c.stream.census
        n = [i for i in range(len(cs) - 1) if BS.pair_visible(cs, i) and cs[i + 1].k + (16 if cs[i + 1].sym == 0xF0 else (cs[i + 1].sym >> 4) + 1) == 64]
        assert len(n) >= 20 and {cs[i + 1].sym for i in n} == {0x21, 0x11, 0xF0}
        assert all(x is not None for x in c.stream.coefs)
    return one_row(PAIR_TABS, blocks, "pair_second_symbol_reaches_index_64", check)


PLACES = (256, 512, 1024, 2048, 4096, 8192)      # bit positions: the ends of the sub-sequences of sub_wl 4..8 and (256 .. 4096) their middles


def _sweep(name, first, second, d, seed):
    """The pair (first, second), moved so that the SECOND symbol starts d bits behind each of PLACES."""
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
            hits = [i for i in pairs_in(cs, first, second) if BS.pair_visible(cs, i) and cs[i + 1].pos - d in PLACES]
            assert [cs[i + 1].pos - d for i in hits] == list(PLACES)
            for wl in range(4, 9):
                assert any(cs[i + 1].pos - d == BS.sub_bits(wl) for i in hits) and any(cs[i + 1].pos - d == BS.sub_bits(wl) // 2 for i in hits)
        return one_row(PAIR_TABS, blocks, name, check)
    build.__name__ = name
    return build


for _pi, (_a, _b) in enumerate(((0x02, 0x01), (0x01, 0x00), (0x01, 0xF0), (0x11, 0x21))):
    for _d in (-1, 0, 1):
        CASES.append(_sweep("sweep_pair_%02x_%02x_second_at_%+d" % (_a, _b, _d), _a, _b, _d, 210 + 3 * _pi + _d))


@case
def sweep_pair_at_restart_interval_ends():
    """A visible pair as the last two symbols of a restart interval, the interval's data ending 7 .. 0 bits in front of the byte the
    marker follows; and intervals whose last block ends at index 64 by the FIRST symbol of what the pad bits make look like a pair."""
    rng = np.random.default_rng(230)
    blocks = []
    for pad in range(8):
        for first, second in ((0x01, 0x00), (0x02, 0x00), (0x11, 0x21), (0x01, 0x01)):
            tail = tok(rng, first, second) + ([(0, 0)] if second else [])
            if second == 0x01:                   # no EOB: the block runs to index 64
                tail = up_to(rng, 62) + tok(rng, first, second)
            nbits = 2 + sum(BITS[s] for s, _ in tail)
            lead = (-(nbits + pad)) % 8
            while lead in (1, 2, 3, 5, 7):
                lead += 8
            f = filler(lead + 16, rng)
            assert len(f) == 1
            blocks += [f[0], [(0, 0)] + tail]
    def check(c):
        s = c.stream; cs = s.census
        assert len(s.iv_ends) == 32 and {(-e) % 8 for e in s.iv_ends} == set(range(8))
        last = {}
        for i, r in enumerate(cs):
            last[r.iv] = i
        assert sum(1 for iv, i in last.items() if BS.pair_visible(cs, i - 1)) >= 24
        assert sum(1 for iv, i in last.items() if cs[i].sym == 0x01 and cs[i].k == 63) == 8
    return one_row(PAIR_TABS, blocks, "sweep_pair_at_restart_interval_ends", check, dri=2)


# ==================================================================================================================== geometry
@case
def symbol_of_31_bits_over_a_subsequence_end():
    """A 16-bit code with 15 value bits, starting 1 .. 32 bits in front of the end of a 64-byte sub-sequence."""
    rng = np.random.default_rng(301)
    blocks = []; cur = 0
    for j in range(1, 33):
        start = 512 * j - j                      # 32 sub-sequence ends, 32 phases
        lead = start - 2 - cur
        blocks += filler(lead, rng)
        t = [(0, 0)] + tok(rng, 0x0F) + [(0, 0)]
        blocks.append(t); cur = start + 31 + 2
    blocks += filler(40, rng)
    def check(c):
        big = [r for r in c.stream.census if r.sym == 0x0F]
        assert all(r.len == 16 and r.size == 15 for r in big)
        assert sorted(BS.to_sub_end(r) for r in big) == list(range(1, 33))
        assert len({BS.subseq(r) for r in big}) == 32
    return one_row(PAIR_TABS, blocks, "symbol_of_31_bits_over_a_subsequence_end", check)


@case
def blocks_longer_than_a_subsequence():
    """63 coefficients per block, each a 16-bit code and 10..15 value bits: 200..245 bytes per block."""
    rng = np.random.default_rng(302)
    blocks = []
    for i in range(36):
        v = [i % 2] + [val(rng, 10 + int(rng.integers(6))) for _ in range(63)]
        blocks.append(v)
    def check(c):
        cs = c.stream.census
        starts = [r.pos for r in cs if r.k == 0]
        sizes = np.diff(starts + [c.stream.iv_ends[-1]])
        assert sizes.min() >= 200 * 8 and sizes.max() <= 246 * 8, (sizes.min(), sizes.max())
        per64 = np.bincount([p // 512 for p in starts]); per128 = np.bincount([p // 1024 for p in starts])
        assert per64.max() == 1 and (per64 == 0).sum() > 2 * len(blocks) and per128.max() == 1
    return Case("blocks_longer_than_a_subsequence", BS.write(gray(6, 6), PAIR_TABS, [(0, 0)], blocks), check)


ONE_BIT = {(0, 0): table([(1, [0])]), (1, 0): table([(1, [0])])}


def _two_bit_blocks(name, frame, per_mcu, dri=0, iv_bytes=(2, 3)):
    def build():
        n = frame.mcu_x * frame.mcu_y * per_mcu
        def check(c):
            s = c.stream
            assert len(frame.mcu_blocks()) == per_mcu
            if not dri:
                assert s.bits == 2 * n + (-2 * n) % 8 and n >= 1024
                assert np.bincount([r.pos // 512 for r in s.census if r.k == 0])[0] == 256, "256 blocks start in one 64-byte sub-sequence"
            else:
                ivb = {(e + 7) // 8 - (s.iv_ends[i - 1] + 7) // 8 if i else (e + 7) // 8 for i, e in enumerate(s.iv_ends)}
                assert ivb <= set(iv_bytes) and len(s.iv_ends) >= 6, ivb
        tabs = {k: v for k, v in ONE_BIT.items()}
        return Case(name, BS.write(frame, tabs, [(0, 0)] * frame.ncomp, [[(0, 0), (0, 0)]] * n, dri), check)
    build.__name__ = name
    return build


CASES.append(_two_bit_blocks("two_bit_blocks_gray", gray(64, 20), 1))
CASES.append(_two_bit_blocks("two_bit_blocks_420", color(16, 12), 6))
CASES.append(_two_bit_blocks("two_bit_blocks_luma_4x4", color(8, 8, 4, 4), 18))
CASES.append(_two_bit_blocks("two_bit_blocks_420_dri_1", color(12, 8), 6, dri=1))
CASES.append(_two_bit_blocks("two_bit_blocks_luma_4x4_dri_1", P.Frame(96, 64, [(4, 4, 0), (1, 1, 0), (1, 1, 0)], {0: QV}), 18, dri=1, iv_bytes=(5,)))


def _scan_end(name, bits, seed):
    def build():
        rng = np.random.default_rng(seed)
        blocks = filler(bits, rng)
        def check(c):
            assert c.stream.iv_ends == [bits] and c.stream.bits == (bits + 7) // 8 * 8
        return one_row(PAIR_TABS, blocks, name, check)
    build.__name__ = name
    return build


CASES.append(_scan_end("scan_ends_at_a_subsequence_end_320_bytes", 320 * 8, 310))
CASES.append(_scan_end("scan_ends_at_a_row_end_4096_bytes", 4096 * 8, 311))            # 64 sub-sequences of 64 B: the last 256-byte row is full
CASES.append(_scan_end("scan_ends_on_a_word_324_bytes", 324 * 8, 312))
CASES.append(_scan_end("last_subsequence_holds_one_bit", 5 * 512 + 1, 313))
CASES.append(_scan_end("last_subsequence_holds_one_bit_at_1_KiB", 8192 + 1, 314))


@case
def restart_intervals_pad_bits_0_to_7():
    """DRI 1, intervals of 2 .. 3 bytes, every number of pad bits."""
    rng = np.random.default_rng(320)
    blocks = []
    for i in range(160):
        blocks += filler([16, 10, 12, 14, 20, 13, 15, 17, 19, 21, 23, 18, 22][i % 13], rng)
    def check(c):
        s = c.stream
        assert {(-e) % 8 for e in s.iv_ends} == set(range(8)) and len(s.iv_ends) == 160
        per = np.bincount([r.iv for r in s.census if r.k == 0]); assert per.max() == 1
        assert np.bincount([e // 512 for e in s.iv_ends]).max() >= 20, "dozens of intervals in one sub-sequence"
    return one_row(PAIR_TABS, blocks, "restart_intervals_pad_bits_0_to_7", check, dri=1)


@case
def restart_interval_ends_at_subsequence_ends():
    """Intervals of exactly 64 bytes (interval end = sub-sequence end, no pad bit), and of 64 bytes less one bit."""
    rng = np.random.default_rng(321)
    blocks = []
    for i in range(8):
        f = filler(512 - (i % 2), rng)
        assert len(f) == 5
        blocks += f
    def check(c):
        s = c.stream
        assert s.iv_ends == [512 * (i + 1) - (i % 2) for i in range(8)] and s.bits == 4096
    return one_row(PAIR_TABS, blocks, "restart_interval_ends_at_subsequence_ends", check, dri=5)


NOSYNC_TABS = {(0, 0): P.flat_table([1], 2), (1, 0): P.flat_table([0x01], 2)}


def _nosync(name, nbx, nby, seed):
    """Every symbol is three bits ('00' + one value bit), every block 64 symbols, no EOB anywhere: a walk that enters with the wrong
    coefficient index parses every symbol and keeps its wrong phase to the end of the picture."""
    def build():
        rng = np.random.default_rng(seed)
        n = nbx * nby
        blocks = [[(1, val(rng, 1))] + tok(rng, *([0x01] * 63)) for _ in range(n)]
        def check(c):
            s = c.stream
            assert all(r.len + r.size == 3 for r in s.census) and not any(r.sym == 0 for r in s.census) and s.bits == n * 192
            assert all(r.pos % 3 == 0 for r in s.census)
            nsub = BS.n_subseq(s)
            assert nsub == -(-n * 24 // 64)
            # the sub-sequences start at every coefficient index modulo 64 a multiple of 3 bits allows, nearly none at a block start
            at_start = sum(1 for i in range(nsub) if (i * 512) % 192 == 0)
            assert at_start * 3 <= nsub + 2
            return nsub
        return Case(name, BS.write(gray(nbx, nby), NOSYNC_TABS, [(0, 0)], blocks), check, group="nosync")
    build.__name__ = name
    return build


CASES.append(_nosync("never_synchronises_40_subsequences", 12, 9, 330))            # 108 blocks: 40.5 sub-sequences of 64 B
CASES.append(_nosync("never_synchronises_600_subsequences", 40, 40, 331))          # 1600 blocks: 600 sub-sequences (> one k_sync workgroup's, at 64 and 128 B)


# ========================================================================================================== malformed endings
def _ending(kind, rng):
    """One block of the given kind: tokens."""
    d = int(rng.integers(3)); t = [(d, val(rng, d))]
    if kind == "zrl_at_48":                       # legal: 48 + 16 = 64
        return t + up_to(rng, 48) + [(0xF0, 0)]
    if kind == "zrl_at_49":                       # 49 + 16 = 65
        return t + up_to(rng, 49) + [(0xF0, 0)]
    if kind == "run_single":                      # 0x51 (a 16-bit code: never part of a pair) from index 60: 60 + 5 = 65 > 63
        return t + up_to(rng, 60) + tok(rng, 0x51)
    if kind == "run_second_of_pair":              # 0x01 leaves 63, 0x21 (3-bit code, visible) asks for index 65
        return t + up_to(rng, 62) + tok(rng, 0x01, 0x21)
    raise KeyError(kind)


def _malformed(kind, where, seed):
    name = "ending_%s_%s" % (kind, where)
    def build():
        rng = np.random.default_rng(seed)
        fr = color(4, 3); n = 12 * 6
        at = {"first_block_of_an_mcu": 5 * 6, "last_block_of_an_mcu": 5 * 6 + 5, "last_block_of_the_image": n - 1}[where]
        blocks = []
        for i in range(n):
            if i == at:
                blocks.append(_ending(kind, rng)); continue
            d = int(rng.integers(3))
            blocks.append([(d, val(rng, d))] + tok(rng, *[[0x01, 0x11, 0x02, 0x21, 0x03][int(x)] for x in rng.integers(0, 5, int(rng.integers(0, 9)))]) + [(0, 0)])
        def check(c):
            cs = [r for r in c.stream.census if r.blk == at]
            last = cs[-1]; end = last.k + (16 if last.sym == 0xF0 else (last.sym >> 4) + 1)
            assert end == {"zrl_at_48": 64, "zrl_at_49": 65}.get(kind, 66), end
            assert (c.stream.coefs[at] is None) == (kind != "zrl_at_48")
            if kind == "run_second_of_pair":
                full = c.stream.census; i = full.index(last)
                assert BS.pair_visible(full, i - 1) and full[i - 1].k == 62
            if kind == "run_single":
                assert last.len == 16
        return Case(name, BS.write(fr, {(0, 0): DC2, (1, 0): AC_PAIR, (0, 1): DC2, (1, 1): AC_PAIR}, [(0, 0), (1, 1), (1, 1)], blocks), check,
                    group=None if kind == "zrl_at_48" else "overshoot")
    build.__name__ = name
    return build


for _k, _kind in enumerate(("zrl_at_48", "zrl_at_49", "run_single", "run_second_of_pair")):
    for _w, _where in enumerate(("first_block_of_an_mcu", "last_block_of_an_mcu", "last_block_of_the_image")):
        CASES.append(_malformed(_kind, _where, 400 + 3 * _k + _w))


# ------------------------------------------------------------------------------------------------------------------ access
_BUILT = None


def build_all():
    """Every case, built once per process, in catalogue order (tests/test_base_cases.py runs every `check`)."""
    global _BUILT
    if _BUILT is None:
        out = []
        for fn in CASES:
            out.append(fn())
        assert len({c.name for c in out}) == len(out)
        _BUILT = out
    return _BUILT


def built(name):
    return next(c for c in build_all() if c.name == name)
