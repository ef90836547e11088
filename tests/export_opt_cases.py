"""Content cases of the export with optimal Huffman tables -- TEST INFRASTRUCTURE shared by tests/test_export_opt_model.py (CPU: every case carries a
census that proves its claim) and tests/test_gpu_export_opt.py (the kernels, byte for byte and count for count against tests/export_opt_model.py).

A case is a grey picture given block by block in decode order, one block row (so no padding blocks change a count), all multipliers 1: every block a
dict {zig-zag position: level} (position 0: the DC level itself).  Symbols are placed one by one: an AC symbol (run, category) takes run + 1 positions
and carries the level 2^(category - 1); a block that leaves position 63 empty ends in EOB.  Slot 0 is the DC table, slot 1 the AC table.

The Fibonacci cases: with the reserved symbol (frequency 1), counts 1, 2, 3, 5, 8, ... over n symbols make every merge of K.2 take the chain built so
far, so the code tree is a comb and its deepest leaf lies exactly n deep -- past 16 for n >= 17, where Adjust_BITS has to work."""
import export_model as EM
import export_opt_model as OM
import prog_codec as PC

TILE = 256
ZRL, EOB = 0xF0, 0x00
# AC symbols in the order the builders hand them out: run 0 first (one position each), so that the largest counts take the least room
AC_ORDER = [(r << 4) | c for r in range(16) for c in range(1, 11)]


def fib(n):
    out = [1, 2]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


class Case:
    def __init__(self, name, blocks, claim):
        self.name = name; self.claim = claim
        n = len(blocks)
        assert 1 <= n <= 8000, n
        self.frame = PC.Frame(8 * n, 8, [(1, 1, 0)], {0: [1] * 64})
        assert self.frame.mcu_x == n and self.frame.mcu_y == 1
        self.nblocks = n
        coefs = self.frame.zeros()
        for i, b in enumerate(blocks):
            for z, v in b.items():
                coefs[0][0, i, z] = v
        self.coefs = coefs
        self._memo = {}

    @property
    def file(self):
        """What the library decodes before it exports: prog_codec's baseline encoding."""
        if "file" not in self._memo:
            self._memo["file"] = PC.encode_baseline(self.frame, self.coefs)
        return self._memo["file"]

    def model(self):
        """(tokens, freq by slot, tables by slot, file) of the optimal export of this case."""
        if "model" not in self._memo:
            arena, dccum, geo, qnat = EM.frame_inputs(self.frame, self.coefs)
            lev, result, _ = EM.levels(arena, dccum, geo, qnat)
            assert result == EM.OK
            res, _d, f, freq, tabs = OM.export_parts(arena, dccum, geo, self.frame.width, self.frame.height, qnat)
            assert res == OM.OK
            self._memo["model"] = (EM.tokens(lev, geo), freq, tabs, f)
        return self._memo["model"]


def ac_block(symbols):
    """A block of the AC symbols given (ZRL is not given: a run above 15 makes it)."""
    b = {}; z = 0
    for s in symbols:
        z += (s >> 4) + 1
        assert z <= 63 and 1 <= (s & 15) <= 10
        b[z] = 1 << ((s & 15) - 1)
    return b


def deal(counts, nblocks):
    """nblocks blocks that hold symbol s counts[s] times in all, dealt round robin; every block keeps position 63 empty (EOB: nblocks times)."""
    occ = [s for s, n in sorted(counts.items()) for _ in range(n)]
    per = [[] for _ in range(nblocks)]
    for i, s in enumerate(occ):
        per[i % nblocks].append(s)
    for p in per:
        if sum((s >> 4) + 1 for s in p) > 62:
            raise OverflowError
    return [ac_block(p) for p in per]


def fibonacci_blocks(n):
    """Blocks whose AC table holds n symbols (EOB among them) with the counts fib(n)."""
    f = fib(n)
    syms = AC_ORDER[:n - 7] + AC_ORDER[n - 7:n - 1][::-1]    # the six rarest in falling symbol order: the deeper code has the smaller symbol value, so the
    for e in range(n):                                  # order by code size is not the order by (final length, symbol).  EOB takes the smallest count that leaves room
        rest = sorted(f[:e] + f[e + 1:], reverse=True)
        try:
            return deal({syms[i]: c for i, c in enumerate(rest)}, f[e])
        except OverflowError:
            continue
    raise AssertionError(n)


def with_dc_diffs(blocks, diffs):
    out = []; level = 0
    for b, d in zip(blocks, diffs):
        level += d
        assert -2048 < level < 2048
        out.append({**b, 0: level})
    return out


def every_symbol_blocks():
    """All 12 DC symbols 11 times and all 162 AC symbols 6 times: six copies of 22 blocks that hold each of the 160 (run, category) symbols once, one of
    them behind a ZRL -- 1376 positions: 21 blocks filled to position 63 (no EOB) and one of 53 positions that ends in EOB."""
    items = sorted(AC_ORDER, key=lambda s: (-(s >> 4), s))
    size = {s: (s >> 4) + 1 for s in items}
    bins = []
    first = items.pop(0)                                  # (15, 1) behind a ZRL opens the first block: 32 positions
    cur = [ZRL_MARK, first]; room = 63 - 32
    while items:
        pick = next((s for s in items if size[s] <= room), None)
        if pick is None:
            assert room == 0, room
            bins.append(cur); cur = []; room = 63
            continue
        items.remove(pick); cur.append(pick); room -= size[pick]
    bins.append(cur)
    assert len(bins) == 22 and room == 10, (len(bins), room)
    blocks = []
    for p in bins:
        b = {}; z = 0
        for s in p:
            if s is ZRL_MARK:
                z += 16; continue
            z += size[s]; b[z] = 1 << ((s & 15) - 1)
        blocks.append(b)
    blocks = blocks * 6
    mags = [0] + [1 << (c - 1) for c in range(1, 12)]       # a difference of every category 0 .. 11 in turn, its sign chosen so that the level stays small
    diffs = []; level = 0
    for i in range(len(blocks)):
        m = mags[i % 12]
        diffs.append(m if level <= 0 else -m); level += diffs[-1]
    return with_dc_diffs(blocks, diffs)


ZRL_MARK = None


def cases():
    out = []
    add = lambda name, blocks, claim: out.append(Case(name, blocks, claim))
    add("one_dc_category_and_eob_alone", with_dc_diffs([{}] * 20, [5] * 20), "every table is one symbol and the reserved point: two code points")
    add("eob_the_only_ac_symbol", with_dc_diffs([{}] * 24, [0, 1, -1, 3, -3, 9, -9, 100, -100, 1000, -1000, 0] * 2), "the AC table holds EOB alone")
    add("two_symbols_of_equal_count", [{1: 1}, {1: 1}], "EOB and (0,1) twice each: the larger symbol is merged first and gets the longer code")
    add("three_symbols_of_equal_count", [{1: 1, 2: 2}, {1: 4}, {1: 1, 2: 4}, {1: 2}], "(0,1), (0,2), (0,3) twice each beside EOB four times: ties at two merges")
    add("every_symbol_with_equal_counts", every_symbol_blocks(), "12 DC symbols 11 times each, 162 AC symbols 6 times each")
    for n in (16, 17, 20, 22):
        add("fibonacci_%d" % n, fibonacci_blocks(n), "AC counts fib(%d): the deepest code is %d before the limit" % (n, n))
    add("one_symbol_70000_times", deal({0x01: 70000}, 1130), "a count above 2^16")
    add("symbol_only_in_the_partial_tile_of_257", [{}] * TILE + [{5: -3}], "(4,2) occurs in block 256 alone")
    add("symbol_only_in_the_partial_tile_of_513", [{}] * (2 * TILE) + [{5: -3}], "(4,2) occurs in block 512 alone")
    add("zrl_heavy", [{33: 1, 50: 2}, {63: 1}, {17: 1, 34: 1, 51: 1}, {}] * 5, "more ZRL than anything else")
    return out


def unlimited_depth(freq):
    return max(OM.group_codesizes(freq).values())


def check_census(case):
    """Asserts the claim the case is named after, on the model's tokens, counts and tables."""
    T, freq, tabs, f = case.model()
    nm = case.name
    dc, ac = freq[0], freq[1]
    assert sum(dc.values()) == case.nblocks and all(0 <= s <= 11 for s in dc) and all((s & 15) <= 10 for s in ac)
    if nm == "one_dc_category_and_eob_alone":
        assert dc == {3: 20} and ac == {EOB: 20} and tabs[0] == ([1] + [0] * 15, [3]) and tabs[1] == ([1] + [0] * 15, [EOB])
    if nm == "eob_the_only_ac_symbol":
        assert ac == {EOB: 24} and len(dc) > 4
    if nm == "two_symbols_of_equal_count":
        assert ac == {EOB: 2, 0x01: 2} and PC._codes(tabs[1]) == {EOB: (0, 1), 0x01: (2, 2)}
    if nm == "three_symbols_of_equal_count":
        assert ac == {EOB: 4, 0x01: 2, 0x02: 2, 0x03: 2} and {s: ln for s, (_c, ln) in PC._codes(tabs[1]).items()} == {EOB: 1, 0x01: 3, 0x02: 3, 0x03: 3}
    if nm == "every_symbol_with_equal_counts":
        assert dc == {s: 11 for s in range(12)} and ac == {s: 6 for s in AC_ORDER + [ZRL, EOB]} and len(ac) == 162
        assert len(tabs[0][1]) == 12 and len(tabs[1][1]) == 162 and len(f) - f.index(b"\xFF\xDA") > 0
    if nm.startswith("fibonacci_"):
        n = int(nm.split("_")[1])
        assert sorted(ac.values()) == fib(n) and sum(ac.values()) == {16: 4179, 17: 6763, 20: 28655, 22: 75023}[n]
        assert unlimited_depth(ac) == n
        assert max(ln for ln in range(1, 17) if tabs[1][0][ln - 1]) == min(n, 16)
    if nm == "one_symbol_70000_times":
        assert ac[0x01] == 70000 > 1 << 16 and ac[EOB] == 1130
    if nm.startswith("symbol_only_in_the_partial_tile_of_"):
        n = int(nm.rsplit("_", 1)[1])
        assert case.nblocks == n and n % TILE == 1 and ac == {EOB: n, 0x42: 1}
        starts = [i for i, t in enumerate(T) if t[0] == 0 and t[1] == 0]
        assert [i for i, t in enumerate(T) if t[:2] == (0, 1) and t[2] == 0x42][0] > starts[n - 1]
    if nm == "zrl_heavy":
        assert ac[ZRL] == max(ac.values()) and ac[ZRL] == 5 * (2 + 1 + 3 + 3)
