"""The catalogue of DAMAGED and IRREGULAR progressive (SOF2) files behind tests/test_prog_damage_cases.py (CPU) and
tests/test_gpu_prog_damaged.py (GPU): the sibling of tests/prog_cases.py for what JPEGsnoop mostly sees.

Every case is a small frame whose coefficients are WRITTEN so that the encoder's token stream is regular (the same number of
Huffman symbols in every block), coded by tests/prog_codec.py, with ONE named, deliberate irregularity: a token replaced (the
`tokens` hook of the encoder), an interval's bytes cut (token kind 3 or the `bytes` hook) or the file cut (`post`).  No bit is
flipped blindly.  The truth is what prog_codec.decode(file, lenient=True) holds at EOI -- the damage contract of DESIGN.md 4.5 --
and every case carries a `check` that proves from the model's record (scan, interval, unit, reason) that the event happened
where it was meant to.

Kinds: 'stop' (decoding of one interval stops: the file is flagged, the strict decoder refuses it), 'accepted' (irregular but
decoded: not flagged, the intended coefficients are asserted), 'runout' (data that runs out or intervals that go missing or
shift), 'seam' (one bad interval at a wave / workgroup / lane-group edge of the kernels among 320).

Frames are at most 64 x 64 with unit quantisers, except the seam frames (grey 20 x 16 blocks, 4:2:0 20 x 16 MCUs); every file
is under 20 KB.  `same_as_clean` says whether the truth is what the file without the irregularity holds (asserted either way).  WIDE names the cases whose truth the baseline writer cannot code (DC differences of more than 11 bits): only
the wide-DC cases, by construction.
"""
from __future__ import annotations

import numpy as np

import prog_cases as PC
import prog_codec as P

S = PC.S
ONES = [1] * 64
SEAMS = (0, 63, 64, 255, 256, 319)         # edges of a wave (64 lanes) and of a workgroup (256 threads) of the lane form, and of the lane groups of 2..16 intervals per wave
NO_CODE = [(1, 0xFFFF, 16)]                # sixteen ones: the optimal tables reserve the all-ones code point (K.2), so this matches nothing


class DCase:
    def __init__(self, name, kind, frame, coefs, script, check, post=None, flagged=None, same_as_clean=False):
        self.name, self.kind, self.frame, self.coefs, self.script, self.check, self.post = name, kind, frame, coefs, script, check, post
        self.expect_flagged = {"stop": True, "accepted": False}.get(kind) if flagged is None else flagged
        self.same_as_clean = same_as_clean

    def clean_script(self):
        return [{k: v for k, v in P._norm_scan(s).items() if k not in ("tokens", "bytes")} for s in self.script]

    def build(self):
        self.file = P.encode_progressive(self.frame, self.coefs, self.script)
        if self.post:
            self.file = self.post(self)
        self.clean_file = P.encode_progressive(self.frame, self.coefs, self.clean_script())
        self.clean = P.decode(self.clean_file)
        self.dec = P.decode(self.file, lenient=True)
        self.truth = self.dec.coefs; self.flagged = self.dec.flagged
        self.arena = P.arena(self.frame, self.truth)
        try:
            self.base = P.encode_baseline(self.frame, self.truth)
        except AssertionError:                                   # a DC difference / AC value the sequential writer has no category for
            self.base = None
        return self

    def owner(self, comp, k):
        return [i for i, s in enumerate(self.dec.scans) if comp in s["comps"] and s["ss"] <= k <= s["se"]]

    def record(self):
        """What the model saw go wrong, one line: scan, interval, unit, reason."""
        out = []
        for i, s in enumerate(self.dec.scans):
            out += ["scan %d interval %d unit %d: stop (%s)" % (i, iv, u, why) for iv, u, why in s["stops"]]
            out += ["scan %d interval %d unit %d: overran in a %s" % (i, iv, u, what) for iv, u, what in s["overran"]]
            if s["missing"]:
                out.append("scan %d: %d of %d intervals missing" % (i, s["missing"], s["want"]))
            if s["surplus"]:
                out.append("scan %d: %d surplus intervals" % (i, s["surplus"]))
            out += ["scan %d interval %d unit %d: accepted %s" % (i, iv, u, what) for iv, u, what in s["irregular"][:4]]
        return "; ".join(out) or "nothing irregular"


# ------------------------------------------------------------------------------------------------------------- token editing
def sym_at(T, iv, nth):
    """Index in T of the nth Huffman symbol token of restart interval iv."""
    cur = 0; k = 0
    for i, (kind, _a, _b) in enumerate(T):
        if kind == 2:
            cur += 1
        elif kind == 0 and cur == iv:
            if k == nth:
                return i
            k += 1
    raise AssertionError("interval %d has no symbol %d" % (iv, nth))


def edit(iv, nth, new, drop=1, after=0):
    """tokens hook: `drop` tokens from (the nth symbol of interval iv) + after are replaced by `new`."""
    def f(T):
        i = sym_at(T, iv, nth) + after
        return T[:i] + list(new) + T[i + drop:]
    return f


def whole_interval(iv, new):
    """tokens hook: every token of interval iv is replaced by `new`."""
    def f(T):
        cuts = [-1] + [i for i, t in enumerate(T) if t[0] == 2] + [len(T)]
        return T[:cuts[iv] + 1] + list(new) + T[cuts[iv + 1]:]
    return f


def chain(*fs):
    def f(T):
        for g in fs:
            T = g(T)
        return T
    return f


def split_ecs(ecs):
    """Entropy-coded bytes of a scan -> [interval bytes], [RSTn marker bytes between them]."""
    ivs = []; marks = []; cur = bytearray(); i = 0
    while i < len(ecs):
        if ecs[i] == 0xFF and i + 1 < len(ecs) and 0xD0 <= ecs[i + 1] <= 0xD7:
            ivs.append(bytes(cur)); marks.append(bytes(ecs[i:i + 2])); cur = bytearray(); i += 2
        else:
            cur.append(ecs[i]); i += 1
    ivs.append(bytes(cur))
    return ivs, marks


def join_ecs(ivs, marks):
    out = bytearray()
    for i, d in enumerate(ivs):
        out += d
        if i < len(marks):
            out += marks[i]
    return bytes(out)


def with_scan(script, index, **hooks):
    out = [dict(P._norm_scan(s)) for s in script]
    out[index].update(hooks)
    return out


# ------------------------------------------------------------------------------------------------------------ frames and coefficients
def grey(w=32, h=24):
    return P.Frame(w, h, [(1, 1, 0)], {0: ONES})


def colour(w=48, h=32):
    return P.Frame(w, h, [(2, 2, 0), (1, 1, 1), (1, 1, 1)], {0: ONES, 1: ONES})


def regular(fr, k6=0, band=None):
    """Every block alike in what the encoder makes of it.  DC: never the value of the block before (one DC symbol with value bits per
    block).  Band 1..6 under a first scan with Al = 1 and a refinement to Al = 0: k1 = 7 and k2 = -5 have history (3 and -2) and
    take correction bits 1 and 1, k3 = 1 and k5 = -1 are new in the refinement, k4 and k6 are zero (k6 = 7 on request: history
    behind the last new coefficient).  First scan: symbols (0,2) (0,2) EOB0 [with k6: (0,2) (0,2) (3,2)] per block; refinement:
    (0,1) (1,1) EOB0 per block, two correction bits behind the first.  k10 = 3 in every block belongs to another scan."""
    co = fr.zeros()
    for c, a in enumerate(co):
        ny, nx = a.shape[:2]
        u = np.arange(ny * nx).reshape(ny, nx)
        a[..., 0] = 40 + 23 * (u % 7) - 9 * (u % 3) + 100 * c + np.where(u % 2, -300, 0)
        a[..., 1] = 7; a[..., 2] = -5; a[..., 3] = 1; a[..., 5] = -1; a[..., 6] = k6; a[..., 10] = 3
        if band:
            for k, v in band.items():
                a[..., k] = v
    return co


def std_script(dri=4, se=6):
    """DC, AC first 1..se at Al 1, the rest of the band, refinement of 1..se."""
    return [S(0, 0, 0, 0, 0, dri=dri), S(0, 1, se, 0, 1), S(0, se + 1, 63, 0, 0), S(0, 1, se, 1, 0)]


POS = (("first", 0), ("middle", 1), ("last", 3))               # a block of interval 1 (units 4..7 of the grey frame, restart interval 4)
CASES = []                                                     # (name, constructor): nothing is built to learn a name


def case(fn):
    CASES.append((fn.__name__, fn))
    return fn


def add(name, fn):
    CASES.append((name, fn))


def has_stop(scan, iv, unit, reason):
    def check(c):
        assert (iv, unit, reason) in c.dec.scans[scan]["stops"], c.record()
        assert c.dec.flagged
    return check


def blk(c, coefs, unit, comp=0):
    nby, nbx = c.frame.coded(comp)
    return coefs[comp][unit // nbx, unit % nbx]


# ================================================================================================================ stops
def _stop_ac_first(pos, j, m):
    name = "stop_ac_first_no_code_%s_block_%s" % (pos, "after_a_stored_symbol" if m else "fresh")
    fr = grey(); sc = with_scan(std_script()[:3], 1, tokens=edit(1, 3 * j + m, NO_CODE))       # (no refinement: the first scan's stores show as they are)
    def check(c):
        has_stop(1, 1, 4 + j, "no_code")(c)
        for u in range(12):                                        # k1 = 3 << 1, k2 = -2 << 1 up to the stop; behind it nothing, the other intervals in full
            want = [6, -4] if not 4 + j <= u < 8 else [6, 0] if (u == 4 + j and m) else [0, 0]
            assert [int(x) for x in blk(c, c.truth, u)[1:3]] == want, (u, c.record())
    return DCase(name, "stop", fr, regular(fr), sc, check)


@case
def stop_ac_first_then_a_refinement_over_the_hole():
    """The refinement scan behind a stopped first scan reads ITS stream against a history that is not the encoder's: what it does to
    units 5..7 is whatever the rules make of it (new values where corrections were meant), the same in every decoder."""
    fr = grey(); sc = with_scan(std_script(), 1, tokens=edit(1, 3 * 1 + 1, NO_CODE))
    def check(c):
        has_stop(1, 1, 5, "no_code")(c)
        assert [int(x) for x in blk(c, c.truth, 4)[1:7]] == [7, -5, 1, 0, -1, 0] and [int(x) for x in blk(c, c.truth, 8)[1:7]] == [7, -5, 1, 0, -1, 0]
        assert [int(x) for x in blk(c, c.truth, 6)[1:7]] != [7, -5, 1, 0, -1, 0]
    return DCase("stop_ac_first_then_a_refinement_over_the_hole", "stop", fr, regular(fr), sc, check)


def _stop_run_past(pos, j, at_se):
    se = 3 if at_se else 4
    name = "stop_ac_first_run_past_se_at_k_%s_%s_block" % ("se" if at_se else "se_minus_1", pos)
    fr = grey(); script = [S(0, 0, 0, 0, 0, dri=4), S(0, 1, se, 0, 1), S(0, se + 1, 63, 0, 0)]
    # after k1 and k2 the position is k = 3: the EOB0 becomes a symbol whose run ends one past Se
    sc = with_scan(script, 1, tokens=edit(1, 3 * j + 2, [(0, 0, ((se - 2) << 4) | 1), (1, 1, 1)]))
    def check(c):
        has_stop(1, 1, 4 + j, "run_past_se")(c)
        b = blk(c, c.truth, 4 + j)
        assert (int(b[1]), int(b[2])) == (6, -4)                                       # the two symbols in front of the stop stay
    # (in the last block of the interval the bad symbol stands where the EOB0 stood: nothing is lost but the flag is set)
    return DCase(name, "stop", fr, regular(fr), sc, check, same_as_clean=j == 3)


def _stop_dc_grey(pos, j, reason):
    name = "stop_dc_%s_%s_block" % (reason, pos)
    fr = grey(); new = NO_CODE if reason == "no_code" else [(0, 0, 16)]
    sc = with_scan(std_script(), 0, tokens=edit(1, j, new))
    def check(c):
        has_stop(0, 1, 4 + j, reason)(c)
        for u in range(4, 8):
            assert int(blk(c, c.truth, u)[0]) == (int(blk(c, c.coefs, u)[0]) if u < 4 + j else 0), (u, c.record())
        assert int(blk(c, c.truth, 8)[0]) == int(blk(c, c.coefs, 8)[0])
    return DCase(name, "stop", fr, regular(fr), sc, check)


MCU_BLOCK = ((0, "first"), (1, "second"), (3, "fourth"))        # luma blocks (v, h) = (0, 0), (0, 1), (1, 1) of a 4:2:0 MCU


def _stop_dc_mcu(pos, j, reason, nb):
    """Interleaved 4:2:0 DC scan, restart interval 3 (MCUs 3..5 are interval 1): the stop is in luma block `nb` of the MCU -- the
    blocks in front of it stay, EVERY block behind it in the MCU keeps its zero (in blocks 0 and 1 the stop is in the first row of
    the component's 2 x 2: a decoder that leaves only the row's loop goes on into the second)."""
    name = "stop_dc_interleaved_%s_%s_mcu_%s_block" % (reason, pos, dict(MCU_BLOCK)[nb])
    fr = colour(); new = NO_CODE if reason == "no_code" else [(0, 0, 17)]
    script = [S([0, 1, 2], 0, 0, 0, 0, dri=3), S(0, 1, 63, 0, 0), S(1, 1, 63, 0, 0), S(2, 1, 63, 0, 0)]
    jj = {0: 0, 1: 1, 3: 2}[j]
    sc = with_scan(script, 0, tokens=edit(1, 6 * jj + nb, new))
    def check(c):
        has_stop(0, 1, 3 + jj, reason)(c)
        my, mx = divmod(3 + jj, fr.mcu_x)
        got = [int(c.truth[0][my * 2 + y, mx * 2 + x, 0]) for y in range(2) for x in range(2)]
        want = [int(c.coefs[0][my * 2 + y, mx * 2 + x, 0]) for y in range(2) for x in range(2)]
        assert all(want) and got == want[:nb] + [0] * (4 - nb) and int(c.truth[1][my, mx, 0]) == 0 and int(c.truth[2][my, mx, 0]) == 0, (got, want)
        for u in range(3 + jj + 1, 6):                             # the MCUs behind it in the interval: untouched
            my, mx = divmod(u, fr.mcu_x)
            assert not c.truth[0][my * 2:my * 2 + 2, mx * 2:mx * 2 + 2, 0].any()
    return DCase(name, "stop", fr, regular(fr), sc, check)


def _stop_refine(pos, j, m, reason):
    name = "stop_refinement_%s_%s_block_%s" % (reason, pos, "after_corrections_and_a_new_value" if m else "fresh")
    fr = grey(); new = NO_CODE if reason == "no_code" else [(0, 0, 0x12)]
    sc = with_scan(std_script(), 3, tokens=edit(1, 3 * j + m, new))
    def check(c):
        has_stop(3, 1, 4 + j, reason)(c)
        b = [int(x) for x in blk(c, c.truth, 4 + j)[1:7]]
        # fresh: what the first scan left (6, -4); after the first symbol: both corrections made (7, -5) and the new value at k3
        assert b == ([7, -5, 1, 0, 0, 0] if m else [6, -4, 0, 0, 0, 0]), (b, c.record())
        if j < 3:
            assert [int(x) for x in blk(c, c.truth, 5 + j)[1:7]] == [6, -4, 0, 0, 0, 0]    # behind the stop: untouched
        assert [int(x) for x in blk(c, c.truth, 8)[1:7]] == [7, -5, 1, 0, -1, 0]           # the next interval: in full
    return DCase(name, "stop", fr, regular(fr), sc, check)


for _pos, _j in POS:
    for _m in (0, 1):
        add("stop_ac_first_no_code_%s_block_%s" % (_pos, "after_a_stored_symbol" if _m else "fresh"), lambda p=_pos, j=_j, m=_m: _stop_ac_first(p, j, m))
    for _at in (True, False):
        add("stop_ac_first_run_past_se_at_k_%s_%s_block" % ("se" if _at else "se_minus_1", _pos), lambda p=_pos, j=_j, a=_at: _stop_run_past(p, j, a))
    for _why in ("no_code", "dc_category"):
        add("stop_dc_%s_%s_block" % (_why, _pos), lambda p=_pos, j=_j, w=_why: _stop_dc_grey(p, j, w))
        for _nb, _nbname in MCU_BLOCK:
            add("stop_dc_interleaved_%s_%s_mcu_%s_block" % (_why, _pos, _nbname), lambda p=_pos, j=_j, w=_why, n=_nb: _stop_dc_mcu(p, j, w, n))
    for _why in ("no_code", "refine_s"):
        for _m in (0, 1):
            add("stop_refinement_%s_%s_block_%s" % (_why, _pos, "after_corrections_and_a_new_value" if _m else "fresh"),
                lambda p=_pos, j=_j, m=_m, w=_why: _stop_refine(p, j, m, w))


# =========================================================================================================== accepted irregularities
WIDE = ("accepted_dc_category_12_al0", "accepted_dc_category_15_wraps_al0", "accepted_dc_category_13_wraps_al3", "accepted_dc_category_15_wraps_al3")


def _dc_wide(name, cat, diff, al):
    """The DC symbol of unit 5 (second block of interval 1) becomes category `cat` with difference `diff`; the blocks behind it in
    the interval carry the offset along."""
    fr = grey(); co = regular(fr)
    for a in co:
        a[..., 0] &= ~np.int16((1 << al) - 1)                       # (no bits below the point transform: the stores show whole)
    script = [S(0, 0, 0, 0, al, dri=4), S(0, 1, 63, 0, 0)]
    sc = with_scan(script, 0, tokens=edit(1, 1, [(0, 0, cat), (1, diff if diff >= 0 else diff - 1, cat)], drop=2))
    def check(c):
        assert (1, 5, "dc_wide") in c.dec.scans[0]["irregular"] and not c.dec.flagged, c.record()
        pred = int(blk(c, c.coefs, 4)[0]) >> al
        for u in (5, 6, 7):
            pred += diff if u == 5 else (int(blk(c, c.coefs, u)[0]) >> al) - (int(blk(c, c.coefs, u - 1)[0]) >> al)
            assert int(blk(c, c.truth, u)[0]) == P._w16(pred * (1 << al)), (u, c.record())
        wrapped = not -32768 <= (((int(blk(c, c.coefs, 4)[0]) >> al) + diff) << al) <= 32767
        assert wrapped == ("wraps" in name)
    return DCase(name, "accepted", fr, co, sc, check)


add(WIDE[0], lambda: _dc_wide(WIDE[0], 12, 2500, 0))
add(WIDE[1], lambda: _dc_wide(WIDE[1], 15, 32767, 0))
add(WIDE[2], lambda: _dc_wide(WIDE[2], 13, -7000, 3))
add(WIDE[3], lambda: _dc_wide(WIDE[3], 15, 32000, 3))


def _same_as_clean(c):
    assert all(np.array_equal(a, b) for a, b in zip(c.truth, c.clean.coefs)), "the irregular file must decode to what the regular one holds"


@case
def accepted_zrl_out_of_the_band_ac_first():
    fr = grey(); sc = with_scan(std_script(), 1, tokens=edit(1, 3 * 1 + 2, [(0, 0, 0xF0)]))
    def check(c):
        assert (1, 5, "zrl_out") in c.dec.scans[1]["irregular"] and not c.dec.flagged, c.record()
        _same_as_clean(c)
    return DCase("accepted_zrl_out_of_the_band_ac_first", "accepted", fr, regular(fr), sc, check, same_as_clean=True)


def _zrl_refine(name, k6):
    fr = grey(); sc = with_scan(std_script(), 3, tokens=edit(1, 3 * 1 + 2, [(0, 0, 0xF0)]))
    def check(c):
        assert (1, 5, "zrl_out") in c.dec.scans[3]["irregular"] and not c.dec.flagged, c.record()
        _same_as_clean(c)
        assert int(blk(c, c.truth, 5)[6]) == k6
    return DCase(name, "accepted", fr, regular(fr, k6=k6), sc, check, same_as_clean=True)


add("accepted_zrl_out_of_the_band_refinement", lambda: _zrl_refine("accepted_zrl_out_of_the_band_refinement", 0))
add("accepted_zrl_out_of_the_band_refinement_over_history", lambda: _zrl_refine("accepted_zrl_out_of_the_band_refinement_over_history", 7))


def _run_out(name, k6):
    """The (1, 1) symbol that would put -1 on k5 of unit 5 asks for three zeros more than the band has left: its correction bits are
    spent (with k6 = 7: the one of k6), the new value is dropped; the block's EOB0 is taken out, the block has ended."""
    fr = grey(); sc = with_scan(std_script(), 3, tokens=edit(1, 3 * 1 + 1, [(0, 0, 0x31), (1, 0, 1)], drop=3))
    def check(c):
        assert (1, 5, "run_out") in c.dec.scans[3]["irregular"] and not c.dec.flagged, c.record()
        want = [a.copy() for a in c.clean.coefs]; blk(c, want, 5)[5] = 0
        assert all(np.array_equal(a, b) for a, b in zip(c.truth, want))
        assert [int(x) for x in blk(c, c.truth, 5)[1:7]] == [7, -5, 1, 0, 0, k6]
    return DCase(name, "accepted", fr, regular(fr, k6=k6), sc, check)


add("accepted_refinement_run_longer_than_the_zeros_left", lambda: _run_out("accepted_refinement_run_longer_than_the_zeros_left", 0))
add("accepted_refinement_run_longer_than_the_zeros_left_over_history", lambda: _run_out("accepted_refinement_run_longer_than_the_zeros_left_over_history", 7))


@case
def accepted_correction_bit_on_a_set_bit():
    """A first scan at Al 0 under a refinement to Al 1: every coefficient has history, the encoder writes a correction bit 1 for 6, 7,
    -6 and -7 (bit 1 of magnitude >> 1 ... = 3), the decoder finds bit 1 of the two's complement value set in 6, 7 and -6 and leaves
    them; -7 (...11111001) has it clear and moves to -9.  4 and 5 get a correction bit 0."""
    fr = grey(); co = regular(fr, band={1: 6, 2: 7, 3: -6, 4: -7, 5: 4, 6: 5})
    script = [S(0, 0, 0, 0, 0, dri=4), S(0, 1, 6, 0, 0), S(0, 7, 63, 0, 0), S(0, 1, 6, 2, 1)]
    def check(c):
        assert sum(1 for _iv, u, w in c.dec.scans[3]["irregular"] if w == "bit_set" and u == 5) == 3 and not c.dec.flagged, c.record()
        assert [int(x) for x in blk(c, c.truth, 5)[1:7]] == [6, 7, -6, -9, 4, 5]
    return DCase("accepted_correction_bit_on_a_set_bit", "accepted", fr, co, script, check, same_as_clean=True)      # (the file IS its own clean form: the script is the irregularity)


@case
def accepted_eobrun_32767_in_an_interval_of_3():
    fr = grey(); script = [S(0, 0, 0, 0, 0, dri=3), S(0, 1, 6, 0, 1), S(0, 7, 63, 0, 0)]
    sc = with_scan(script, 1, tokens=whole_interval(1, [(0, 0, 0xE0), (1, 0x3FFF, 14)]))
    def check(c):
        assert (1, 5, "eobrun_cut") in c.dec.scans[1]["irregular"] and not c.dec.flagged, c.record()
        for u in range(12):
            assert int(blk(c, c.truth, u)[1]) == (0 if 3 <= u < 6 else 6), u
    return DCase("accepted_eobrun_32767_in_an_interval_of_3", "accepted", fr, regular(fr), sc, check)


@case
def accepted_component_named_twice_in_a_dc_scan():
    """T.81 forbids it, the parser takes it: the second naming codes the same blocks again with a predictor of its own."""
    fr = colour(); script = [S([0, 0], 0, 0, 0, 0, dri=2), S([1, 2], 0, 0, 0, 0), S(0, 1, 63, 0, 0), S(1, 1, 63, 0, 0), S(2, 1, 63, 0, 0)]
    def check(c):
        assert c.dec.scans[0]["comps"] == [0, 0] and not c.dec.flagged
        assert all(np.array_equal(a, b) for a, b in zip(c.truth, c.coefs))
    return DCase("accepted_component_named_twice_in_a_dc_scan", "accepted", fr, regular(fr), script, check, same_as_clean=True)


@case
def accepted_dc_scan_of_two_components():
    fr = colour(); script = [S([0, 2], 0, 0, 0, 1, dri=2), S(1, 0, 0, 0, 0), S([2, 0], 0, 0, 1, 0), S(0, 1, 63, 0, 0), S(1, 1, 63, 0, 0), S(2, 1, 63, 0, 0)]
    def check(c):
        assert c.dec.scans[0]["comps"] == [0, 2] and c.dec.scans[2]["comps"] == [2, 0] and not c.dec.flagged
        assert all(np.array_equal(a, b) for a, b in zip(c.truth, c.coefs))
    return DCase("accepted_dc_scan_of_two_components", "accepted", fr, regular(fr), script, check, same_as_clean=True)


# ============================================================================================================ data that runs out
def overran(scan, iv, unit=None, what=None):
    def check(c):
        hit = [(i, u, w) for i, u, w in c.dec.scans[scan]["overran"] if i == iv]
        assert hit and (unit is None or hit[0][1] == unit) and (what is None or hit[0][2] == what), c.record()
        assert c.dec.flagged
    return check


def zero_is_category_0(f):
    """A DC table whose one-bit code 0 is category 0: an interval that reads zeros decodes differences of 0 (and its truth stays within
    what the baseline writer codes)."""
    return P.ladder_table([0] + sorted(s for s in f if s != 0))


def _emptied(name, scan):
    def empty(ecs):
        ivs, marks = split_ecs(ecs); ivs[1] = b""
        return join_ecs(ivs, marks)
    fr = grey()
    return DCase(name, "runout", fr, regular(fr), with_scan(std_script(), scan, bytes=empty, dc_tab=[zero_is_category_0]), overran(scan, 1, 4), flagged=True)


add("runout_interval_emptied_dc", lambda: _emptied("runout_interval_emptied_dc", 0))
add("runout_interval_emptied_ac_first", lambda: _emptied("runout_interval_emptied_ac_first", 1))
add("runout_interval_emptied_refinement", lambda: _emptied("runout_interval_emptied_refinement", 3))


def long_codes(f):
    return P.flat_table(sorted(f), 12)


@case
def runout_cut_inside_a_code():
    """Every AC code has 12 bits: a cut that takes 1..8 bits off the end of the second symbol of unit 5 is inside that code."""
    fr = grey(); sc = with_scan(std_script(), 1, ac_tab=long_codes, tokens=edit(1, 3 * 1 + 1, [(3, 1, 0)], drop=0, after=1))
    return DCase("runout_cut_inside_a_code", "runout", fr, regular(fr), sc, overran(1, 1, 5, "code"), flagged=True)


@case
def runout_cut_inside_value_bits():
    """DC differences of -300 and so on: nine value bits, the cut takes 1..8 of them."""
    fr = grey(); sc = with_scan(std_script(), 0, tokens=edit(1, 1, [(3, 1, 0)], drop=0, after=2))
    def check(c):
        overran(0, 1, 5, "value")(c)
        assert abs(int(blk(c, c.coefs, 5)[0]) - int(blk(c, c.coefs, 4)[0])) >= 256
    return DCase("runout_cut_inside_value_bits", "runout", fr, regular(fr), sc, check, flagged=True)


@case
def runout_cut_inside_a_correction_stretch():
    """k1..k16 have history, k17 is new: the first refinement symbol of a block is followed by its sign and 16 correction bits."""
    fr = grey(); band = {k: (7 if k % 2 else -5) for k in range(1, 17)}; band.update({17: 1, 18: 0, 19: 0, 20: 0})
    co = regular(fr, band=band)
    script = [S(0, 0, 0, 0, 0, dri=4), S(0, 1, 20, 0, 1), S(0, 21, 63, 0, 0), S(0, 1, 20, 1, 0)]
    def cut(T):
        i = sym_at(T, 1, 2 * 1)                                    # unit 5: symbol, sign, 16 correction bits
        assert T[i][2] == 0x01 and all(t == (1, 1, 1) for t in T[i + 2:i + 18]) and T[i + 18][0] != 1, T[i:i + 20]
        return T[:i + 18] + [(3, 1, 0)] + T[i + 18:]
    return DCase("runout_cut_inside_a_correction_stretch", "runout", fr, co, with_scan(script, 3, tokens=cut), overran(3, 1, 5, "correction"), flagged=True)


@case
def runout_cut_inside_an_eobn_length_field():
    fr = grey(); script = [S(0, 0, 0, 0, 0, dri=3), S(0, 1, 6, 0, 1), S(0, 7, 63, 0, 0)]
    sc = with_scan(script, 1, tokens=whole_interval(1, [(0, 0, 0xE0), (1, 0x3FFF, 14), (3, 1, 0)]))
    def check(c):
        overran(1, 1, 3, "eob_length")(c)
        assert not c.dec.scans[1]["stops"]
    return DCase("runout_cut_inside_an_eobn_length_field", "runout", fr, regular(fr), sc, check, flagged=True)


def _cut_file(scan, where):
    """post hook: the file ends inside scan `scan` ('middle' of its entropy-coded bytes, never behind an FF) or in front of its
    second RSTn ('rst')."""
    def post(c):
        s = P.decode(c.file).scans[scan]
        if where == "rst":
            return c.file[:s["intervals"][1][1]]
        q = (s["start"] + s["end"]) // 2
        while c.file[q - 1] == 0xFF:
            q -= 1
        return c.file[:q]
    return post


@case
def runout_file_cut_inside_scan_1():
    fr = grey()
    def check(c):
        assert len(c.dec.scans) == 2 and c.dec.scans[1]["missing"] >= 1 and c.dec.flagged, c.record()
    return DCase("runout_file_cut_inside_scan_1", "runout", fr, regular(fr), std_script(), check, post=_cut_file(1, "middle"), flagged=True)


@case
def runout_file_cut_inside_the_last_scan():
    fr = grey()
    def check(c):
        assert len(c.dec.scans) == 4 and c.dec.scans[3]["missing"] >= 1 and c.dec.flagged, c.record()
    return DCase("runout_file_cut_inside_the_last_scan", "runout", fr, regular(fr), std_script(), check, post=_cut_file(3, "middle"), flagged=True)


@case
def runout_file_cut_inside_the_last_scan_no_restarts():
    fr = grey()
    def check(c):
        assert len(c.dec.scans) == 4 and not c.dec.scans[3]["missing"] and c.dec.scans[3]["overran"] and c.dec.flagged, c.record()
    return DCase("runout_file_cut_inside_the_last_scan_no_restarts", "runout", fr, regular(fr), std_script(dri=0), check, post=_cut_file(3, "middle"), flagged=True)


@case
def runout_file_cut_exactly_at_an_rstn():
    """Two whole intervals of the last scan, then nothing: no interval stops or overruns, a third of the picture was never coded --
    the flag comes from the count of intervals alone."""
    fr = grey()
    def check(c):
        s = c.dec.scans[3]
        assert s["missing"] == 1 and not s["stops"] and not s["overran"] and c.dec.flagged, c.record()
        assert [int(x) for x in blk(c, c.truth, 7)[1:7]] == [7, -5, 1, 0, -1, 0] and [int(x) for x in blk(c, c.truth, 8)[1:7]] == [6, -4, 0, 0, 0, 0]
    return DCase("runout_file_cut_exactly_at_an_rstn", "runout", fr, regular(fr), std_script(), check, post=_cut_file(3, "rst"), flagged=True)


def _rst(name, scan, fn, check, flagged, **kw):
    fr = grey()
    def hook(ecs):
        ivs, marks = split_ecs(ecs); ivs, marks = fn(list(ivs), list(marks))
        return join_ecs(ivs, marks)
    return DCase(name, "runout", fr, regular(fr), with_scan(std_script(), scan, bytes=hook, **kw), check, flagged=flagged)


@case
def runout_last_rstn_deleted():
    """Intervals 1 and 2 of the AC first scan fuse: interval 1 decodes its own four blocks, what follows is never read; interval 2
    is missing."""
    def check(c):
        s = c.dec.scans[1]
        assert s["missing"] == 1 and not s["stops"] and not s["overran"] and c.dec.flagged, c.record()
    return _rst("runout_last_rstn_deleted", 1, lambda ivs, m: (ivs[:1] + [ivs[1] + ivs[2]], m[:1]), check, True)


@case
def runout_last_rstn_deleted_dc():
    """The same in the DC scan, whose fused interval DOES go on: the first interval takes the second one's bytes for its own (the
    padding ones in between shift every code)."""
    def check(c):
        s = c.dec.scans[0]
        assert s["missing"] == 1 and c.dec.flagged, c.record()
    return _rst("runout_last_rstn_deleted_dc", 0, lambda ivs, m: ([ivs[0] + ivs[1], ivs[2]], m[:1]), check, True)


@case
def runout_surplus_rstn_in_the_middle():
    """An RSTn too many behind interval 0 of the refinement scan: interval 1 is empty, interval 2 gets the data of interval 1, the
    data of interval 2 is surplus."""
    def check(c):
        s = c.dec.scans[3]
        assert s["surplus"] == 1 and (1, 4, "code") in s["overran"] and c.dec.flagged, c.record()
    return _rst("runout_surplus_rstn_in_the_middle", 3, lambda ivs, m: (ivs[:1] + [b""] + ivs[1:], m[:1] + [b"\xFF\xD7"] + m[1:]), check, True)


@case
def runout_surplus_rstn_at_the_end():
    def check(c):
        assert c.dec.scans[1]["surplus"] == 1 and not c.dec.flagged, c.record()
        _same_as_clean(c)
    c = _rst("runout_surplus_rstn_at_the_end", 1, lambda ivs, m: (ivs + [b""], m + [b"\xFF\xD3"]), check, False)
    c.same_as_clean = True
    return c


@case
def runout_fill_bytes_before_an_rstn():
    def check(c):
        assert not c.dec.flagged and c.file.count(b"\xFF\xFF\xFF\xD0") == 1, c.record()
        _same_as_clean(c)
    c = _rst("runout_fill_bytes_before_an_rstn", 1, lambda ivs, m: (ivs, [b"\xFF\xFF" + m[0]] + m[1:]), check, False)
    c.same_as_clean = True
    return c


@case
def runout_fill_bytes_behind_a_cut_interval():
    """A DC refinement scan (one bit per block, 8 blocks per interval, every bit 0): interval 1 is emptied and three fill bytes stand in
    front of the RSTn behind it.  Its reader runs on through where the fill bytes are and must get zero bits there, not ones: the
    coefficients stay as they are, the file is flagged."""
    fr = grey(64, 32); co = regular(fr)
    co[0][..., 0] &= ~np.int16(1)
    script = [S(0, 0, 0, 0, 1, dri=8), S(0, 1, 63, 0, 0), S(0, 0, 0, 1, 0)]
    def hook(ecs):
        ivs, marks = split_ecs(ecs)
        assert ivs == [b"\x00"] * 4, ivs
        ivs[1] = b""; marks[1] = b"\xFF\xFF\xFF" + marks[1]
        return join_ecs(ivs, marks)
    def check(c):
        assert c.dec.scans[2]["overran"] == [(1, 8, "dc_bit")] and c.dec.flagged, c.record()
        _same_as_clean(c)
    return DCase("runout_fill_bytes_behind_a_cut_interval", "runout", fr, co, with_scan(script, 2, bytes=hook), check, flagged=True, same_as_clean=True)


@case
def runout_stuffed_ff_is_the_last_byte_of_a_cut_interval():
    """A DC refinement scan is one bit per block: 16 blocks whose bit is 1 are FF 00 FF 00; the interval is cut to FF 00."""
    fr = grey(64, 32); co = regular(fr)                              # 8 x 4 blocks, restart interval 16
    co[0][..., 0] |= 1
    script = [S(0, 0, 0, 0, 1, dri=16), S(0, 1, 63, 0, 0), S(0, 0, 0, 1, 0)]
    def hook(ecs):
        ivs, marks = split_ecs(ecs)
        assert ivs[1] == b"\xFF\x00\xFF\x00", ivs
        ivs[1] = b"\xFF\x00"
        return join_ecs(ivs, marks)
    def check(c):
        assert (1, 24, "dc_bit") in c.dec.scans[2]["overran"] and c.dec.flagged, c.record()
        assert int(blk(c, c.truth, 23)[0]) & 1 == 1 and int(blk(c, c.truth, 24)[0]) & 1 == 0
    return DCase("runout_stuffed_ff_is_the_last_byte_of_a_cut_interval", "runout", fr, co, with_scan(script, 2, bytes=hook), check, flagged=True)


@case
def runout_file_ends_in_an_ff_that_is_data():
    """The last scan is a DC refinement of 32 blocks whose bit is 1: FF 00 FF 00, RSTn, FF 00 FF 00.  The file is cut behind the very
    last FF: no marker follows it, so it is no fill byte and no half marker but the data byte FF -- blocks 24..31 get their bit, no
    interval overruns, the file is not flagged.  (A reader that dropped the byte would starve the interval.)"""
    fr = grey(64, 32); co = regular(fr)
    co[0][..., 0] |= 1
    script = [S(0, 0, 0, 0, 1, dri=16), S(0, 1, 63, 0, 0), S(0, 0, 0, 1, 0)]
    def post(c):
        assert c.file.endswith(b"\xFF\x00\xFF\x00\xFF\xD9")
        return c.file[:-3]
    def check(c):
        assert c.file.endswith(b"\x00\xFF") and len(c.dec.scans) == 3 and not c.dec.scans[2]["overran"] and not c.dec.flagged, c.record()
        _same_as_clean(c)
    return DCase("runout_file_ends_in_an_ff_that_is_data", "runout", fr, co, script, check, post=post, flagged=False, same_as_clean=True)


# ===================================================================================================================== seams
def seam_frame():
    return grey(160, 128)                                            # 20 x 16 blocks; restart interval 1: 320 intervals per scan


SEAM_SCANS = (("dc", 0, 1), ("ac_first", 1, 3), ("refinement", 3, 3))           # name, scan index, symbols per block


def _seam(kind, scan, iv):
    fr = seam_frame()
    sc = with_scan(std_script(dri=1), scan, tokens=edit(iv, 0, NO_CODE))
    return DCase("seam_%s_interval_%d" % (kind, iv), "seam", fr, regular(fr), sc, has_stop(scan, iv, iv, "no_code"), flagged=True)


PAIR = (70, 71)                                                 # one wave whatever the form: iv // per is the same for per = 2, 4, 8, 16 (intervals per wave) and 64 (lanes)
assert all(PAIR[0] // per == PAIR[1] // per for per in (2, 4, 8, 16, 64))


def _seam_pair(kind, scan):
    """Two bad intervals that share a wave in every form that puts more than one interval into a wave: neighbours inside one aligned
    pair.  The first stops at its first symbol, the second is empty and overruns; the intervals around them decode in full."""
    fr = seam_frame(); a, b = PAIR
    def empty(ecs):
        ivs, marks = split_ecs(ecs); ivs[b] = b""
        return join_ecs(ivs, marks)
    def check(c):
        s = c.dec.scans[scan]
        assert (a, a, "no_code") in s["stops"] and [x for x in s["overran"] if x[0] == b], c.record()
        assert not [x for x in s["stops"] + s["overran"] if x[0] not in PAIR], c.record()
        for u in (a - 1, b + 1):
            assert np.array_equal(blk(c, c.truth, u), blk(c, c.clean.coefs, u)), u
    return DCase("seam_%s_two_bad_intervals_in_one_wave" % kind, "seam", fr, regular(fr), with_scan(std_script(dri=1), scan, tokens=edit(a, 0, NO_CODE), bytes=empty),
                 check, flagged=True)


for _kind, _scan, _n in SEAM_SCANS:
    for _iv in SEAMS:
        add("seam_%s_interval_%d" % (_kind, _iv), lambda k=_kind, s=_scan, i=_iv: _seam(k, s, i))
    add("seam_%s_two_bad_intervals_in_one_wave" % _kind, lambda k=_kind, s=_scan: _seam_pair(k, s))


def _seam_mcu(nb, nbname):
    fr = colour(320, 256)                                            # 20 x 16 MCUs
    script = [S([0, 1, 2], 0, 0, 0, 0, dri=1), S(0, 1, 63, 0, 0, dri=0)]
    sc = with_scan(script, 0, tokens=edit(64, nb, [(0, 0, 16)]))
    def check(c):
        has_stop(0, 64, 64, "dc_category")(c)
        my, mx = divmod(64, fr.mcu_x)
        got = [int(c.truth[0][my * 2 + y, mx * 2 + x, 0]) for y in range(2) for x in range(2)]
        want = [int(c.coefs[0][my * 2 + y, mx * 2 + x, 0]) for y in range(2) for x in range(2)]
        assert all(want) and got == want[:nb] + [0] * (4 - nb), (got, want)
        assert len(c.file) < 20000
    return DCase("seam_interleaved_dc_420_interval_64_%s_block" % nbname, "seam", fr, regular(fr), sc, check, flagged=True)


for _nb, _nbname in MCU_BLOCK:
    add("seam_interleaved_dc_420_interval_64_%s_block" % _nbname, lambda n=_nb, nn=_nbname: _seam_mcu(n, nn))


# ======================================================================================================================== builds
NAMES = [n for n, _fn in CASES]
assert len(set(NAMES)) == len(NAMES), [n for n in NAMES if NAMES.count(n) > 1]
_BUILT = {}


def built(name):
    if name not in _BUILT:
        c = CASES[NAMES.index(name)][1]().build()
        assert c.name == name, (c.name, name)
        _BUILT[name] = c
    return _BUILT[name]


def build_all():
    return [built(n) for n in NAMES]


# ================================================================================================================ random damage
MUTATIONS = ("flip", "delete", "insert", "truncate", "rst_deleted", "rst_doubled")
# The mix: a flipped or inserted byte mostly changes values without stopping or starving an interval (about a quarter of them are
# flagged), so the kinds that always cost an interval its data are drawn more often.
WEIGHTS = (1, 2, 1, 3, 3, 2)
N_RANDOM = 200
_RANDOM = {}


def _free(ecs, i):
    """Byte i of the entropy-coded bytes is neither part of a marker or of a stuffed FF 00 nor next to an FF: changing it makes or
    breaks no marker (markers are the parser's subject: see the refusal files)."""
    return ecs[i] != 0xFF and (i == 0 or ecs[i - 1] != 0xFF) and (i + 1 >= len(ecs) or ecs[i + 1] != 0xFF)


def mutate(rng, ecs, kind):
    """One mutation of a scan's entropy-coded bytes (RSTn markers included); None where this scan offers no place for it."""
    ecs = bytearray(ecs)
    free = [i for i in range(len(ecs)) if _free(ecs, i)]
    rsts = [i for i in range(len(ecs) - 1) if ecs[i] == 0xFF and 0xD0 <= ecs[i + 1] <= 0xD7]
    if kind in ("rst_deleted", "rst_doubled"):
        if not rsts:
            return None
        i = rsts[int(rng.integers(len(rsts)))]
        return bytes(ecs[:i] + ecs[i + 2:]) if kind == "rst_deleted" else bytes(ecs[:i + 2] + ecs[i:])
    if not free:
        return None
    i = free[int(rng.integers(len(free)))]
    if kind == "flip":
        v = int(ecs[i]) ^ (1 << int(rng.integers(8)))
        if v == 0xFF:
            v ^= 0x81
        ecs[i] = v
        return bytes(ecs)
    if kind == "delete":
        return bytes(ecs[:i] + ecs[i + 1:])
    if kind == "insert":
        return bytes(ecs[:i] + bytes([int(rng.integers(0, 255))]) + ecs[i:])
    return bytes(ecs[:i])                                            # truncate: the tail of the scan's data goes (the next marker follows at once)


class RCase:
    """One randomly damaged file and its lenient truth."""
    owner = DCase.owner; record = DCase.record

    def __init__(self, name, frame, file, clean_file, clean_coefs):
        self.name, self.frame, self.file, self.clean_file = name, frame, file, clean_file
        self.dec = P.decode(file, lenient=True); self.truth = self.dec.coefs; self.flagged = self.dec.flagged
        self.arena = P.arena(frame, self.truth); self.clean_arena = P.arena(frame, clean_coefs)
        try:
            self.base = P.encode_baseline(frame, self.truth)
        except AssertionError:
            self.base = None


def random_damage(n=N_RANDOM, seed=4711):
    """n files: a random legal script over a random frame of at most 48 x 48 (tests/prog_cases.py), then ONE mutation inside the
    entropy-coded bytes of one scan.  No file is skipped: a mutation that finds no place in the scan drawn (no RSTn to delete) is
    drawn again."""
    if (n, seed) in _RANDOM:
        return _RANDOM[(n, seed)]
    rng = np.random.default_rng(seed); out = []
    for k in range(n):
        geo = list(PC.GEOMETRIES)[int(rng.integers(len(PC.GEOMETRIES)))]
        fr = PC.frame_of(geo, int(rng.integers(8, 49)), int(rng.integers(8, 49)))
        co = PC.noise(fr, int(rng.integers(1 << 30)), density=float(rng.choice([0.05, 0.3, 0.8])), amp=int(rng.choice([2, 12, 200])))
        script = PC.random_script(rng, fr.ncomp)
        if not any("dri" in s and s["dri"] for s in script):
            script[0]["dri"] = int(rng.choice([1, 2, 5]))
        clean = P.encode_progressive(fr, co, script)
        whole = P.decode(clean, lenient=True); scans = whole.scans
        assert not whole.flagged
        while True:
            si = int(rng.integers(len(scans))); kind = str(rng.choice(MUTATIONS, p=np.array(WEIGHTS) / sum(WEIGHTS)))
            s = scans[si]
            new = mutate(rng, clean[s["start"]:s["end"]], kind)
            if new is not None and new != clean[s["start"]:s["end"]]:
                break
        c = RCase("damage_%03d_%s_scan_%d_%s_%dx%d" % (k, kind, si, geo, fr.width, fr.height), fr, clean[:s["start"]] + new + clean[s["end"]:], clean, whole.coefs)
        out.append(c)
    _RANDOM[(n, seed)] = out
    return out


# ================================================================================================================ parser refusals
def _parts(f):
    """A file as a list of [marker, payload] segments and [None, entropy-coded bytes] runs, between SOI and EOI."""
    out = []; pos = 2
    while f[pos + 1] != 0xD9:
        m = f[pos + 1]; ln = int.from_bytes(f[pos + 2:pos + 4], "big")
        out.append([m, bytearray(f[pos + 4:pos + 2 + ln])]); pos += 2 + ln
        if m == 0xDA:
            _ivs, end = P._split_intervals_lenient(f, pos)
            out.append([None, bytearray(f[pos:end])]); pos = end
    return out


def _file(parts, eoi=True):
    out = bytearray(b"\xFF\xD8")
    for m, p in parts:
        out += bytes(p) if m is None else bytes([0xFF, m]) + (len(p) + 2).to_bytes(2, "big") + bytes(p)
    return bytes(out + (b"\xFF\xD9" if eoi else b""))


def _first(parts, marker, nth=0):
    return [i for i, (m, _p) in enumerate(parts) if m == marker][nth]


def refusals():
    """[(name, file, substring of jsnoop_last_error)]: one file per refusal branch of the progressive parser, each a well-formed colour
    file with one header field changed."""
    fr = colour(); good = P.encode_progressive(fr, regular(fr), [S([0, 1, 2], 0, 0, 0, 0), S(0, 1, 63, 0, 0), S(1, 1, 63, 0, 0), S(2, 1, 63, 0, 0)])
    out = []

    def add(name, text, fn, **kw):
        parts = _parts(good); r = fn(parts)
        out.append((name, _file(parts if r is None else r, **kw), text))

    def seg(marker, nth=0):
        return lambda parts: parts[_first(parts, marker, nth)][1]

    def poke(marker, off, val, nth=0):
        def fn(parts):
            seg(marker, nth)(parts)[off] = val
        return fn

    def cut_dqt(parts):                                            # the DQT's length says 67 bytes, the file ends after 20 of them
        return parts[:_first(parts, 0xDB)] + [[None, b"\xFF\xDB\x00\x43" + bytes(20)]]
    add("truncated_segment", "truncated marker segment", cut_dqt, eoi=False)
    add("dqt_destination_4", "DQT destination out of range", poke(0xDB, 0, 4))
    add("precision_12", "8-bit precision only", poke(0xC2, 0, 12))
    add("two_components", "2 components", poke(0xC2, 5, 2))
    add("four_components", "4 components", poke(0xC2, 5, 4))
    add("sampling_factor_0", "sampling factor out of range", poke(0xC2, 7, 0x02))
    add("sampling_factor_5", "sampling factor out of range", poke(0xC2, 7, 0x25))
    def sof0(parts):
        i = _first(parts, 0xC2); parts[i][0] = 0xC0
    add("sof0", "not a progressive file (SOF0)", sof0)
    add("dht_class_2", "DHT class/destination out of range", poke(0xC4, 0, 0x20))
    def many_codes(parts):
        p = seg(0xC4)(parts); p[1:17] = bytes([0] * 8 + [40] * 7 + [0]); p[17:] = bytes(280)
    add("dht_more_than_256_codes", "more than 256 codes", many_codes)
    def sos_first(parts):
        i = _first(parts, 0xC2); s = _first(parts, 0xDA)
        return parts[:i] + parts[s:s + 2] + parts[i:s] + parts[s + 2:]
    add("sos_before_sof", "SOS before SOF2", sos_first)
    add("ns_0", "SOS with 0 components", poke(0xDA, 0, 0))
    add("unknown_component", "unknown component 9", poke(0xDA, 1, 9))
    n1 = 1 + 2 * 1                                                 # offset of Ss in the SOS of a one-component scan (the second SOS), 1 + 2 * 3 in the first
    def ss_above_se(parts):
        poke(0xDA, n1, 5, nth=1)(parts); poke(0xDA, n1 + 1, 4, nth=1)(parts)
    add("scan_ss_above_se", "illegal progressive scan parameters", ss_above_se)
    add("scan_se_64", "illegal progressive scan parameters", poke(0xDA, n1 + 1, 64, nth=1))
    add("scan_al_14", "illegal progressive scan parameters", poke(0xDA, n1 + 2, 14, nth=1))
    add("scan_ss_0_se_5", "illegal progressive scan parameters", poke(0xDA, 1 + 2 * 3 + 1, 5))
    def ac_of_two(parts):                                          # Ss = 1 in the three-component scan
        p = seg(0xDA)(parts); p[0] = 2; del p[5:7]; p[5] = 1; p[6] = 63
    add("scan_ac_of_two_components", "illegal progressive scan parameters", ac_of_two)
    add("huffman_table_undefined", "undefined or malformed Huffman table", poke(0xDA, 2, 0x03, nth=1))     # AC table 3 was never sent
    def oversubscribed(parts):
        i = _first(parts, 0xC4, 3); p = parts[i][1]; assert p[0] >> 4 == 1   # the AC table of the second scan: three codes of one bit
        n = sum(p[1:17]); p[1:17] = bytes([3] + [0] * 15); p[17:] = bytes(range(3)); assert n >= 3
    add("huffman_table_oversubscribed", "undefined or malformed Huffman table", oversubscribed)
    def no_dqt(parts):
        i = _first(parts, 0xC2); parts[i][1][8 + 3] = 2                # Cb selects table 2
    add("dqt_undefined", "undefined quantisation table", no_dqt)
    def no_scans(parts):
        return parts[:_first(parts, 0xDA)]
    add("no_scans", "no SOF2 / no scans", no_scans)
    return good, out
