"""The catalogue behind tests/test_coef_hist_cases.py (CPU) and tests/test_gpu_coef_hist.py (GPU): tiny files for the edges of
jsnoop_batch_pack_coef_hist (k_coef_hist, jpegsnoop_amd/csrc/jsnoop_coef_hist.hip), written block by block with prog_codec.Frame /
encode_baseline / encode_progressive -- the quantised levels of every block are chosen here, the frame writer emits 8- and 16-bit DQT.

A case carries a CLAIM: a function of a `view` (tensor(c), q(c), row(c, R, quantised, zigzag)) that asserts what the rows must hold, derived a
second time in plain Python integers (math on single values, collections.Counter) from the values the view's tensor holds.  The CPU test feeds the
view with the oracle's blocks through coef_hist_model and requires every claim to hold; it then swaps the rows for those of six wrong models and
requires the case named for each to refuse it.

What a file can reach.  An arena value is (int16)(level * q): a multiple of q modulo 2^16.  A baseline AC level is at most 1023 in magnitude, a
DC difference 2047, but the cumulative DC sums differences, so position 0 reaches (int16)(s * q) for any s a walk of differences gets to.  For an
odd q every int16 is reachable (q is invertible modulo 2^16): v = +-(q - 1), +-q, +-(q + 1) for q = 3 and 255 are walked to below.  For an even q only
multiples of gcd(q, 2^16) exist: q = 2 has no v = -1, q = 256 no v = 255.  For q = 65535 every int16 is smaller than the divisor.  Those
combinations no file can hold are the business of the exhaustive sweep of the binning header (tests/cpp/coef_hist_sweep.cpp)."""
from __future__ import annotations

import collections

import numpy as np

import prog_codec as PC

RANGES = (1, 2, 16, 127)
EDGE_INDICES = (0, 1, 7, 8, 62, 63)          # natural indices at the edges of a lane's eight
POSITION = [0] * 64                          # zig-zag position of natural index k
for _z, _n in enumerate(PC.ZIGZAG):
    POSITION[_n] = _z


class Case:
    def __init__(self, name, data, claim, truth_data=None, decode_ac=True, refuses=()):
        self.name, self.data, self.claim, self.decode_ac, self.refuses = name, data, claim, decode_ac, tuple(refuses)
        self.truth_data = data if truth_data is None else truth_data      # a progressive file: its baseline encoding, which the oracle decodes


def trunc_div(v, q):
    v, q = int(v), max(int(q), 1)
    return -(-v // q) if v < 0 else v // q


def expect_position(view, c, R, quantised, zigzag, p, what=""):
    """Position p of the row against a count in Python integers over the tensor's values at the natural index behind p."""
    k = PC.ZIGZAG[p] if zigzag else p
    vals = [int(v) for v in view.tensor(c)[..., k].reshape(-1)]
    q = int(view.q(c)[k])
    xs = [trunc_div(v, q) if quantised else v for v in vals]
    want = collections.Counter(min(max(x, -R), R) + R for x in xs)
    row = view.row(c, R, quantised, zigzag)
    nb = 2 * R + 1
    hist = row[:64 * nb].reshape(64, nb)[p]
    for b in range(nb):
        assert int(hist[b]) == want.get(b, 0), "%s component %d position %d bin %d: got %d, want %d" % (what, c, p, b, int(hist[b]), want.get(b, 0))
    mn, mx = int(row[64 * nb:].view(np.int32)[p]), int(row[64 * nb + 64:].view(np.int32)[p])
    assert (mn, mx) == (min(xs), max(xs)), "%s component %d position %d: min / max got %d / %d, want %d / %d" % (what, c, p, mn, mx, min(xs), max(xs))
    return xs


def _grey(width, height, q_zigzag):
    return PC.Frame(width, height, [(1, 1, 0)], {0: list(q_zigzag)})


def _walk(targets, step=2047):
    """Cumulative DC levels, one per block, that visit every target in turn with differences of at most `step`."""
    out, cur = [], 0
    for t in targets:
        while abs(t - cur) > step:
            cur += step if t > cur else -step
            out.append(cur)
        cur = t
        out.append(cur)
    return out


CASES = []


def _add(fn):
    CASES.append(fn)
    return fn


# ------------------------------------------------------------------------------------------------------------------ clamp edges
def _clamp(R):
    def build():
        vals = [-R - 1, -R, -R + 1, R - 1, R, R + 1]
        fr = _grey(8 * len(vals), 8, [1] * 64); co = fr.zeros()
        for j, v in enumerate(vals):
            for k in EDGE_INDICES:
                co[0][0, j, POSITION[k]] = v
        def claim(view):
            for zz in (False, True):
                for k in EDGE_INDICES:
                    p = POSITION[k] if zz else k
                    xs = expect_position(view, 0, R, True, zz, p, "clamp R=%d" % R)
                    assert sorted(xs) == sorted(vals), (k, xs)
                    h = view.row(0, R, True, zz)[:64 * (2 * R + 1)].reshape(64, -1)[p]
                    assert int(h[0]) == 2 and int(h[2 * R]) == 2, "both end bins saturate: -R - 1 and -R, R and R + 1"
        return Case("clamp_edges_r%d" % R, PC.encode_baseline(fr, co), claim, refuses=("clamp_r_minus_1",) if R == 16 else ())
    build.__name__ = "clamp_edges_r%d" % R
    _add(build)


for _r in RANGES:
    _clamp(_r)


# ------------------------------------------------------------------------------------------------------------------ division edges
def _inverse_mod_2_16(q):
    return pow(q, -1, 65536)


def _signed16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _div_dc(q):
    """Odd q: the cumulative DC walks to the levels s with (int16)(s * q) = +-(q - 1), +-q, +-(q + 1)."""
    def build():
        want_v = [q - 1, -(q - 1), q, -q, q + 1, -(q + 1)]
        levels = _walk([_signed16(v * _inverse_mod_2_16(q)) for v in want_v])
        fr = _grey(8 * len(levels), 8, [q] * 64); co = fr.zeros()
        co[0][0, :, 0] = levels
        def claim(view):
            vals = set(int(v) for v in view.tensor(0)[..., 0].reshape(-1))
            assert set(want_v) <= vals, "the walk reaches every edge value: %s lacks %s" % (sorted(vals), sorted(set(want_v) - vals))
            for R in RANGES:
                expect_position(view, 0, R, True, False, 0, "division by %d" % q)
                expect_position(view, 0, R, False, False, 0, "no division, table of %d" % q)
        return Case("div_edges_dc_q%d" % q, PC.encode_baseline(fr, co), claim, refuses=("floor_div",) if q == 3 else ())
    build.__name__ = "div_edges_dc_q%d" % q
    _add(build)


for _q in (1, 3, 255):
    _div_dc(_q)


@_add
def div_edges_ac_table_of_many_divisors():
    """One 16-bit table with 1, 2, 3, 255, 256, 65535 at zig-zag positions 1..6: levels +-1, +-2 at each, and at the position of 255 the level +-258
    whose product wraps to +-254 = +-(q - 1), +-257 whose product wraps to -+1 (|v| < q), and +-256 whose product wraps to +-256 = +-(q + 1)."""
    qs = [1, 2, 3, 255, 256, 65535]
    qt = [16] * 64
    for z, q in enumerate(qs, start=1):
        qt[z] = q
    lv = [1, -1, 2, -2, 258, -258, 257, -257, 256, -256]
    fr = _grey(8 * len(lv), 8, qt); co = fr.zeros()
    for j, l in enumerate(lv):
        co[0][0, j, 1:7] = l
    def claim(view):
        t = view.tensor(0)
        assert {254, -254, 256, -256} <= set(int(v) for v in t[..., PC.ZIGZAG[4]].reshape(-1)), "255 * 258 wraps to q - 1, 255 * -256 to q + 1"
        assert {1, -1, 2, -2} <= set(int(v) for v in t[..., PC.ZIGZAG[6]].reshape(-1)), "65535 * level = -level"
        for R in (1, 127):
            for z in range(1, 7):
                xs = expect_position(view, 0, R, True, True, z, "table of many divisors")
                if z == 6:
                    assert set(xs) == {0}, "every int16 is smaller than 65535: truncation gives 0, never -1"
    return Case("div_edges_ac_table_of_many_divisors", PC.encode_baseline(fr, co), claim, refuses=())


@_add
def div_table_with_a_zero_entry():
    """A table holding 0 at zig-zag position 2: every product is 0, the divisor counts as 1."""
    qt = [4] * 64; qt[2] = 0
    fr = _grey(24, 8, qt); co = fr.zeros()
    co[0][0, :, 1] = [3, -3, 1]; co[0][0, :, 2] = [5, -5, 9]
    def claim(view):
        assert int(view.q(0)[PC.ZIGZAG[2]]) == 0 and not view.tensor(0)[..., PC.ZIGZAG[2]].any()
        for z in (1, 2):
            expect_position(view, 0, 16, True, True, z, "zero entry")
    return Case("div_table_with_a_zero_entry", PC.encode_baseline(fr, co), claim)


# ------------------------------------------------------------------------------------------------------------------ extrema
@_add
def extrema_through_the_int16_wrap():
    """128 * 256 wraps to -32768 at zig-zag position 1, -99 * 331 = -32769 wraps to 32767 at position 2; position 3 holds only negative values,
    position 4 only positive ones: a record seeded with 0 shows at both."""
    qt = [1] * 64; qt[1] = 256; qt[2] = 331
    fr = _grey(32, 8, qt); co = fr.zeros()
    co[0][0, :, 1] = [128, 1, 0, -1]; co[0][0, :, 2] = [-99, 0, 2, -2]; co[0][0, :, 3] = [-5, -7, -1, -300]; co[0][0, :, 4] = [5, 7, 1, 300]
    def claim(view):
        for quantised in (False, True):
            for z in (1, 2, 3, 4):
                expect_position(view, 0, 127, quantised, True, z, "extrema")
        row = view.row(0, 127, False, True); nb = 255
        mn, mx = row[64 * nb:].view(np.int32), row[64 * nb + 64:].view(np.int32)
        assert int(mn[1]) == -32768 and int(mx[2]) == 32767
        assert int(mx[3]) == -1 and int(mn[4]) == 1, "all negative / all positive: no seed of 0"
    return Case("extrema_through_the_int16_wrap", PC.encode_baseline(fr, co), claim, refuses=("seed_0",))


# ------------------------------------------------------------------------------------------------------------------ position 0
def _dc_ramp(dri, progressive):
    name = "dc_constant_difference_1_%s%s" % ("dri3" if dri else "no_restart", "_progressive" if progressive else "")
    def build():
        fr = PC.Frame(40, 24, [(1, 1, 0)], {0: [1] * 64}); co = fr.zeros()
        n = np.arange(15)
        co[0][:, :, 0] = ((n % dri if dri else n) + 1).reshape(3, 5)
        co[0][:, :, 1] = 2
        base = PC.encode_baseline(fr, co, dri=dri)
        data = PC.encode_progressive(fr, co, [dict(comps=[0], ss=0, se=0, ah=0, al=0, dri=dri), ([0], 1, 63, 0, 0)]) if progressive else base
        def claim(view):
            xs = expect_position(view, 0, 16, True, False, 0, name)
            assert sorted(xs) == sorted(((n % dri if dri else n) + 1).tolist()), "position 0 is the cumulative DC: %s" % xs
        return Case(name, data, claim, truth_data=base, refuses=("arena_slot_0",) if not dri and not progressive else ())
    build.__name__ = name
    _add(build)


for _dri in (0, 3):
    for _p in (False, True):
        _dc_ramp(_dri, _p)


# ------------------------------------------------------------------------------------------------------------------ same address, zeros, order
@_add
def one_value_everywhere_64x64_blocks():
    """Every coefficient of every block is 1: each lane adds to the same bin of its positions in every block, 4096 times in all."""
    fr = _grey(512, 512, [1] * 64); co = fr.zeros()
    for c in co:
        c[...] = 1
    def claim(view):
        for R in (1, 127):
            row = view.row(0, R, True, False); nb = 2 * R + 1
            hist = row[:64 * nb].reshape(64, nb)
            assert (hist[:, R + 1] == 4096).all() and int(hist.sum()) == 64 * 4096
            assert (row[64 * nb:].view(np.int32) == 1).all()
    return Case("one_value_everywhere_64x64_blocks", PC.encode_baseline(fr, co), claim)


@_add
def decode_ac_0_leaves_positions_1_to_63_in_the_zero_bin():
    fr = PC.Frame(40, 24, [(2, 2, 0), (1, 1, 1), (1, 1, 1)], {0: [2] * 64, 1: [3] * 64}); co = fr.zeros()
    rng = np.random.default_rng(5)
    for c in co:
        c[...] = rng.integers(-9, 10, c.shape)
    def claim(view):
        for c in range(3):
            row = view.row(c, 2, True, False)
            hist = row[:64 * 5].reshape(64, 5); n = view.tensor(c).shape[0] * view.tensor(c).shape[1]
            assert (hist[1:, 2] == n).all() and int(hist[1:].sum()) == 63 * n, "every AC position entirely in the zero bin"
            assert not row[64 * 5 + 1:64 * 5 + 64].any() and not row[64 * 5 + 65:].any()
            expect_position(view, c, 2, True, False, 0, "decode_ac = 0")
    return Case("decode_ac_0_leaves_positions_1_to_63_in_the_zero_bin", PC.encode_baseline(fr, co), claim, decode_ac=False, refuses=("zero_bin_not_rebuilt",))


@_add
def zigzag_position_5_is_natural_index_2():
    fr = _grey(16, 8, [1] * 64); co = fr.zeros()
    co[0][0, :, 5] = 7                                              # frame coefficients are in zig-zag order: position 5 = natural index 2
    def claim(view):
        assert (view.tensor(0)[..., 2] == 7).all() and PC.ZIGZAG[5] == 2 and POSITION[5] == 15
        nat = view.row(0, 16, True, False)[:64 * 33].reshape(64, 33); zz = view.row(0, 16, True, True)[:64 * 33].reshape(64, 33)
        assert int(nat[2, 23]) == 2 and int(nat[:, 23].sum()) == 2 and int(zz[5, 23]) == 2 and int(zz[:, 23].sum()) == 2
    return Case("zigzag_position_5_is_natural_index_2", PC.encode_baseline(fr, co), claim, refuses=("zigzag_wrong_way_round",))


_BUILT = None


def built():
    global _BUILT
    if _BUILT is None:
        _BUILT = [fn() for fn in CASES]
        assert len({c.name for c in _BUILT}) == len(_BUILT)
    return _BUILT


# ------------------------------------------------------------------------------------------------------------------ the oracle's answer
def natural_dqt(parsed, c):
    """The 64 DQT entries of component c in natural order, from oracle.harness.parse_jpeg's record."""
    return np.asarray(parsed.dqt[parsed.comps[c][3]], np.int64).reshape(64)


class OracleView:
    """One file through the oracle (tests/test_gpu_coefs.py's Truth): the blocks of a Full-IDCT decode (or of the decode_ac = 0 decode), the cumulative DC
    read off the planes of the decode_ac = 0 decode, the tables of the file's header; rows by tests/coef_hist_model.py, computed once."""

    def __init__(self, harness, oracles, data, decode_ac=True):
        import coef_hist_model as HM
        import coef_model as M
        full, dc = oracles
        self.parsed = harness.drive(dc, data)
        self.geo = M.geometry_of(self.parsed)
        self.cum = M.cum_from_planes(dc.planes(), self.geo)
        if decode_ac:
            harness.drive(full, data); self.blocks = harness.oracle_coefs(full)
        else:
            self.blocks = harness.oracle_coefs(dc)
        assert self.blocks.shape == (self.geo.nblocks, 64)
        self._M, self._HM, self._rows, self._tensors = M, HM, {}, {}

    def tensor(self, c):
        if c not in self._tensors:
            self._tensors[c] = self._M.coef_tensor(self.blocks, self.cum, self.geo, c); self._tensors[c].setflags(write=False)
        return self._tensors[c]

    def q(self, c):
        return natural_dqt(self.parsed, c)

    def row(self, c, R, quantised=True, zigzag=False):
        key = (c, R, bool(quantised), bool(zigzag))
        if key not in self._rows:
            self._rows[key] = self._HM.row_of_tensor(self.tensor(c), self.q(c), R, quantised, zigzag); self._rows[key].setflags(write=False)
        return self._rows[key]
