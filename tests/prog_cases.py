"""The catalogue of progressive (SOF2) files behind tests/test_prog_codec.py (CPU) and tests/test_gpu_progressive_forms.py (GPU).

Every case is built by WRITING COEFFICIENTS (not by encoding pictures) so that a named event is in the stream, is coded by
tests/prog_codec.py, and carries a `check` that asserts -- on the CPU, from the event record of prog_codec.decode -- that the
event is really there: a change to a generator that loses the coverage fails in the CPU suite, not silently on the GPU.

`build_all()` builds every file once per process (the pure-Python codec is the cost) and is shared by the CPU and GPU modules.
The truth for the GPU is what `decode` holds at EOI (padding blocks that non-interleaved scans do not code stay as the DC scan
left them), never the coefficients handed to the encoder.

Races.  The `race_*` cases put two scans of ONE dependency level on the two halves of one 32-bit word of every block (the lane
form of the kernels changes coefficients by 32-bit atomic adds, the wave form's DC refinement by a 32-bit atomic or, the
rest by 16-bit stores).  A lost update shows as a wrong coefficient -- but a pass cannot prove the absence of a race, only a
failure its presence.

Geometries.  Kept: luma 1x1, 2x1, 1x2, 2x2, 4x1, 1x4, 4x2 with 1x1 chroma; Y 2x2 / Cb 2x1 / Cr 1x1; a grey frame that declares
2x2.  Dropped: none of the issue's list (sampling factors of 3, which the back end's integer replication does not take, were
never on it).
"""
from __future__ import annotations

import numpy as np

import prog_codec as P

Q0 = [1 + k // 4 for k in range(64)]              # zig-zag order
Q1 = [2 + k // 3 for k in range(64)]
GEOMETRIES = {
    "1x1": [(1, 1, 0), (1, 1, 1), (1, 1, 1)], "2x1": [(2, 1, 0), (1, 1, 1), (1, 1, 1)], "1x2": [(1, 2, 0), (1, 1, 1), (1, 1, 1)],
    "2x2": [(2, 2, 0), (1, 1, 1), (1, 1, 1)], "4x1": [(4, 1, 0), (1, 1, 1), (1, 1, 1)], "1x4": [(1, 4, 0), (1, 1, 1), (1, 1, 1)],
    "4x2": [(4, 2, 0), (1, 1, 1), (1, 1, 1)], "2x2_2x1_1x1": [(2, 2, 0), (2, 1, 1), (1, 1, 1)], "grey_declares_2x2": [(2, 2, 0)],
    "grey": [(1, 1, 0)],
}


def frame_of(geo, w, h, q0=Q0, q1=Q1):
    comps = GEOMETRIES[geo]
    return P.Frame(w, h, comps, {0: q0, 1: q1} if len(comps) == 3 else {0: q0})


def noise(fr, seed, density=0.25, amp=60, dc=400):
    """Sparse random coefficients over the whole padded grid (the padding blocks too: DC scans code them)."""
    rng = np.random.default_rng(seed); co = fr.zeros()
    for a in co:
        v = rng.integers(-amp, amp + 1, a.shape) * (rng.random(a.shape) < density * np.linspace(1.5, 0.3, 64))
        a[...] = v.astype(np.int16)
        a[..., 0] = rng.integers(-dc, dc + 1, a.shape[:2])
    return co


def S(comps, ss, se, ah, al, **kw):
    return dict(comps=comps, ss=ss, se=se, ah=ah, al=al, **kw)


def script_standard(ncomp, dri=None):
    """DC with one refinement, luma two levels of successive approximation over two bands, chroma one."""
    allc = list(range(ncomp)); kw = {} if dri is None else dict(dri=dri)
    s = [S(allc, 0, 0, 0, 1, **kw), S(0, 1, 5, 0, 2), S(0, 6, 63, 0, 2)]
    for c in allc[1:]:
        s.append(S(c, 1, 63, 0, 1))
    s += [S(0, 1, 63, 2, 1), S(allc, 0, 0, 1, 0)]
    for c in allc[1:]:
        s.append(S(c, 1, 63, 1, 0))
    s.append(S(0, 1, 63, 1, 0))
    return s


class Case:
    def __init__(self, name, frame, coefs, script, check=None, **enc):
        self.name, self.frame, self.coefs, self.script, self.check, self.enc = name, frame, coefs, script, check, enc

    def build(self):
        self.file = P.encode_progressive(self.frame, self.coefs, self.script, **self.enc)
        self.dec = P.decode(self.file)
        self.truth = self.dec.coefs
        self.base = P.encode_baseline(self.frame, self.truth)
        self.arena = P.arena(self.frame, self.truth)
        return self

    def owner(self, comp, k):
        """Indices of the scans that write zig-zag position k of component comp."""
        return [i for i, s in enumerate(self.dec.scans) if comp in s["comps"] and s["ss"] <= k <= s["se"]]


def shift_for(cur, want, mod):
    """Length of a COM segment's payload that moves file offset `cur` to `want` modulo `mod` (the segment adds 4 + payload)."""
    s = (want - cur) % mod
    while s < 4:
        s += mod
    return s - 4


# =========================================================================================================== the cases
CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def _scans(D, **kw):
    return [s for s in D.scans if all(s[k] == v for k, v in kw.items())]


# ---------------------------------------------------------------------------------------------- scripts and the level logic
@case
def dc_interleaved_ac_whole_cr_y_cb():
    fr = frame_of("2x2", 67, 53)
    def check(c):
        D = c.dec
        assert [s["comps"] for s in D.scans] == [[0, 1, 2], [2], [0], [1]] and all(s["ss"] == 1 and s["se"] == 63 for s in D.scans[1:])
        nby, nbx = fr.coded(0); gy, gx = fr.grid(0)
        assert nbx % 2 and nby % 2 and nbx < gx and nby < gy, "luma grid of the AC scans must be narrower and shorter than the padded one"
    return Case("dc_interleaved_ac_whole_cr_y_cb", fr, noise(fr, 1), [S([0, 1, 2], 0, 0, 0, 0), S(2, 1, 63, 0, 0), S(0, 1, 63, 0, 0), S(1, 1, 63, 0, 0)], check)


@case
def dc_per_component_single_coefficient_bands():
    fr = frame_of("2x1", 61, 43)
    sc = [S(0, 0, 0, 0, 0), S(1, 0, 0, 0, 0), S(2, 0, 0, 0, 0), S(0, 1, 1, 0, 0), S(0, 2, 30, 0, 0), S(0, 31, 31, 0, 0), S(0, 32, 62, 0, 0), S(0, 63, 63, 0, 0),
          S(1, 1, 63, 0, 0), S(2, 1, 1, 0, 0), S(2, 2, 63, 0, 0)]
    co = noise(fr, 2, density=0.4)
    co[0][::2, ::2, 63] = 7; co[0][1::2, :, 31] = -2; co[0][:, 1::2, 1] = 5; co[2][..., 1] = 3
    def check(c):
        D = c.dec
        assert sum(1 for s in D.scans if s["ss"] == 0 and len(s["comps"]) == 1) == 3
        single = {s["ss"] for s in D.scans if s["ss"] == s["se"] and s["ss"]}
        assert {1, 31, 63} <= single
        assert len([s for s in D.scans if s["comps"] == [0] and s["ss"]]) >= 5
        for k in (1, 31, 63):
            assert np.count_nonzero(D.coefs[0][..., k]) > 3, "single-coefficient band without coefficients"
    return Case("dc_per_component_single_coefficient_bands", fr, co, sc, check)


@case
def dc_al3_three_refinements_between_ac():
    fr = frame_of("2x2", 67, 53)
    sc = [S([0, 1, 2], 0, 0, 0, 3), S(0, 1, 63, 0, 0), S(0, 0, 0, 3, 2), S(1, 1, 63, 0, 0), S([1, 2], 0, 0, 3, 2), S([0, 1, 2], 0, 0, 2, 1),
          S(2, 1, 63, 0, 0), S(2, 0, 0, 1, 0), S(0, 0, 0, 1, 0), S(1, 0, 0, 1, 0)]
    co = noise(fr, 3)
    def check(c):
        D = c.dec
        assert len(_scans(D, ss=0, ah=0, al=3)) == 1 and len([s for s in D.scans if s["ss"] == 0 and s["ah"]]) == 6
        assert any(len(s["comps"]) == 2 for s in D.scans), "a DC scan of two components"
        dc = D.coefs[0][..., 0]
        assert (dc < 0).any() and ((dc < 0) & (dc & 7 != 0)).any(), "negative DC values with low bits under Al = 3"
    return Case("dc_al3_three_refinements_between_ac", fr, co, sc, check)


@case
def successive_approximation_three_and_two_levels():
    fr = frame_of("2x1", 75, 37)
    sc = [S([0, 1, 2], 0, 0, 0, 0), S(0, 1, 63, 0, 3), S(1, 1, 63, 0, 2), S(2, 1, 63, 0, 3), S(0, 1, 63, 3, 2), S(1, 1, 63, 2, 1), S(2, 1, 63, 3, 2),
          S(0, 1, 63, 2, 1), S(2, 1, 63, 2, 1), S(1, 1, 63, 1, 0), S(0, 1, 63, 1, 0), S(2, 1, 63, 1, 0)]
    def check(c):
        D = c.dec
        for comp, n in ((0, 3), (1, 2), (2, 3)):
            assert len([s for s in D.scans if s["comps"] == [comp] and s["ss"] and s["ah"]]) == n
        assert all(sum(nb for nb, _k, _u in s["stretches"]) > 20 for s in D.scans if s["ss"] and s["ah"] and s["al"] < 2)
    return Case("successive_approximation_three_and_two_levels", fr, noise(fr, 4, density=0.35, amp=90), sc, check)


@case
def first_split_refined_whole():
    fr = frame_of("1x2", 43, 61)
    sc = [S([0, 1, 2], 0, 0, 0, 0)]
    for c in (0, 1, 2):
        sc += [S(c, 1, 5, 0, 1), S(c, 6, 63, 0, 1)]
    for c in (0, 1, 2):
        sc += [S(c, 1, 63, 1, 0)]
    def check(c):
        assert len(c.dec.scans) == 10 and len(_scans(c.dec, ss=1, se=63, ah=1)) == 3
    return Case("first_split_refined_whole", fr, noise(fr, 5, density=0.3), sc, check)


@case
def first_whole_refined_split():
    fr = frame_of("1x1", 45, 35)
    sc = [S([0, 1, 2], 0, 0, 0, 0)]
    for c in (0, 1, 2):
        sc += [S(c, 1, 63, 0, 1)]
    for c in (0, 1, 2):
        sc += [S(c, 10, 63, 1, 0), S(c, 1, 9, 1, 0)]
    def check(c):
        assert len(c.dec.scans) == 10 and len(_scans(c.dec, ss=1, se=9, ah=1)) == 3 and len(_scans(c.dec, ss=10, se=63, ah=1)) == 3
    return Case("first_whole_refined_split", fr, noise(fr, 6, density=0.3), sc, check)


def _race_frame():
    return frame_of("grey", 512, 512)              # 4096 blocks: the scans of a level overlap in time


@case
def race_dc_refinement_beside_band_1():
    fr = _race_frame(); rng = np.random.default_rng(7); co = fr.zeros()[0]
    co[..., 0] = rng.integers(-300, 300, co.shape[:2])
    co[..., 1] = rng.integers(-7, 8, co.shape[:2])                                  # natural index 1: the other half of the DC's word
    co[..., 2:12] = rng.integers(-3, 4, co.shape[:2] + (10,))
    sc = [S(0, 0, 0, 0, 1, dri=64), S(0, 1, 1, 0, 1), S(0, 2, 63, 0, 0), S(0, 0, 0, 1, 0), S(0, 1, 1, 1, 0)]
    def check(c):
        D = c.dec
        assert D.scans[3]["ss"] == 0 and D.scans[3]["ah"] == 1 and D.scans[4]["ss"] == D.scans[4]["se"] == 1 and D.scans[4]["ah"] == 1
        assert P.ZIGZAG[1] == 1 and D.scans[4]["units"] >= 4096
        z1 = D.coefs[0][..., 1]
        assert np.count_nonzero(np.abs(z1) == 1) > 500 and np.count_nonzero((np.abs(z1) > 1) & (z1 & 1 != 0)) > 500, "new values and corrections at natural index 1"
        assert np.count_nonzero(D.coefs[0][..., 0] & 1) > 1000
    return Case("race_dc_refinement_beside_band_1", fr, [co], sc, check)


@case
def race_bands_split_inside_a_word():
    fr = _race_frame(); rng = np.random.default_rng(8); co = fr.zeros()[0]
    co[..., 0] = rng.integers(-300, 300, co.shape[:2])
    co[..., 1:8] = rng.integers(-9, 10, co.shape[:2] + (7,))
    sc = [S(0, 0, 0, 0, 0, dri=32), S(0, 1, 2, 0, 1), S(0, 3, 3, 0, 1), S(0, 4, 63, 0, 1), S(0, 4, 63, 1, 0), S(0, 1, 2, 1, 0), S(0, 3, 3, 1, 0)]
    def check(c):
        D = c.dec
        assert P.ZIGZAG[2] == 8 and P.ZIGZAG[4] == 9, "zig-zag 2 and 4 share a 32-bit word of the natural-order row"
        assert [(s["ss"], s["se"], s["ah"]) for s in D.scans[1:]] == [(1, 2, 0), (3, 3, 0), (4, 63, 0), (4, 63, 1), (1, 2, 1), (3, 3, 1)]
        for k in (2, 4):
            z = D.coefs[0][..., k]
            assert np.count_nonzero(np.abs(z) == 1) > 300 and np.count_nonzero((z < -1) & (z & 1 != 0)) > 300 and np.count_nonzero((z > 1) & (z & 1 != 0)) > 300
    return Case("race_bands_split_inside_a_word", fr, [co], sc, check)


@case
def values_every_category_al0():
    q0 = list(Q0); q0[5] = 300; q0[0] = 3                                          # a 16-bit quantiser table; products wrap in int16
    fr = frame_of("grey", 96, 64, q0=q0); co = fr.zeros()[0]
    flat = co.reshape(-1, 64)
    for i in range(len(flat)):
        flat[i, 0] = (1023, -1023, 1023, 0, 1, 0, -1, 512)[i % 8]
        for j in range(10):
            m = (1 << j) if (i + j) % 3 else (1 << (j + 1)) - 1
            flat[i, 1 + (i + 5 * j) % 63] = m if (i + j) % 2 else -m
    def check(c):
        D = c.dec; z = D.coefs[0].reshape(-1, 64).astype(int)
        cats = {(int(abs(v)).bit_length(), v > 0) for v in z[:, 1:].ravel() if v}
        assert cats >= {(n, sg) for n in range(1, 11) for sg in (True, False)}, "AC categories 1..10, both signs"
        d = np.diff(np.concatenate([[0], z[:, 0]]))
        dc = {(int(abs(v)).bit_length(), v > 0) for v in d if v}
        assert dc >= {(11, True), (11, False), (1, True), (1, False)}, "DC differences up to category 11"
    return Case("values_every_category_al0", fr, [co], [S(0, 0, 0, 0, 0), S(0, 1, 63, 0, 0)], check)


@case
def values_point_transform_al1():
    fr = frame_of("1x1", 64, 48); co = noise(fr, 10, density=0.5, amp=3, dc=40)
    def check(c):
        D = c.dec
        for comp in range(3):
            z = D.coefs[comp]
            assert (z[..., 1:] == 1).sum() > 20 and (z[..., 1:] == -1).sum() > 20, "+1 / -1: zero in the first scan, new in the refinement"
            assert (z[..., 1:] == -3).sum() > 5 and (z[..., 1:] == 3).sum() > 5
            dc = z[..., 0]
            assert ((dc < 0) & (dc & 1 == 1)).any() and ((dc < 0) & (dc & 1 == 0)).any(), "negative DC, odd and even, under Al = 1"
    return Case("values_point_transform_al1", fr, co, script_standard(3), check)


# ------------------------------------------------------------------------------------------------------------------ geometry
def _geo_case(geo, w, h, seed):
    def make():
        fr = frame_of(geo, w, h)
        def check(c):
            D = c.dec
            assert D.frame.comps == fr.comps
            nby, nbx = fr.coded(0); gy, gx = fr.grid(0); H, V = fr.hv[0]
            if fr.ncomp == 3 and (H > 1 or V > 1):
                assert (H == 1 or nbx % H) and (V == 1 or nby % V) and (nbx < gx or H == 1) and (nby < gy or V == 1), (nbx, nby, gx, gy)
            assert all(s["overrun"] == 0 for s in D.scans)
        return Case("geometry_" + geo, fr, noise(fr, seed), script_standard(fr.ncomp, dri=(None, 3, 5)[seed % 3]), check)
    make.__name__ = "geometry_" + geo
    CASES.append(make)


for _i, (_g, _w, _h) in enumerate([("1x1", 43, 29), ("2x1", 51, 27), ("1x2", 29, 51), ("2x2", 83, 51), ("4x1", 75, 21), ("1x4", 21, 75), ("4x2", 67, 37),
                                   ("2x2_2x1_1x1", 51, 83), ("grey_declares_2x2", 45, 35)]):
    _geo_case(_g, _w, _h, 20 + _i)


def _partial_case(name, w, h, seed):
    def make():
        fr = frame_of("2x2", w, h)
        def check(c):
            assert (w % 16 == 0) != (h % 16 == 0), "not an MCU multiple in one direction only"
        return Case(name, fr, noise(fr, seed), script_standard(3, dri=4), check)
    make.__name__ = name
    CASES.append(make)


_partial_case("geometry_2x2_partial_mcus_in_x_only", 67, 64, 31)
_partial_case("geometry_2x2_partial_mcus_in_y_only", 64, 53, 32)


# --------------------------------------------------------------------------------------------------------- restart intervals
def _dri_case(name, dri_of, extra_check):
    def make():
        fr = frame_of("2x1", 75, 50)                  # luma 10 x 7 coded blocks in a 10 x 7 grid... chroma 5 x 7
        sc = script_standard(3)
        for i, s in enumerate(sc):
            s["dri"] = dri_of(i, s)
        def check(c):
            for s in c.dec.scans:
                assert len(s["intervals"]) == (-(-s["units"] // s["dri"]) if s["dri"] else 1)
            extra_check(c)
        return Case(name, fr, noise(fr, 30 + len(name)), sc, check)
    make.__name__ = name
    CASES.append(make)


def _chk_dri1(c):
    assert all(len(s["intervals"]) > 8 for s in c.dec.scans), "RSTn numbering wraps"
    assert any(s["ss"] == 0 and s["ah"] and all(e - a <= 2 for a, e in s["intervals"]) and
               sum(e - a == 1 for a, e in s["intervals"]) > 8 for s in c.dec.scans), "DC refinement intervals of one byte (two where it is FF 00)"


def _chk_dri7(c):
    nby, nbx = c.frame.coded(0)
    assert nbx % 7 and all(s["dri"] == 7 for s in c.dec.scans)


def _chk_dri_big(c):
    assert all(s["dri"] > s["units"] and len(s["intervals"]) == 1 for s in c.dec.scans)


def _chk_dri_changes(c):
    d = [s["dri"] for s in c.dec.scans]
    assert d[:3] == [0, 7, 64] and len(set(d)) >= 4


_dri_case("dri_1", lambda i, s: 1, _chk_dri1)
_dri_case("dri_7_does_not_divide_a_row", lambda i, s: 7, _chk_dri7)
_dri_case("dri_larger_than_the_scan", lambda i, s: 1000, _chk_dri_big)
_dri_case("dri_changes_between_scans", lambda i, s: (0, 7, 64, 3, 0, 8, 5, 2, 11)[i % 9], _chk_dri_changes)


@case
def dri_interval_of_one_eobrun_and_dc_refinement_byte():
    fr = frame_of("grey", 128, 96); co = noise(fr, 40, density=0.3)[0]              # 16 x 12 blocks
    co[3:5, :, 1:] = 0; co[8, :, 1:6] = 0                                          # two whole block rows without AC; one without the low band
    sc = [S(0, 0, 0, 0, 1, dri=16), S(0, 1, 5, 0, 1), S(0, 6, 63, 0, 1), S(0, 0, 0, 1, 0, dri=8), S(0, 1, 63, 1, 0, dri=16)]
    def check(c):
        D = c.dec
        for s in (D.scans[1], D.scans[2], D.scans[4]):
            runs = dict(s["eobruns"])
            assert any(runs.get(iv * 16) == 16 and e - a <= 2 for iv, (a, e) in enumerate(s["intervals"])), "an interval that is one EOBRUN symbol"
        assert all(e - a == 1 for a, e in D.scans[3]["intervals"]) and len(D.scans[3]["intervals"]) == 24
    return Case("dri_interval_of_one_eobrun_and_dc_refinement_byte", fr, [co], sc, check)


# --------------------------------------------------------------------------------------------- end-of-band runs and zero runs
RUN_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256]


@case
def eobrun_lengths():
    fr = frame_of("grey", 320, 240); co = fr.zeros()[0]; flat = co.reshape(-1, 64)   # 40 x 30 = 1200 blocks
    flat[:, 0] = np.arange(len(flat)) % 50 - 25
    u = 0
    for i, n in enumerate(RUN_LENGTHS):
        flat[u, 63] = 5; flat[u, 1 + i % 20] = -3; u += 1 + n                       # a block that ends on Se, then n empty ones
    flat[u, 63] = 2; u += 1
    for k in range(5):                                                              # EOBn after some coefficients of the same block
        flat[u, 1 + k] = 4; flat[u, 9] = -2; u += 3
    assert u < len(flat)
    def check(c):
        s = c.dec.scans[1]
        assert {n for _u, n in s["eobruns"]} >= set(RUN_LENGTHS), sorted({n for _u, n in s["eobruns"]})
        assert s["eob_after_coefs"] >= 5
        assert s["eobruns"][-1][0] + s["eobruns"][-1][1] == s["units"], "the last run ends on the last block of the scan"
    return Case("eobrun_lengths", fr, [co], [S(0, 0, 0, 0, 0), S(0, 1, 63, 0, 0)], check)


@case
def eobrun_crosses_rows_of_a_2x2_component():
    fr = frame_of("2x2", 67, 59); co = noise(fr, 42, density=0.0)                   # luma: 9 x 8 coded in a 10 x 8 grid
    nby, nbx = fr.coded(0); y = co[0]
    def put(u):
        y[u // nbx, u % nbx, 63] = 3
    # runs (start, length): short ones (stepped) and long ones (re-seek) over the end of a block row and of an MCU row
    plan = [(nbx - 1, 2), (2 * nbx - 2, 3), (3 * nbx - 2, 5), (4 * nbx - 1, 1 + nbx), (6 * nbx - 3, 4)]
    busy = set(range(nby * nbx))
    for s0, n in plan:
        busy -= set(range(s0, s0 + n))
    for u in busy:
        put(u)
    co[1][..., 1:] = 0; co[1][1, 2, 7] = 9                                           # chroma: nearly empty bands
    def check(c):
        s = [q for q in c.dec.scans if q["comps"] == [0] and q["ss"] == 1][0]
        runs = s["eobruns"]
        assert set(runs) >= set(plan), runs
        cross_row = [(u, n) for u, n in runs if u % nbx + n > nbx]; cross_mcu = [(u, n) for u, n in runs if (u // nbx) // 2 != ((u + n - 1) // nbx) // 2]
        assert any(n <= 4 for _u, n in cross_row) and any(n >= 5 for _u, n in cross_row) and cross_mcu
        assert any(n - 1 == 3 for _u, n in runs) and any(n - 1 == 4 for _u, n in runs), "skips of exactly 3 and 4 blocks"
    sc = [S([0, 1, 2], 0, 0, 0, 0), S(0, 1, 63, 0, 0), S(1, 1, 63, 0, 0), S(2, 1, 63, 0, 0)]
    return Case("eobrun_crosses_rows_of_a_2x2_component", fr, co, sc, check)


@case
def eobrun_ends_on_the_last_block_of_an_interval():
    fr = frame_of("grey", 160, 96); co = fr.zeros()[0]; flat = co.reshape(-1, 64)     # 20 x 12 = 240 blocks, intervals of 12
    # band 1..31 (first scan only) ends every block on position 31; band 32..63 is refined: history on 40, a new value on 63
    flat[:, 0] = 7; flat[:, 2] = 6; flat[:, 31] = 5; flat[:, 40] = 6; flat[:, 63] = 1
    for iv in (1, 4, 9):
        flat[iv * 12 + 5: iv * 12 + 12, 1:] = 0                                     # a run of 7 up to the interval's last block
    flat[19 * 12 + 8:, 1:] = 0                                                      # ... and up to the scan's last block
    flat[3 * 12: 4 * 12, 1:] = 0                                                    # a whole interval
    sc = [S(0, 0, 0, 0, 0, dri=12), S(0, 1, 31, 0, 0), S(0, 32, 63, 0, 1), S(0, 32, 63, 1, 0)]
    def check(c):
        for s in (c.dec.scans[1], c.dec.scans[3]):
            ends = {u + n for u, n in s["eobruns"]}
            assert {24, 60, 120, 240, 48} <= ends, sorted(ends)
            assert (17, 7) in s["eobruns"] and (36, 12) in s["eobruns"]
    return Case("eobrun_ends_on_the_last_block_of_an_interval", fr, [co], sc, check)


def _big_case():
    """256 x 130 = 33 280 blocks: an empty band is one run of 32 767 and one of 513, in a first scan and in a refinement scan;
    the DC refinement scan is a bit pipe of 4160 bytes before stuffing in one interval: all ones for its first part (every byte
    stuffed, more than 4 KiB: the 2 KiB ring of the wave reader wraps more than once), then noise."""
    fr = frame_of("grey", 2048, 1040); rng = np.random.default_rng(44); co = fr.zeros()[0]; flat = co.reshape(-1, 64)
    n = len(flat); assert n == 33280
    flat[:, 0] = rng.integers(-100, 100, n) * 2
    flat[: 8 * 2600, 0] |= 1
    flat[8 * 2600:, 0] |= rng.integers(0, 2, n - 8 * 2600).astype(np.int16)
    idx = rng.choice(n, 900, replace=False)
    flat[idx, 6 + rng.integers(0, 58, 900)] = rng.integers(1, 9, 900) * rng.choice([-1, 1], 900)
    sc = [S(0, 0, 0, 0, 1), S(0, 1, 5, 0, 1), S(0, 6, 63, 0, 1), S(0, 1, 5, 1, 0), S(0, 6, 63, 1, 0), S(0, 0, 0, 1, 0)]
    def check(c):
        D = c.dec
        assert D.scans[1]["eobruns"] == [(0, 32767), (32767, 513)] and D.scans[3]["eobruns"] == [(0, 32767), (32767, 513)]
        s = D.scans[5]
        assert s["end"] - s["start"] > 6000 and len(s["intervals"]) == 1
        ff = np.array(s["ff00"])
        assert len(ff) > 2600 and np.all(np.diff(ff[:2600]) == 2), "a stretch in which every byte is stuffed"
        for mod in (8, 32, 1024):
            assert {int(x) for x in ff % mod} >= {mod - 1}, "an FF 00 pair across a %d-byte line of the file" % mod
    return Case("eobrun_32767_then_a_shorter_one_and_long_scans", fr, [co], sc, check)


def _with_odd_start(c, scan_index):
    """COM pad so that the entropy data of scan `scan_index` starts on an odd file offset (its FF 00 pairs, which follow each
    other at a distance of two in an all-ones pipe, then sit across the even-sized grids' lines)."""
    f = P.encode_progressive(c.frame, c.coefs, c.script)
    start = P.decode(f).scans[scan_index]["start"]
    c.enc["com_len"] = shift_for(start, 1, 2) if start % 2 == 0 else None
    return c


@case
def eobrun_32767_then_a_shorter_one_and_long_scans():
    return _with_odd_start(_big_case(), 5)


@case
def first_scan_zero_runs_one_two_three_zrl():
    fr = frame_of("grey", 128, 64); co = fr.zeros()[0]; flat = co.reshape(-1, 64)      # 128 blocks
    flat[:, 0] = 11
    for i, k in enumerate([17, 18, 32, 33, 40, 48, 49, 55, 63, 63, 16, 1]):
        flat[i * 3, k] = -6 if i % 2 else 6
        flat[i * 3 + 1, 1] = 2; flat[i * 3 + 1, k] = 3                              # the same run after a coefficient
    def check(c):
        per = {}
        for u, _k, _k1 in c.dec.scans[1]["zrl"]:
            per[u] = per.get(u, 0) + 1
        assert set(per.values()) >= {1, 2, 3}, per
    return Case("first_scan_zero_runs_one_two_three_zrl", fr, [co], [S(0, 0, 0, 0, 0), S(0, 1, 63, 0, 1), S(0, 1, 63, 1, 0)], check)


@case
def refinement_stretches_and_zrl():
    """Refinement at Al = 0 after a first scan at Al = 1: |v| >= 2 is history (takes a correction bit: its low bit), |v| == 1 is new."""
    fr = frame_of("grey", 192, 64); co = fr.zeros()[0]; flat = co.reshape(-1, 64); rng = np.random.default_rng(50)   # 24 x 8 = 192 blocks
    flat[:, 0] = 9
    def hist(u, ks):
        for k in ks:
            flat[u, k] = int(rng.choice([-1, 1])) * int(rng.integers(2, 12))
    u = 0
    for n in (31, 32, 33, 60, 62, 1, 5):                       # n correction bits inside a (run, 1) symbol: history 1..n, new at n + 1 / at 63
        hist(u, range(1, n + 1)); flat[u, n + 1] = 1; u += 1
        hist(u, range(1, n + 1)); flat[u, 63] = -1; u += 1
    for n in (31, 32, 33, 60, 63, 2):                           # n correction bits in the tail after EOBn / inside a run
        hist(u, range(1, n + 1)); u += 1
        u += 1                                                  # (an empty block inside the same run)
        hist(u, range(64 - n, 64)); flat[u, 1] = 1 if n < 62 else flat[u, 1]; u += 1
    # ZRL whose sixteen zeros are interleaved with history; ends at Se - 1 with the new value on Se; new value on Ss
    hist(u, range(1, 41, 2)); flat[u, 45] = 1; u += 1           # zeros at 2, 4, .. 40 (20) + 41..44: ZRL + (8, 1), corrections on the way
    hist(u, range(1, 62, 3)); flat[u, 63] = -1; u += 1
    hist(u, [k for k in range(1, 63) if k % 4 == 0]); flat[u, 63] = 1; flat[u, 1] = -1; u += 1
    zeros = list(range(32, 63, 2))                              # exactly sixteen zeros, the last on 62, between position 1 and the new value on 63
    hist(u, [k for k in range(2, 63) if k not in zeros]); flat[u, 1] = 1; flat[u, 63] = 1; u += 1
    flat[u, 1] = 1; flat[u, 20] = -1; flat[u, 40] = 1; flat[u, 63] = -1; u += 1   # no history: ZRL without correction bits
    for k in range(10):                                          # a run over blocks with and without history
        if k % 3 == 0:
            hist(u, [5, 17, 63])
        u += 1
    flat[u, 7] = 1; u += 1
    assert u < len(flat)
    def check(c):
        s = c.dec.scans[2]
        assert s["ah"] == 1 and s["ss"] == 1 and s["se"] == 63
        sym = {nb for nb, k, _u in s["stretches"] if k == "sym"}; tail = {nb for nb, k, _u in s["stretches"] if k == "tail"}
        zrl = [nb for nb, k, _u in s["stretches"] if k == "zrl"]
        assert sym >= {31, 32, 33, 60, 62} and tail >= {31, 32, 33, 60, 63}, (sorted(sym), sorted(tail))
        assert any(nb > 0 for nb in zrl) and any(nb == 0 for nb in zrl) and len(s["zrl"]) >= 5
        assert any(k1 == 63 for _u, _k, k1 in s["zrl"]), "a ZRL whose zeros end on Se - 1 (the new value sits on Se: as far as a ZRL of a conforming encoder reaches)"
        runs = dict(s["eobruns"]); tails = {}
        for nb, k, uu in s["stretches"]:
            if k == "tail":
                tails[uu] = nb
        mixed = [u0 for u0, n in runs.items() if n >= 4 and any(uu in tails for uu in range(u0 + 1, u0 + n)) and any(uu not in tails for uu in range(u0 + 1, u0 + n))]
        assert mixed, "an end-of-band run over blocks with and without history"
        z = c.dec.coefs[0].reshape(-1, 64)
        assert (np.abs(z[:, 1]) == 1).any() and (np.abs(z[:, 63]) == 1).any(), "new values on Ss and on Se"
    return Case("refinement_stretches_and_zrl", fr, [co], [S(0, 0, 0, 0, 0), S(0, 1, 63, 0, 1), S(0, 1, 63, 1, 0)], check)


# ------------------------------------------------------------------------------------------------ bytes under the readers' grids
@case
def dc_pipe_all_ones_ff00_ends_every_interval():
    fr = frame_of("grey", 256, 128); co = noise(fr, 60)[0]; co[..., 0] |= 1              # 512 blocks, 16 per interval: FF 00 FF 00 RSTn
    sc = [S(0, 0, 0, 0, 1), S(0, 1, 63, 0, 0), S(0, 0, 0, 1, 0, dri=16)]
    def check(c):
        s = c.dec.scans[2]; ff = set(s["ff00"])
        assert len(s["intervals"]) == 32 and all(e - a == 4 and (e - 2) in ff and a in ff for a, e in s["intervals"])
    return Case("dc_pipe_all_ones_ff00_ends_every_interval", fr, [co], sc, check)


def _phase_case(k):
    def make():
        fr = frame_of("2x1", 40, 24); c = Case("scan_start_phase_%02d" % k, fr, noise(fr, 70 + k, density=0.4), script_standard(3, dri=(None, 2)[k % 2]))
        f = P.encode_progressive(fr, c.coefs, c.script); D = P.decode(f)
        tgt = 4 + k % 6                                         # a different kind of scan is moved onto the phase from file to file
        c.enc["com_len"] = shift_for(D.scans[tgt]["start"], k, 32)
        def check(cc):
            assert cc.dec.scans[tgt]["start"] % 32 == k
        c.check = check
        return c
    make.__name__ = "scan_start_phase_%02d" % k
    CASES.append(make)


for _k in range(32):
    _phase_case(_k)


@case
def scan_ends_on_a_1k_line():
    fr = frame_of("grey", 256, 192); c = Case("scan_ends_on_a_1k_line", fr, noise(fr, 80, density=0.5), script_standard(1))
    D = P.decode(P.encode_progressive(fr, c.coefs, c.script))
    c.enc["com_len"] = shift_for(D.scans[1]["end"], 0, 1024)
    def check(cc):
        assert cc.dec.scans[1]["end"] % 1024 == 0 and cc.dec.scans[1]["end"] - cc.dec.scans[1]["start"] > 100
        assert len(cc.file) > 4096
    c.check = check
    return c


def _rare_first(f):
    return P.ladder_table(sorted(f, key=lambda s: (f[s], s)), ladder=min(8, max(1, len(f) - 1)))


def _nine_bits(f):
    return P.flat_table(sorted(f), 9)


@case
def huffman_16_bit_code_for_the_most_frequent_symbol():
    fr = frame_of("2x1", 96, 64); sc = script_standard(3, dri=4)
    for s in sc:
        if s["ss"] == 0 and s["ah"] == 0:
            s["dc_tab"] = [_rare_first] * 3
        elif s["ss"]:
            s["ac_tab"] = _rare_first
    def check(c):
        for s in c.dec.scans:
            if s["ss"] or s["ah"] == 0:
                h = s["code_lens"]
                assert s["max_code"] == 16 and h[16] == max(h), (s["ss"], s["ah"], h)
                assert sum(h[1:9]) > 0, "short codes beside the long ones: the slow path in single lanes"
    return Case("huffman_16_bit_code_for_the_most_frequent_symbol", fr, noise(fr, 90, density=0.4), sc, check)


@case
def huffman_only_codes_of_nine_bits():
    fr = frame_of("1x1", 64, 64); sc = script_standard(3, dri=8)
    for s in sc:
        if s["ss"] == 0 and s["ah"] == 0:
            s["dc_tab"] = [_nine_bits] * 3
        elif s["ss"]:
            s["ac_tab"] = _nine_bits
    def check(c):
        for s in c.dec.scans:
            if s["ss"] or s["ah"] == 0:
                h = s["code_lens"]
                assert sum(h[1:9]) == 0 and h[9] > 0
    return Case("huffman_only_codes_of_nine_bits", fr, noise(fr, 91, density=0.4), sc, check)


@case
def huffman_four_dc_tables_and_ac_table_redefined():
    fr = frame_of("2x2", 64, 48)
    spare = P.flat_table(list(range(12)), 5)
    sc = [S(0, 0, 0, 0, 1, dc_ids=[3], extra_dht=[(0, 0, spare)]), S(1, 0, 0, 0, 1, dc_ids=[2]), S(2, 0, 0, 0, 1, dc_ids=[1]),
          S(0, 1, 63, 0, 0, ac_id=3), S(1, 1, 63, 0, 0, ac_id=0), S(2, 1, 63, 0, 0, ac_id=0), S([0, 1, 2], 0, 0, 1, 0)]
    def check(c):
        D = c.dec
        dc = {}
        for tc, th, t in D.dht_defs:
            if tc == 0:
                dc[th] = (tuple(t[0]), tuple(t[1]))
        assert set(dc) == {0, 1, 2, 3} and len(set(dc.values())) == 4, "four distinct DC tables, ids 0..3"
        assert [s["dc_ids"] for s in D.scans[:3]] == [[3], [2], [1]]
        ac0 = [(tuple(t[0]), tuple(t[1])) for tc, th, t in D.dht_defs if tc == 1 and th == 0]
        assert len(ac0) == 2 and ac0[0] != ac0[1], "AC table 0 redefined between two scans"
    co = noise(fr, 92); co[2][..., 1:] //= 4
    return Case("huffman_four_dc_tables_and_ac_table_redefined", fr, co, sc, check)


# ================================================================================================================= random scripts
def random_partition(rng, lo, hi):
    cuts = sorted({int(x) for x in rng.integers(lo + 1, hi + 1, int(rng.integers(0, 4)))})
    edges = [lo] + cuts + [hi + 1]
    return [(a, b - 1) for a, b in zip(edges[:-1], edges[1:]) if a < b]


def random_script(rng, ncomp):
    """A random legal script: per component the band 1..63 is cut at random for the first scans (at a random Al) and cut again,
    differently, for every bit plane below; DC likewise, interleaved or per component.  Legal by construction: every position
    of a plane was coded by the plane above.  The per-component order is kept, components are shuffled into each other."""
    chains = []
    dcal = int(rng.integers(0, 3)); allc = list(range(ncomp))
    dc = [S(allc, 0, 0, 0, dcal)] if (ncomp == 1 or rng.integers(2)) else [S([c], 0, 0, 0, dcal) for c in allc]
    for a in range(dcal - 1, -1, -1):
        dc += [S(allc, 0, 0, a + 1, a)] if (ncomp == 1 or rng.integers(2)) else [S([c], 0, 0, a + 1, a) for c in rng.permutation(ncomp).tolist()]
    for c in allc:
        al = int(rng.integers(0, 3)); ch = [S(c, a, b, 0, al) for a, b in random_partition(rng, 1, 63)]
        for a in range(al - 1, -1, -1):
            part = random_partition(rng, 1, 63); order = rng.permutation(len(part)).tolist()
            ch += [S(c, part[i][0], part[i][1], a + 1, a) for i in order]
        chains.append(ch)
    # DC first scans lead; the rest is merged at random, each chain in its own order
    ndc_first = 1 if len(dc[0]["comps"]) == ncomp else ncomp
    out = dc[:ndc_first]; chains.append(dc[ndc_first:])
    while any(chains):
        live = [ch for ch in chains if ch]
        out.append(live[int(rng.integers(len(live)))].pop(0))
    for s in out:
        if rng.integers(3) == 0:
            s["dri"] = int(rng.choice([0, 1, 2, 5, 9, 40, 500]))
    return out


def random_case(rng, k):
    geo = list(GEOMETRIES)[int(rng.integers(len(GEOMETRIES)))]
    fr = frame_of(geo, int(rng.integers(8, 120)), int(rng.integers(8, 100)))
    co = noise(fr, int(rng.integers(1 << 30)), density=float(rng.choice([0.02, 0.2, 0.6, 1.0])), amp=int(rng.choice([2, 12, 200])))
    return Case("random_%03d_%s_%dx%d" % (k, geo, fr.width, fr.height), fr, co, random_script(rng, fr.ncomp), com_len=int(rng.integers(0, 40)))


# ======================================================================================================================== builds
NAMES = [fn.__name__ for fn in CASES]
assert len(set(NAMES)) == len(NAMES)
_BUILT = {}
_RANDOM = {}


def built(name):
    """Catalogue case `name`, built once per process."""
    if name not in _BUILT:
        c = CASES[NAMES.index(name)]().build()
        assert c.name == name, (c.name, name)
        _BUILT[name] = c
    return _BUILT[name]


def build_all():
    return [built(n) for n in NAMES]


def build_random(n, seed=2025):
    if (n, seed) not in _RANDOM:
        rng = np.random.default_rng(seed)
        _RANDOM[(n, seed)] = [random_case(rng, k).build() for k in range(n)]
    return _RANDOM[(n, seed)]
