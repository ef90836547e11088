"""The catalogue of preview states behind tests/test_preview_cases.py (CPU: the model against the oracle, the census) and
tests/test_gpu_preview.py (GPU: the general colour path of the back end -- back_end_mcus<false,1,1> -> mcu_to_dib -> ycc_to_bgra /
channel_extract -- against the oracle).  CPU only: harness.synth_jpeg, the SOF rewrite of test_gpu_parity.py::test_header_variations, and
one progressive file of tests/prog_cases.py.

Pictures: one per layout, 11 x 7 MCUs each, width and height no multiples of the MCU.  The two `partial` layouts rewrite the SOF of a 4:2:0
file, so their scans decode to garbage, deterministically: the DC predictors drift, which is where samples far outside [-1024, 1023] come from
(the two large magnitudes need them, see the census).

States: (mode, shift_mcu_x, shift_mcu_y, shift_y, shift_cb, shift_cr) as tests/preview_model.py takes them.  The crossing is sparse and
asserted at import (assert_crossing): every layout with every mode, every layout with every start, every magnitude with every mode, every
layout with a mode other than 1 together with a shift.

Start MCUs at wave and workgroup seams come from the work split of upload() as tests/test_gpu_backend_tiling.py states it (wgs_of), at three
MCUs per wave, for both ways the back end hands MCUs to waves: back_end_pairs gives a workgroup a contiguous range of ceil(nmcu / workgroups)
MCUs, back_end_mcus (the general path) gives wave w of workgroup g the MCUs 8 g + w, 8 g + w + 8 * workgroups, ...

What a state can change.  A mode shows some components only (VISIBLE), so e.g. a Cb shift under PREVIEW_Y changes nothing; a grey picture's
chroma is 0, so a chroma shift s with 0 <= s < 8 gives (0 + s) >> 3 == 0.  `inert` names those states: the census demands a changed pixel of
every other state whose start lies inside the picture, and of the inert ones that nothing changes."""
from collections import namedtuple

from test_gpu_backend_tiling import wgs_of

Case = namedtuple("Case", "layout state")
Picture = namedtuple("Picture", "name data parsed oracle_data mcu_w mcu_h xmax ymax progressive")

XMAX, YMAX = 11, 7
# name -> (synth keywords, SOF rewrite or None, (mcu_w, mcu_h)); sizes: 11 x 7 MCUs less a few pixels each way
LAYOUTS = {
    "gray":  (dict(width=83, height=53, gray=1, seed=501), None, (8, 8)),
    "444":   (dict(width=85, height=51, hs=1, vs=1, seed=502), None, (8, 8)),
    "422":   (dict(width=171, height=53, hs=2, vs=1, seed=503), None, (16, 8)),
    "440":   (dict(width=83, height=107, hs=1, vs=2, seed=504), None, (8, 16)),
    "420":   (dict(width=171, height=107, hs=2, vs=2, seed=505), None, (16, 16)),
    "411":   (dict(width=345, height=53, hs=4, vs=1, seed=506), None, (32, 8)),
    "partial_311": (dict(width=259, height=53, hs=2, vs=2, seed=507), [(3, 1), (1, 1), (1, 1)], (24, 8)),      # 385 of the file's 408 blocks
    "partial_421": (dict(width=345, height=107, hs=2, vs=2, seed=525), [(4, 2), (2, 1), (1, 2)], (32, 16)),    # 924 blocks, as many as the file has
    "prog420": (dict(width=171, height=107, seed=509), None, (16, 16)),
}
QUALITY = 92
PARTIAL = ("partial_311", "partial_421")
MODES = tuple(range(1, 9))
ORDINARY = ((160, -80, 40), (0, 0, 8), (-8, 0, 0), (0, 7, 0), (16376, -16376, 16376))
LARGE = ((-30000, 30000, -30000), (30000, 0, 0))            # sample + shift leaves the int16 range for some sample of the partial pictures
MAGNITUDES = ORDINARY + LARGE
SEAM_MPW = 3
GRAY_AS_RGB = (3, 4, 5, 6)
VISIBLE = {1: (0, 1, 2), 2: (0, 1, 2), 3: (0, 2), 4: (0, 1, 2), 5: (0, 1), 6: (0,), 7: (1,), 8: (2,)}      # components (Y, Cb, Cr) a mode's pixels depend on

_PICS = {}


def picture(H, name):
    """The picture of a layout, built once per process.  `data` / `parsed` are what harness.drive takes; `oracle_data` is the same for every
    picture but the progressive one, where it is the baseline file of the same coefficients (the oracle refuses SOF2)."""
    if name in _PICS:
        return _PICS[name]
    kw, samp, (mw, mh) = LAYOUTS[name]
    if name == "prog420":
        import prog_cases as PC
        fr = PC.frame_of("2x2", kw["width"], kw["height"])
        c = PC.Case(name, fr, PC.noise(fr, kw["seed"]), PC.script_standard(3)).build()
        data, parsed, oracle_data, prog = c.file, None, c.base, True
    else:
        data = H.synth_jpeg(quality=QUALITY, **kw)
        parsed = H.parse_jpeg(data)
        if samp:
            parsed.comps = [(c[0], h, v, c[3]) for c, (h, v) in zip(parsed.comps, samp)]
        oracle_data, prog = data, False
    assert (-(-kw["width"] // mw), -(-kw["height"] // mh)) == (XMAX, YMAX) and kw["width"] % mw and kw["height"] % mh, name
    _PICS[name] = Picture(name, data, parsed, oracle_data, mw, mh, XMAX, YMAX, prog)
    return _PICS[name]


def oracle_drive(H, oracle, pic):
    """The picture through the oracle (the progressive one: its baseline twin)."""
    H.drive(oracle, pic.oracle_data, None if pic.progressive else pic.parsed)


def starts(xmax=XMAX, ymax=YMAX, mpw=SEAM_MPW):
    """label -> (shift_mcu_x, shift_mcu_y)."""
    nmcu = xmax * ymax
    wgs = wgs_of(nmcu, mpw)
    per = -(-nmcu // wgs)
    assert wgs >= 2 and per > 8
    xy = lambda i: (i % xmax, i // xmax)
    strided_first = 8 + 3                                         # wave 3 of workgroup 1 (back_end_mcus)
    strided_last = strided_first + (nmcu - 1 - strided_first) // (8 * wgs) * (8 * wgs)
    out = {
        "all": (0, 0), "last_mcu": (xmax - 1, ymax - 1), "at_nmcu": (0, ymax), "x_past_the_row": (xmax + 2, 0), "middle": (5, 2),
        "general_wave_first": xy(strided_first), "general_wave_last": xy(strided_last), "general_second_workgroup": xy(8),
        "range_wave_first": xy(per + 3), "range_last": xy(min(2 * per, nmcu) - 1), "range_second_workgroup": xy(per),
    }
    assert strided_last > strided_first and len(set(out.values())) == len(out)
    return out


def start_index(state, xmax=XMAX):
    return state[2] * xmax + state[1]


def inside(state, xmax=XMAX, ymax=YMAX):
    return start_index(state, xmax) < xmax * ymax


def inert(layout, state):
    """True where the state cannot change a pixel of this layout's picture against the same mode without the shift (module docstring)."""
    shift = state[3:6]
    seen = [c for c in VISIBLE[state[0]] if shift[c]]
    if layout == "gray":
        seen = [c for c in seen if c == 0 or not 0 <= shift[c] < 8]
    return not seen


def shows_rgb(layout, mode):
    """True where the mode's rendering must EQUAL mode 1's: a grey picture has Cb = Cr = 0, so R = 0 * k + Y and B likewise are exactly Y,
    and G = (Y - 0.114 Y - 0.299 Y) / 0.587 comes back to Y within the truncation on every sample of the picture: PREVIEW_R, _G, _B and _Y
    show what PREVIEW_RGB shows.  Everywhere else the census demands a difference."""
    return mode == 1 or (layout == "gray" and mode in GRAY_AS_RGB)


def _build():
    names = list(LAYOUTS)
    st = starts()
    inner = [v for k, v in st.items() if k not in ("at_nmcu",)]
    wide = [v for k, v in st.items() if k not in ("at_nmcu", "last_mcu")]         # (the large magnitudes need a sample far out among the shifted ones)
    cases = []
    for li, name in enumerate(names):
        for m in MODES:
            cases.append(Case(name, (m, 0, 0, 0, 0, 0)))
        # every start under mode 1 with a magnitude the picture can show: grey has no use for a chroma shift below one output step
        mags = [g for g in ORDINARY if not inert(name, (1, 0, 0) + g)]
        for k, (label, (sx, sy)) in enumerate(st.items()):          # (one MCU alone: the magnitude that moves every pixel of any content)
            cases.append(Case(name, (1, sx, sy) + (ORDINARY[4] if label == "last_mcu" else mags[(li + k) % len(mags)])))
    for k, (mag, mode) in enumerate((mag, mode) for mag in ORDINARY for mode in MODES):
        sx, sy = inner[(k // len(names) * 3 + k) % len(inner)]
        cases.append(Case(names[k % len(names)], (mode, sx, sy) + mag))
    for k, (mag, mode) in enumerate((mag, mode) for mag in LARGE for mode in MODES):
        sx, sy = wide[(3 * k + 1) % len(wide)]
        cases.append(Case(PARTIAL[(k + k // len(MODES)) % 2], (mode, sx, sy) + mag))
    return list(dict.fromkeys(cases))                                # (a mode-1 combination may repeat a start case)


CASES = _build()


def cases_of(layout):
    return [c.state for c in CASES if c.layout == layout]


def assert_crossing(cases=CASES):
    names, st = set(LAYOUTS), set(starts().values())
    assert {(c.layout, c.state[0]) for c in cases} >= {(n, m) for n in names for m in MODES}, "every layout meets every mode"
    assert {(c.layout, c.state[1:3]) for c in cases if not inert(c.layout, c.state)} >= {(n, s) for n in names for s in st}, "every layout meets every start"
    assert {(c.state[3:], c.state[0]) for c in cases} >= {(g, m) for g in MAGNITUDES for m in MODES}, "every magnitude meets every mode"
    assert {c.layout for c in cases if c.state[0] != 1 and any(c.state[3:]) and inside(c.state)} == names, "every layout meets a mode other than 1 with a shift"
    assert {c.state[3:] for c in cases if any(c.state[3:])} == set(MAGNITUDES)
    assert all(c.layout in PARTIAL for c in cases if c.state[3:] in LARGE)
    assert len(set(cases)) == len(cases)


assert_crossing()
