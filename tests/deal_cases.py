"""The unit deal that ten kernels copy, restated and simulated -- TEST INFRASTRUCTURE behind tests/test_deal_cases.py (CPU) and one GPU test in each of
test_gpu_encode.py, test_gpu_transform.py, test_gpu_coefs.py, test_gpu_batch_stats.py, test_gpu_coef_hist.py, test_gpu_pack_ijg.py and
test_gpu_pack_ijg_scaled.py: seven kernels have a test sized here; k_pack_rgb, k_pack_planes and k_pack_resize rely on their 1080p tests.

A launcher lays the units of all records of a call end to end over a prefix table and gives a workgroup a contiguous share of
S = ceil(T / min(F * cus, ceil(T / W))) units.  In k_encode, k_transform, k_pack_coefs, k_stats_batch, k_render_ijg and k_render_ijg_scaled wave w takes units
u0 + w, u0 + w + W, ...: it finds the record of its first unit by a binary search and moves on with `while (u >= unit_base[k + 1]) k++`.  k_coef_hist
walks its share destination by destination, and its W waves interleave inside one destination (`by_record`).  While T <= W * F * cus a share is W units,
a wave takes one unit and none of this happens; `census` says what does happen for a given record list, and the builders below make record lists for
which everything happens on a device of `cus` compute units.

The constants, and where the sources state them (KERNELS / SOURCE; the CPU test reads the lines back):
  kernel       W                                       F (workgroups per compute unit)                 unit
  encode       jsnoop_encode.hip:35, :81               jsnoop_encode.hip:180                           jsnoop_types.h:241 JS_ENC_RUN MCUs of an MCU row
  transform    jsnoop_transform.hip:24, :67            jsnoop_transform.hip:96                         jsnoop_types.h:251 JS_XF_RUN destination blocks
  coefs        jsnoop_coef.hip:35, :93                 jsnoop_coef.hip:187 (direct / through a tile)   jsnoop_types.h:159 JS_COEF_TILE blocks of a block row
  stats        jsnoop_stats.hip:35, :126               jsnoop_stats.hip:262 (histograms / none)        jsnoop_types.h:165 JS_STATS_UNIT pixels of a picture row
  coef_hist    jsnoop_types.h:174, jsnoop_coef_hist.hip:83   jsnoop_types.h:175                        jsnoop_types.h:173 JS_COEF_HIST_UNIT blocks, arena order
  render       jsnoop_render.hip:31, :129              jsnoop_render.hip:219                           jsnoop_render_check.h:71 JS_REN_RUN MCUs of an MCU row
  render_scaled  jsnoop_render_scaled.hip:26, :138     jsnoop_render_scaled.hip:176                    jsnoop_render_scaled_check.h:135 js_rs_run: 64 reduced pixels of an MCU row

The two renders keep the most in LDS from unit to unit (luma rectangle, chroma planes with halo columns and rows, transpose tile, workspace), and what a
unit leaves there depends on its picture's layout.  Their lists are therefore also asked for ADJACENT: which kind of unit a wave takes directly behind
which (`adjacency_missing` walks the simulated wave order; the builders search until it is empty and assert it).

A record list is built from about a dozen distinct pictures: a few long ones that carry the volume and short ones of 1, 2, 3 and 5 units (k_stats_batch:
block rows, a record is never less than eight picture rows) between them, among them a stretch of one-unit records several shares long.  A builder
returns [Rec]; `pic` names the picture (a tuple the GPU test turns into a file, a tensor or a (file, component) pair), `sizes` the size of each of
its units, None where the call refuses the entry and it gets no record."""
from __future__ import annotations

import bisect
from types import SimpleNamespace

import ijg_cases as IC
import transform_model as TM

KERNELS = {
    "encode": dict(waves=4, per_cu={"any": 4}, unit=8, by_record=False),
    "transform": dict(waves=4, per_cu={"any": 8}, unit=8, by_record=False),
    "coefs": dict(waves=4, per_cu={"direct": 8, "tiled": 5}, unit=64, by_record=False),
    "stats": dict(waves=4, per_cu={"hist": 4, "plain": 8}, unit=512, by_record=False),
    "coef_hist": dict(waves=8, per_cu={"any": 2}, unit=64, by_record=True),
    "render": dict(waves=4, per_cu={"any": 6}, unit=8, by_record=False),
    "render_scaled": dict(waves=4, per_cu={"any": 6}, unit=64, by_record=False),
}
# (file, line, text of that line) per kernel, written with the numbers of KERNELS
_K = KERNELS
SOURCE = {
    "encode": [("jsnoop_encode.hip", 34, "#define EN_THREADS %d" % (64 * _K["encode"]["waves"])), ("jsnoop_encode.hip", 35, "#define EN_WAVES   (EN_THREADS / 64)"),
               ("jsnoop_encode.hip", 81, "for (; u < u1; u += EN_WAVES)"), ("jsnoop_encode.hip", 83, "while (u >= unit_base[k + 1]) k++;"),
               ("jsnoop_encode.hip", 180, "std::min<uint64_t>((uint64_t)cus * %du, ((uint64_t)total_units + EN_WAVES - 1u) / EN_WAVES)" % _K["encode"]["per_cu"]["any"]),
               ("jsnoop_types.h", 241, "#define JS_ENC_RUN %du" % _K["encode"]["unit"])],
    "transform": [("jsnoop_transform.hip", 23, "#define XF_THREADS %d" % (64 * _K["transform"]["waves"])), ("jsnoop_transform.hip", 24, "#define XF_WAVES   (XF_THREADS / 64)"),
                  ("jsnoop_transform.hip", 67, "for (; u < kend; u += XF_WAVES)"), ("jsnoop_transform.hip", 64, "while (u >= unit_base[k + 1]) k++;"),
                  ("jsnoop_transform.hip", 96, "std::min<uint64_t>((uint64_t)cus * %du, ((uint64_t)total_units + XF_WAVES - 1u) / XF_WAVES)" % _K["transform"]["per_cu"]["any"]),
                  ("jsnoop_types.h", 251, "#define JS_XF_RUN %du" % _K["transform"]["unit"])],
    "coefs": [("jsnoop_coef.hip", 34, "#define CF_THREADS %d" % (64 * _K["coefs"]["waves"])), ("jsnoop_coef.hip", 35, "#define CF_WAVES   (CF_THREADS / 64)"),
              ("jsnoop_coef.hip", 93, "for (; u < u1; u += CF_WAVES)"), ("jsnoop_coef.hip", 95, "while (u >= unit_base[k + 1]) k++;"),
              ("jsnoop_coef.hip", 187, "(uint64_t)cus * (direct ? %du : %du), ((uint64_t)total_units + CF_WAVES - 1u) / CF_WAVES)" % (_K["coefs"]["per_cu"]["direct"], _K["coefs"]["per_cu"]["tiled"])),
              ("jsnoop_types.h", 159, "#define JS_COEF_TILE %du" % _K["coefs"]["unit"])],
    "stats": [("jsnoop_stats.hip", 34, "#define SB_THREADS %d" % (64 * _K["stats"]["waves"])), ("jsnoop_stats.hip", 35, "#define SB_WAVES   (SB_THREADS / 64)"),
              ("jsnoop_stats.hip", 126, "for (; u < u1; u += SB_WAVES)"), ("jsnoop_stats.hip", 129, "while (u >= unit_base[k + 1]) k++;"),
              ("jsnoop_stats.hip", 262, "(uint64_t)cus * (hist_en ? %du : %du), (total_units + SB_WAVES - 1u) / SB_WAVES)" % (_K["stats"]["per_cu"]["hist"], _K["stats"]["per_cu"]["plain"])),
              ("jsnoop_types.h", 165, "#define JS_STATS_UNIT %du" % _K["stats"]["unit"])],
    "coef_hist": [("jsnoop_types.h", 174, "#define JS_COEF_HIST_WAVES %du" % _K["coef_hist"]["waves"]), ("jsnoop_coef_hist.hip", 33, "#define CH_WAVES   JS_COEF_HIST_WAVES"),
                  ("jsnoop_coef_hist.hip", 83, "for (uint32_t lu = lu0 + wave; lu < lu1; lu += CH_WAVES)"), ("jsnoop_coef_hist.hip", 72, "while (s0 >= unit_base[k + 1]) k++;"),
                  ("jsnoop_types.h", 175, "#define JS_COEF_HIST_WG_PER_CU %du" % _K["coef_hist"]["per_cu"]["any"]),
                  ("jsnoop_coef_hist.hip", 154, "(uint64_t)cus * std::min(JS_COEF_HIST_WG_PER_CU, CH_LDS_PER_CU / lds), (total_units + CH_WAVES - 1u) / CH_WAVES)"),
                  ("jsnoop_types.h", 173, "#define JS_COEF_HIST_UNIT %du" % _K["coef_hist"]["unit"])],
    "render": [("jsnoop_render.hip", 30, "#define RN_THREADS %d" % (64 * _K["render"]["waves"])), ("jsnoop_render.hip", 31, "#define RN_WAVES   (RN_THREADS / 64)"),
               ("jsnoop_render.hip", 129, "for (; u < u1; u += RN_WAVES)"), ("jsnoop_render.hip", 131, "while (u >= unit_base[k + 1]) k++;"),
               ("jsnoop_render.hip", 219, "std::min<uint64_t>((uint64_t)cus * %du, ((uint64_t)total_units + RN_WAVES - 1u) / RN_WAVES)" % _K["render"]["per_cu"]["any"]),
               ("jsnoop_render_check.h", 71, "#define JS_REN_RUN      %du" % _K["render"]["unit"])],
    "render_scaled": [("jsnoop_render_scaled.hip", 25, "#define RS_THREADS %d" % (64 * _K["render_scaled"]["waves"])), ("jsnoop_render_scaled.hip", 26, "#define RS_WAVES   (RS_THREADS / 64)"),
                      ("jsnoop_render_scaled.hip", 138, "for (; un < u1; un += RS_WAVES)"), ("jsnoop_render_scaled.hip", 140, "while (un >= unit_base[k + 1]) k++;"),
                      ("jsnoop_render_scaled.hip", 176, "std::min<uint64_t>((uint64_t)cus * %du, ((uint64_t)total_units + RS_WAVES - 1u) / RS_WAVES)" % _K["render_scaled"]["per_cu"]["any"]),
                      ("jsnoop_render_scaled_check.h", 135, "inline uint32_t js_rs_run(uint32_t H, uint32_t m) { return %du / (H * m); }" % _K["render_scaled"]["unit"])],
}
CUS = (64, 104, 228, 256, 304)                                      # the devices the CPU test proves the builders for


# ------------------------------------------------------------------------------------------------------------------ the grid rule and the walk
def share(total_units, cus, per_cu, waves):
    """Units of one workgroup's contiguous share: never more workgroups than per_cu * cus, nor than there are steps of `waves` units."""
    want = min(per_cu * cus, -(-total_units // waves))
    return -(-total_units // want)


def census(unit_counts, cus, per_cu, waves, sizes=None, full=None, by_record=False):
    """What the walk over records of unit_counts[k] >= 1 units does.  sizes: one number per unit of the call, `full` the size of a full unit.

    S, total, grid     the share, the units of the call, the workgroups
    wave_units         [workgroup][wave]: units the wave takes;  min_full: the least of them over the workgroups with a whole share;  best_full: the
                       most that every wave of one such workgroup takes
    max_skip           most records one step of a wave passes over without taking a unit of them (always 0 by_record: the share goes record by record)
    carried_then_left  a wave takes two or more consecutive units of one record and then one of another record
    start_inside, start_on_boundary   some share but the first starts strictly inside a record; some share but the first starts on a record's first unit
    last_ragged        the last share is shorter than S
    narrow_after_full  a wave takes a unit smaller than `full` directly after a full one (None without sizes)
    max_held, max_span most records one share holds units of; most shares one record has units in;  longest: the units of the longest record"""
    counts = [int(n) for n in unit_counts]
    assert counts and min(counts) >= 1
    base = [0]
    for n in counts:
        base.append(base[-1] + n)
    T = base[-1]
    S = share(T, cus, per_cu, waves); grid = -(-T // S)
    rec = lambda u: bisect.bisect_right(base, u) - 1
    if sizes is not None:
        assert len(sizes) == T and full is not None
    c = SimpleNamespace(S=S, total=T, grid=grid, wave_units=[], max_skip=0, carried_then_left=False, start_inside=False, start_on_boundary=False, last_ragged=T % S != 0,
                        narrow_after_full=None if sizes is None else False, max_held=0, max_span=0)
    for g in range(grid):
        u0, u1 = g * S, min(T, g * S + S)
        k0, k1 = rec(u0), rec(u1 - 1)
        c.max_held = max(c.max_held, k1 - k0 + 1)
        if g and base[k0] == u0:
            c.start_on_boundary = True
        if g and base[k0] < u0:
            c.start_inside = True
        taken = []
        for w in range(waves):
            if by_record:                                           # the wave's units, in the order it takes them
                walk = [u for k in range(k0, k1 + 1) for u in range(max(u0, base[k]) + w, min(u1, base[k + 1]), waves)]
            else:
                walk = list(range(u0 + w, u1, waves))
            taken.append(len(walk))
            run, prev = 0, None
            for u in walk:
                k = rec(u)
                if prev is None or k == rec(prev):
                    run += 1
                else:
                    if not by_record:
                        c.max_skip = max(c.max_skip, k - rec(prev) - 1)
                    if run >= 2:
                        c.carried_then_left = True
                    run = 1
                if sizes is not None and prev is not None and sizes[prev] == full and sizes[u] < full:
                    c.narrow_after_full = True
                prev = u
        c.wave_units.append(taken)
    full_shares = [t for g, t in enumerate(c.wave_units) if g * S + S <= T]
    c.min_full = min(min(t) for t in full_shares); c.best_full = max(min(t) for t in full_shares)
    c.longest = max(counts)
    c.max_span = max((base[k + 1] - 1) // S - base[k] // S + 1 for k in range(len(counts)))
    return c


def missing(c, waves, narrow=False, skip=3, held=0, span=0):
    """The conditions of the GPU tests that census `c` does not meet, by name (none: []).  skip: records one step must pass over; held: records one share
    must hold; span: shares one record must have units in, and the longest record must be 3 S units or more (the last two where no step can skip)."""
    out = []
    if not (c.S >= 3 * waves and (c.best_full if span else c.min_full) >= 3):    # (record by record a wave has nothing to take of a one-unit record)
        out.append("S >= 3 W")
    if c.max_skip < skip:
        out.append("a step skips %d records" % skip)
    if c.max_held < held:
        out.append("a share holds %d records" % held)
    if not c.carried_then_left:
        out.append("units of one record carried, then left")
    if not (c.start_inside and c.start_on_boundary):
        out.append("share starts inside records and on their boundaries")
    if not c.last_ragged:
        out.append("a ragged last share")
    if narrow and not c.narrow_after_full:
        out.append("a narrow unit after a full one")
    if span and (c.max_span < span or c.longest < 3 * c.S):
        out.append("a record of 3 S units over %d shares" % span)
    return out


def summary(c):
    """The asserted figures in one line (the GPU tests print it)."""
    flat = [n for t in c.wave_units[:-1] for n in t] or [0]
    return "T = %d units, grid %d, S = %d, units per wave %d..%d (last share %s), records skipped by one step <= %d, records in one share <= %d, shares of one record <= %d" % (
        c.total, c.grid, c.S, min(flat), max(flat), c.wave_units[-1], c.max_skip, c.max_held, c.max_span)


# ------------------------------------------------------------------------------------------------------------------ record lists
class Rec:
    def __init__(self, pic, sizes):
        self.pic, self.sizes = pic, sizes if isinstance(sizes, list) else None
        self.units = len(sizes) if isinstance(sizes, list) else 0


def _arrange(shorts, longs, refused, n_long, tail, waves, prelude=()):
    """pictures -> the order of the call.  shorts: {units: [pic]} with 1 (STEP for stats), 2, 3 and 5 (times STEP); the first long record, a stretch of
    12 W smallest records, a long one, every short one three times over, the `prelude` as it stands, then long ones with five short ones behind every
    third, `tail` smallest ones."""
    small = sorted(shorts)
    ones = shorts[small[0]]; every = [p for n in small for p in shorts[n]]
    seq = [longs[0]] + [ones[i % len(ones)] for i in range(12 * waves)] + [longs[1 % len(longs)]]
    for i in range(3 * len(every)):
        seq.append(every[i % len(every)])
        if refused and i % 4 == 1:
            seq.append(refused[(i // 4) % len(refused)])
    seq += list(prelude)
    for i in range(n_long):
        seq.append(longs[(i + 2) % len(longs)])
        if i % 3 == 2:
            seq += [every[(5 * i + j) % len(every)] for j in range(5)]
    return seq + [ones[(i + 1) % len(ones)] for i in range(tail)]


def _pick(cands, sizes_of, wanted, full, per=2):
    """{units: up to `per` of the candidates with that many units, those with a unit below `full` first}, [refused candidates], one per reason."""
    shorts, refused = {n: [] for n in wanted}, []
    for narrow_first in (True, False):
        for p in cands:
            s = sizes_of(p)
            if not isinstance(s, list):                             # refused, `s` says why: one candidate per reason
                if s not in [sizes_of(q) for q in refused]:
                    refused.append(p)
            elif len(s) in shorts and len(shorts[len(s)]) < per and p not in shorts[len(s)] and (min(s) < full) == narrow_first:
                shorts[len(s)].append(p)
    assert all(shorts[n] for n in wanted), {n: len(v) for n, v in shorts.items()}
    return shorts, refused


def _build(kernel, form, cus, cands, longs, sizes_of, wanted=(1, 2, 3, 5), per=2, prelude=(), also=None):
    """also(recs, cus) -> further conditions the list does not meet, by name: searched for like those of `missing`."""
    K = KERNELS[kernel]; W = K["waves"]; F = K["per_cu"][per_cu_form(kernel, form)]; need = conditions(kernel, form)
    shorts, refused = _pick(cands, sizes_of, wanted, K["unit"], per)
    size = {p: sizes_of(p) for p in set(cands) | set(longs) | set(prelude)}
    assert all(isinstance(size[p], list) and len(size[p]) >= 4 * 3 * W for p in longs), "a long record is more than three shares"
    fixed = sum(len(size[p]) for p in _arrange(shorts, longs, [], 0, 0, W, prelude))          # (without the refused entries)
    per_long = sum(len(size[p]) for p in longs) / len(longs)
    first = max(0, int(((3 * W - 1) * F * cus - fixed) / per_long) - 1)
    for n_long in range(first, first + 12):
        for tail in range(3 * W):
            recs = [Rec(p, size[p]) for p in _arrange(shorts, longs, refused, n_long, tail, W, prelude)]
            c = census_of(kernel, form, recs, cus)
            lacks = missing(c, W, **need)
            if not lacks and also is not None:
                lacks = also(recs, cus)
            if not lacks:
                return recs
    raise AssertionError("%s %s at %d compute units: no list meets the conditions, last: %s" % (kernel, form, cus, lacks))


def census_of(kernel, form, recs, cus):
    """The census of a builder's list on a device of `cus` compute units (refused entries have no record)."""
    K = KERNELS[kernel]
    live = [r for r in recs if r.sizes is not None]
    return census([r.units for r in live], cus, K["per_cu"][per_cu_form(kernel, form)], K["waves"], [s for r in live for s in r.sizes], K["unit"], K["by_record"])


def conditions(kernel, form):
    """The keywords of `missing` for a kernel form: what the form can meet at all.
    k_stats_batch: a record is at least eight picture rows, two steps of four units, so no step passes over a record -- a share must hold three records; a
    unit's size changes nothing.  k_coef_hist: a share is walked record by record, `k++` once a record -- a share must hold four records, a record of 3 S
    units or more must have units in three shares.  The direct form of k_pack_coefs and the non-transposing k_transform keep nothing in LDS from unit to
    unit: no narrow unit is asked for.  The two renders reuse all of a wave's LDS: a narrow unit, and `adjacency_missing` besides."""
    return {"render": dict(narrow=True), "render_scaled": dict(narrow=True), "encode": dict(narrow=True), "transform": dict(narrow=form == "turned"), "coefs": dict(narrow=form == "tiled"), "stats": dict(skip=0, held=3),
            "coef_hist": dict(skip=0, held=4, span=3)}[kernel]


def per_cu_form(kernel, form):
    """The key of KERNELS[kernel]["per_cu"] a builder form runs under."""
    return form if form in KERNELS[kernel]["per_cu"] else "any"


# ---- k_encode: pic = ("grey" | "colour", width, height); form "420" (a mixed call) or "422"
def encode_sizes(pic, form):
    kind, w, h = pic
    mw = 8 if kind == "grey" else 16; mh = 16 if (kind == "colour" and form == "420") else 8
    mx, my = -(-w // mw), -(-h // mh); runs = -(-mx // 8)
    return ([8] * (runs - 1) + [mx - 8 * (runs - 1)]) * my


ENCODE_SHORT = [(k, w, h) for h in (8, 13, 16, 24, 40, 33, 48, 80) for w in (8, 5, 17, 130, 72, 64, 128) for k in ("grey", "colour")]
ENCODE_LONG = [("grey", 8, 8 * 509), ("colour", 16, 16 * 401), ("grey", 133, 8 * 101), ("colour", 270, 16 * 67 - 3)]


def encode_records(cus, form="420"):
    return _build("encode", form, cus, ENCODE_SHORT, ENCODE_LONG, lambda p: encode_sizes(p, form))


# ---- k_transform: pic = (layout of transform_cases.LAYOUTS, width, height); form "plain" (flip_v, trim) or "turned" (rot90, a crop, edge = "perfect")
TRANSFORM_FORMS = {"plain": dict(op="flip_v"), "turned": dict(op="rot90", edge="perfect", crop=(16, 16, 1000, 100000))}
_HV = {"grey": [(1, 1)], "4:4:4": [(1, 1)] * 3, "4:2:2": [(2, 1), (1, 1), (1, 1)], "4:2:0": [(2, 2), (1, 1), (1, 1)]}


def transform_sizes(pic, form):
    layout, w, h = pic; hv = _HV[layout]; o = TRANSFORM_FORMS[form]; op = TM.OPS[o["op"]]
    mw, mh = 8 * max(a for a, _ in hv), 8 * max(b for _, b in hv)
    res, reg = TM.region(w, h, mw, mh, op, {"trim": TM.TRIM, "perfect": TM.PERFECT}[o.get("edge", "trim")], o.get("crop"))
    if res != TM.OK:
        return res                                                  # no list: the entry is refused and gets no record
    mx = reg[2] // mw if op in TM.REVERSES_X else -(-reg[2] // mw); my = reg[3] // mh if op in TM.REVERSES_Y else -(-reg[3] // mh)
    n = mx * my * sum(a * b for a, b in hv)
    return [8] * (n // 8) + ([n % 8] if n % 8 else [])


TRANSFORM_SHORT = [(l, w, h) for w in (8, 16, 24, 30, 32, 40, 48, 56) for h in (8, 16, 24, 20, 32, 40, 48, 56, 64) for l in ("grey", "4:2:0", "4:4:4", "4:2:2")]
TRANSFORM_LONG = [("grey", 80, 16 + 8 * 200), ("4:2:0", 64, 16 + 16 * 61), ("4:2:2", 48, 16 + 8 * 160)]


def transform_records(cus, form):
    return _build("transform", form, cus, TRANSFORM_SHORT, TRANSFORM_LONG, lambda p: transform_sizes(p, form))


# ---- k_pack_coefs: pic = (LAYOUTS index of test_gpu_coefs.py, width, height, component); form "direct" or "tiled"
def _grid(layout, w, h, comp):
    hs, vs = {0: (1, 1), 1: (2, 1), 2: (2, 2), 3: (1, 2), 4: (1, 1)}[layout]
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    return (mx * hs, my * vs) if comp == 0 else (mx, my)


def coefs_sizes(pic, form=None):
    bw, bh = _grid(*pic); tiles = -(-bw // 64)
    return ([64] * (tiles - 1) + [bw - 64 * (tiles - 1)]) * bh


COEFS_SHORT = [(l, w, h, c) for h in (8, 16, 24, 40, 80) for w in (8, 24, 512, 520, 1032) for l, c in ((4, 0), (2, 1), (2, 0), (0, 2))]
COEFS_LONG = [(4, 8, 8 * 1000, 0), (2, 16, 16 * 300, 0), (4, 1032, 8 * 33, 0), (2, 16, 16 * 300, 2)]


def coefs_records(cus, form):
    return _build("coefs", form, cus, COEFS_SHORT, COEFS_LONG, coefs_sizes)


# ---- k_stats_batch: pic = (layout of stats_cases.LAYOUTS, width, height); a record is the picture's MCU-padded rows; form "hist" or "plain"
def stats_sizes(pic, form=None):
    layout, w, h = pic
    mw, mh = {"gray": (8, 8), "444": (8, 8), "420": (16, 16), "422": (16, 8)}[layout]
    img_x, img_y = -(-w // mw) * mw, -(-h // mh) * mh
    tiles = -(-img_x // 512)
    return ([512] * (tiles - 1) + [img_x - 512 * (tiles - 1)]) * img_y


STATS_STEP = 8                                                      # picture rows of a block row: the least a record can have
STATS_SHORT = [(l, w, h) for h in (8, 16, 24, 40) for w in (8, 16) for l in ("gray", "444", "420", "422")]
STATS_LONG = [("gray", 8, 8 * 100), ("420", 16, 16 * 30), ("444", 8, 8 * 60), ("gray", 520, 8 * 20)]


def stats_records(cus, form):
    return _build("stats", form, cus, STATS_SHORT, STATS_LONG, stats_sizes, wanted=tuple(STATS_STEP * n for n in (1, 2, 3, 5)))


# ---- k_coef_hist: pic = (LAYOUTS index of test_gpu_coef_hist.py, width, height, component); the units of a component's blocks in arena order
def coef_hist_sizes(pic, form=None):
    layout, w, h, comp = pic
    bw, bh = _grid(layout, w, h, comp); n = bw * bh
    return [64] * (n // 64) + ([n % 64] if n % 64 else [])


COEF_HIST_SHORT = [(l, w, h, c) for w, h in ((8, 8), (64, 64), (24, 16), (72, 64), (65, 9), (104, 80), (128, 96), (160, 120), (100, 200)) for l, c in ((4, 0), (2, 1), (2, 0), (0, 2))]
COEF_HIST_LONG = [(4, 640, 640, 0), (2, 768, 512, 0)]               # (two pictures: the oracle's decode and the model's bins of these are the test's time)


def coef_hist_records(cus, form="any"):
    return _build("coef_hist", "any", cus, COEF_HIST_SHORT, COEF_HIST_LONG, coef_hist_sizes)


# ---- k_render_ijg, k_render_ijg_scaled: pic = (mode of ijg_cases.MODES, width, height); denom 1 is the full-size render, 2 | 4 | 8 the scaled one
def render_grid(pic, denom=1):
    """(H, V, MCUs across, MCU rows, MCUs of a full run, runs of an MCU row): js_ren_units / js_rs_units are rows * runs."""
    mode, w, h = pic; H, V = IC.HV[mode][0]
    mx, my = -(-w // (8 * H)), -(-h // (8 * V))
    run = KERNELS["render"]["unit"] if denom == 1 else KERNELS["render_scaled"]["unit"] // (H * (8 // denom))
    return H, V, mx, my, run, -(-mx // run)


def render_sizes(pic):
    """The MCUs of every unit of the picture."""
    _H, _V, mx, my, run, runs = render_grid(pic)
    return ([run] * (runs - 1) + [mx - run * (runs - 1)]) * my


def render_scaled_sizes(pic, denom):
    """The reduced pixels (MCU-padded) every unit of the picture is wide: nm * H * m."""
    H, _V, mx, my, run, runs = render_grid(pic, denom); m = 8 // denom
    return ([run * H * m] * (runs - 1) + [(mx - run * (runs - 1)) * H * m]) * my


def render_chroma(pic, denom=1):
    """(the width in samples the chroma filter clamps to, whether the picture's units are filtered horizontally).  Full size: dw = ceil(X / H), H = 2 is
    filtered from dw = 3 on and replicated below (js_ren_chroma4).  Scaled: 4:2:2 alone at denom 2 and 4, dwc = ceil(X nc / 16) with nc = m (js_rs_chroma4)."""
    mode, w, _h = pic; H, V = IC.HV[mode][0]
    if denom == 1:
        dw = -(-w // H)
        return dw, mode != "grey" and H == 2 and dw > 2
    m = 8 // denom; dw = -(-w * m // 16)
    return dw, mode == "422" and m > 1 and dw > 2


def render_filters(denom):
    return denom in (1, 2, 4)                                       # (at denom 8 nothing is filtered: 4:2:2 chroma is replicated)


ADJACENT = ("a grey unit behind a colour unit", "a 4:4:4 unit behind a 4:2:0 unit", "a 4:2:0 unit behind a 4:2:2 unit", "a first MCU row behind an interior unit of 4:2:0",
            "a last MCU row behind an interior unit of 4:2:0", "a chroma width of 2 or less behind a filtered unit", "a chroma width of 3 behind a filtered unit")


def _kinds(pic, denom):
    """Per unit of the picture what the adjacency conditions ask of it: (mode, interior row of 4:2:0, first row of 4:2:0, last row of 4:2:0, filtered, chroma width)."""
    mode = pic[0]; H, _V, _mx, my, _run, runs = render_grid(pic, denom); dw, filtered = render_chroma(pic, denom)
    narrow = dw if (H == 2 and (denom == 1 or mode == "422")) else 0
    tall = mode == "420" and my >= 2
    return [(mode, mode == "420" and my >= 3 and 0 < y < my - 1, tall and y == 0, tall and y == my - 1, filtered, narrow) for y in range(my) for _ in range(runs)]


def wave_steps(recs, cus, kernel, form="any", S=None):
    """Every (record, unit of it) -> (record, unit of it) one wave of the simulated deal takes directly one behind the other (S: a share given, not worked out)."""
    K = KERNELS[kernel]; W = K["waves"]
    live = [r for r in recs if r.sizes is not None]
    where = [(k, lu) for k, r in enumerate(live) for lu in range(r.units)]
    T = len(where); S = S or share(T, cus, K["per_cu"][per_cu_form(kernel, form)], W)
    return [(where[u], where[u + W]) for u in range(T - W) if u // S == (u + W) // S]


def adjacency_missing(recs, cus, denom=1):
    """The entries of ADJACENT no wave of the deal meets, for k_render_ijg (denom 1) or k_render_ijg_scaled."""
    kernel = "render" if denom == 1 else "render_scaled"
    live = [r for r in recs if r.sizes is not None]
    kinds = {r.pic: _kinds(r.pic, denom) for r in live}
    met = set()
    for (k, lu), (j, lv) in wave_steps(recs, cus, kernel):
        a, b = kinds[live[k].pic][lu], kinds[live[j].pic][lv]
        if a[0] != "grey" and b[0] == "grey":
            met.add(ADJACENT[0])
        if a[0] == "420" and b[0] == "444":
            met.add(ADJACENT[1])
        if a[0] == "422" and b[0] == "420":
            met.add(ADJACENT[2])
        if a[1] and b[2]:
            met.add(ADJACENT[3])
        if a[1] and b[3]:
            met.add(ADJACENT[4])
        if a[4] and 0 < b[5] <= 2:
            met.add(ADJACENT[5])
        if a[4] and b[5] == 3:
            met.add(ADJACENT[6])
    asked = ADJACENT[:5] + (ADJACENT[5:6] if denom == 1 else ADJACENT[5:] if render_filters(denom) else ())
    return [name for name in asked if name not in met]


def render_pictures(denom=1):
    """(short candidates, long pictures, prelude).  `px(mode)` is the width in pixels of a full unit: widths are stated in it, so the lists have the same units at
    every denominator.  One-unit pictures: a 4:2:2 one whose chroma plane is two samples wide, a grey one that fills its unit, and one whose chroma plane is
    two (4:2:0, full size) or three (4:2:2, scaled) samples wide.  Long ones: two tall pictures one MCU wide, grey and 4:2:0; a 4:2:0 picture of two full runs
    and a short one, sixteen MCU rows; a 4:2:2 picture of a full and a short run; a 4:4:4 picture of one full run.  The prelude puts a long picture of one
    kind directly in front of short ones of another; in the body the tall 4:2:0 picture stands in front of the wide one."""
    px = lambda mode: 64 * IC.HV[mode][0][0] if denom == 1 else 64 * denom
    two = ("422", 4, 8) if denom == 1 else ("422", 4 * denom, 8)
    three = ("420", 3, 13) if denom == 1 else ("422", 4 * denom + denom // 2, 8)
    shorts = [two, ("grey", px("grey"), 5), three, ("420", 3, 17), ("444", px("444") + 8, 8), ("422", 2 * px("422") + 5, 8), ("grey", 13, 24), ("420", 16, 79), ("444", 20, 40)]
    tall, wide, l422 = ("420", 16, 16 * 67), ("420", 2 * px("420") + px("420") // 4 + 5, 16 * 16 - 3), ("422", px("422") + px("422") // 8 + 2, 8 * 30)
    longs = [("grey", 8, 8 * 101), tall, wide, l422, ("444", px("444"), 8 * 50)]
    prelude = [wide, ("444", 20, 40), l422, ("420", 16, 79), l422, two, three, ("grey", 13, 24), tall, ("420", 16, 79)]
    return shorts, longs, prelude


def _render_build(kernel, form, cus, denom, sizes_of):
    shorts, longs, prelude = render_pictures(denom)
    recs = _build(kernel, form, cus, shorts, longs, sizes_of, per=3, prelude=prelude, also=lambda recs, cus: adjacency_missing(recs, cus, denom))
    assert adjacency_missing(recs, cus, denom) == []
    full = KERNELS[kernel]["unit"]
    assert any(r.units >= 48 and r.sizes[:2] == [full, full] and render_grid(r.pic, denom)[5] >= 3 for r in recs), "a long picture wider than two full runs"
    assert {r.pic[0] for r in recs if r.units >= 48} == set(IC.MODES) == {r.pic[0] for r in recs if r.units <= 5}, "all four modes among the long and the short pictures"
    return recs


def render_records(cus, form="any"):
    return _render_build("render", "any", cus, 1, render_sizes)


def render_scaled_records(cus, denom):
    return _render_build("render_scaled", str(denom), cus, int(denom), lambda p: render_scaled_sizes(p, int(denom)))


def deal_place(recs, cus, kernel, form, k, lu):
    """Where the deal puts unit `lu` of live record k: for a failure message that can be read without another run."""
    K = KERNELS[kernel]; W = K["waves"]
    live = [r for r in recs if r.sizes is not None]
    T = sum(r.units for r in live); S = share(T, cus, K["per_cu"][per_cu_form(kernel, form)], W)
    u = sum(r.units for r in live[:k]) + lu; g = u // S
    return "unit %d of the call = unit %d of record %d: share %d (units %d..%d, S = %d), wave %d, its turn %d" % (u, lu, k, g, g * S, min(T, g * S + S) - 1, S, (u - g * S) % W, (u - g * S) // W)


BUILDERS = {("render", "any"): render_records, ("render_scaled", "2"): lambda cus: render_scaled_records(cus, 2), ("render_scaled", "4"): lambda cus: render_scaled_records(cus, 4),
            ("render_scaled", "8"): lambda cus: render_scaled_records(cus, 8),
            ("encode", "420"): lambda cus: encode_records(cus, "420"), ("encode", "422"): lambda cus: encode_records(cus, "422"),
            ("transform", "plain"): lambda cus: transform_records(cus, "plain"), ("transform", "turned"): lambda cus: transform_records(cus, "turned"),
            ("coefs", "direct"): lambda cus: coefs_records(cus, "direct"), ("coefs", "tiled"): lambda cus: coefs_records(cus, "tiled"),
            ("stats", "hist"): lambda cus: stats_records(cus, "hist"), ("stats", "plain"): lambda cus: stats_records(cus, "plain"),
            ("coef_hist", "any"): coef_hist_records}
