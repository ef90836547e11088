"""CPU: tests/deal_cases.py says what the kernels say and its builders make what the GPU tests assert.  The constants are read back from the sources at
the lines the catalogue names; `share` is held against capi.coef_hist_share and `census` against a word-for-word transcription of the kernels' loops;
and for every builder, on devices of 64, 104, 228, 256 and 304 compute units, every condition the GPU test of that kernel asserts is proven here, so
a catalogue that is too small for a device fails without a GPU."""
import os
import random

import pytest

import deal_cases as D

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "jpegsnoop_amd", "csrc")


def test_the_constants_are_the_kernels():
    assert sorted(D.SOURCE) == sorted(D.KERNELS)
    text = {}
    for kernel, lines in D.SOURCE.items():
        for name, line, want in lines:
            if name not in text:
                text[name] = open(os.path.join(CSRC, name)).read().split("\n")
            assert want in text[name][line - 1], (kernel, name, line, text[name][line - 1])
    # k_coef_hist's two workgroups a compute unit hold at every range: 160 KiB of LDS take two histograms of 64 * (2 * 127 + 1) words
    assert 163840 // (256 * (2 * 127 + 1)) >= D.KERNELS["coef_hist"]["per_cu"]["any"]


def test_share_is_the_grid_rule_and_capis():
    from jpegsnoop_amd import capi
    K = D.KERNELS["coef_hist"]
    assert (capi.COEF_HIST_WAVES, capi.COEF_HIST_WG_PER_CU, capi.COEF_HIST_UNIT) == (K["waves"], K["per_cu"]["any"], K["unit"])
    for cus in (1, 2, 64, 104, 228, 256, 304):
        for total in list(range(1, 70)) + [4095, 4096, 4097, 11776, 11777, 123457]:
            for R in (1, 16, 127):
                assert D.share(total, cus, K["per_cu"]["any"], K["waves"]) == capi.coef_hist_share(total, cus, R), (cus, total, R)
    # below W * F * cus units a share is W units and a wave takes one: the regime of every test but the new ones (the largest calls the suite made before)
    for kernel, form, most in (("encode", "any", 100), ("transform", "any", 3600), ("coefs", "direct", 4500), ("coefs", "tiled", 4500), ("stats", "hist", 400), ("coef_hist", "any", 100),
                               ("render", "any", 1000), ("render_scaled", "any", 1000)):
        K = D.KERNELS[kernel]
        assert most <= K["waves"] * K["per_cu"][form] * 256 and D.share(most, 256, K["per_cu"][form], K["waves"]) == K["waves"], (kernel, form)
        assert D.share(K["waves"] * K["per_cu"][form] * 256 + 1, 256, K["per_cu"][form], K["waves"]) == K["waves"] + 1


def transcription(counts, S, W, by_record):
    """The kernels' loops with their own variables (u, k, kend / s0, s1, lu): [workgroup][wave] -> [(unit, record)] in the order taken, and per wave
    the largest number of `k++` one pass through the `while` makes."""
    base = [0]
    for n in counts:
        base.append(base[-1] + n)
    T = base[-1]; nrec = len(counts); out = []; most = 0
    for g in range(-(-T // S)):
        u0, u1 = g * S, min(T, g * S + S); waves = []
        for wave in range(W):
            took = []
            if not by_record:
                u = u0 + wave
                if u < u1:
                    k, top = 0, nrec
                    while top - k > 1:
                        mid = (k + top) >> 1
                        if base[mid] <= u:
                            k = mid
                        else:
                            top = mid
                    fresh, kend = True, 0
                    while u < u1:
                        if fresh or u >= kend:
                            n = 0
                            while u >= base[k + 1]:
                                k += 1; n += 1
                            if not fresh:
                                most = max(most, n)
                            fresh, kend = False, base[k + 1]
                        took.append((u, k)); u += W
            else:
                k, top = 0, nrec
                while top - k > 1:
                    mid = (k + top) >> 1
                    if base[mid] <= u0:
                        k = mid
                    else:
                        top = mid
                s0 = u0
                while s0 < u1:
                    while s0 >= base[k + 1]:
                        k += 1
                    kbeg, s1 = base[k], min(u1, base[k + 1])
                    took += [(kbeg + lu, k) for lu in range(s0 - kbeg + wave, s1 - kbeg, W)]
                    s0 = s1
            waves.append(took)
        out.append(waves)
    return out, most


@pytest.mark.parametrize("by_record", [False, True])
def test_census_is_the_walk_of_the_kernels(by_record):
    rng = random.Random(5)
    for trial in range(60):
        W = rng.choice((4, 8)); per_cu = rng.choice((1, 2, 5)); cus = rng.choice((1, 2, 3, 7))
        counts = [rng.choice((1, 1, 1, 2, 3, 5, 8, 40)) for _ in range(rng.randrange(1, 60))]
        T = sum(counts)
        sizes = [rng.choice((3, 8)) for _ in range(T)]
        c = D.census(counts, cus, per_cu, W, sizes, 8, by_record)
        assert c.S == D.share(T, cus, per_cu, W) and c.total == T and c.grid == -(-T // c.S) and c.last_ragged == (T % c.S != 0)
        walk, most = transcription(counts, c.S, W, by_record)
        assert c.wave_units == [[len(t) for t in waves] for waves in walk]
        assert sorted(u for waves in walk for t in waves for u, _ in t) == list(range(T)), "every unit is taken once"
        skip, carried, narrow = 0, False, False
        for waves in walk:
            for t in waves:
                run = 1
                for (u, k), (v, j) in zip(t, t[1:]):
                    if j != k:
                        skip = max(skip, j - k - 1); carried |= run >= 2; run = 1
                    else:
                        run += 1
                    narrow |= sizes[u] == 8 and sizes[v] < 8
        assert (c.max_skip, c.carried_then_left, c.narrow_after_full) == (0 if by_record else skip, carried, narrow), (trial, counts, W, c.S)
        assert by_record or c.max_skip == max(0, most - 1)
        starts = [waves[0][0] for waves in walk[1:]]
        base = [sum(counts[:k]) for k in range(len(counts))]
        assert c.start_on_boundary == any(base[k] == u for u, k in starts) and c.start_inside == any(base[k] < u for u, k in starts)
        assert c.max_held == max(len({k for t in waves for _, k in t}) for waves in walk)
        assert c.max_span == max(len({u // c.S for u in range(base[k], base[k] + counts[k])}) for k in range(len(counts))) and c.longest == max(counts)


def test_census_by_hand():
    # 24 one-unit records, one compute unit, one workgroup of four waves: a share of 24, six units a wave, every step passes over three records
    c = D.census([1] * 24, 1, 1, 4)
    assert (c.S, c.grid, c.wave_units, c.max_skip, c.carried_then_left, c.last_ragged, c.narrow_after_full) == (24, 1, [[6, 6, 6, 6]], 3, False, False, None)
    assert D.missing(c, 4) == ["units of one record carried, then left", "share starts inside records and on their boundaries", "a ragged last share"]
    # records of 9, 1, 1, 1, 1, 13 units on two workgroups: S = 13; wave 0 takes units 0, 4, 8 of record 0 and then unit 12, the last one-unit record
    c = D.census([9, 1, 1, 1, 1, 13], 2, 1, 4, [8] * 8 + [2] + [8] * 17, 8)
    assert (c.S, c.grid, c.wave_units) == (13, 2, [[4, 3, 3, 3], [4, 3, 3, 3]]) and c.max_skip == 3 and c.carried_then_left and c.narrow_after_full
    assert c.start_on_boundary and not c.start_inside and not c.last_ragged and (c.max_held, c.max_span, c.min_full) == (5, 1, 3)
    # the same list record by record with eight waves: nothing is passed over; wave 0 takes two units of the first record before the share moves on
    c = D.census([9, 1, 1, 1, 1, 13], 2, 1, 8, by_record=True)
    assert (c.S, c.wave_units[0], c.max_skip, c.carried_then_left) == (13, [6, 1, 1, 1, 1, 1, 1, 1], 0, True)
    # too few units: a share of W, one unit a wave
    c = D.census([3, 1, 2, 5, 1], 256, 8, 4)
    assert c.S == 4 and c.min_full == 1 and "S >= 3 W" in D.missing(c, 4)


@pytest.mark.parametrize("key", sorted(D.BUILDERS), ids=lambda k: "%s-%s" % k)
def test_every_builder_meets_the_conditions_of_its_gpu_test(key):
    kernel, form = key; K = D.KERNELS[kernel]; W = K["waves"]; need = D.conditions(kernel, form)
    for cus in D.CUS:
        recs = D.BUILDERS[key](cus)
        c = D.census_of(kernel, form, recs, cus)
        assert D.missing(c, W, **need) == [], (cus, D.summary(c))
        assert c.total > (3 * W - 1) * K["per_cu"][D.per_cu_form(kernel, form)] * cus and c.S <= 3 * W + 3, (cus, D.summary(c))       # in the regime, and no larger than it takes
        pics = {r.pic for r in recs}
        assert len(pics) <= 16, (cus, len(pics))
        step = D.STATS_STEP if kernel == "stats" else 1
        assert {r.units for r in recs} >= {step, 2 * step, 3 * step, 5 * step}
        live = [r for r in recs if r.sizes is not None]
        assert len({r.pic for r in live if r.units >= 3 * c.S}) >= 2 and live[0].units >= 3 * c.S, "long records of several pictures; the call starts with one"
        ones = [k for k, r in enumerate(live) if r.units == step]
        stretch = max(b - a for a, b in zip([-1] + [k for k, r in enumerate(live) if r.units != step], [k for k, r in enumerate(live) if r.units != step] + [len(live)])) - 1
        assert stretch >= 10 * W and stretch * step >= 3 * c.S, "a stretch of smallest records several shares long"
        assert all(live[k].pic != live[k + 1].pic for k in ones if k + 1 < len(live)), "a smallest record differs from the record behind it"
        k_long = [k for k, r in enumerate(live) if r.units >= 3 * c.S]
        assert any(0 < k < len(live) - 1 and live[k - 1].units <= 5 * step and live[k + 1].units <= 5 * step for k in k_long), "a long record between short ones"
        if need.get("narrow"):
            assert any(min(r.sizes) < K["unit"] for r in live if r.units >= 3 * c.S) and any(max(r.sizes) == K["unit"] for r in live if r.units >= 3 * c.S)
        if kernel in ("render", "render_scaled"):
            denom = 1 if kernel == "render" else int(form)
            assert D.adjacency_missing(recs, cus, denom) == [], cus
            assert adjacency_by_the_transcription(recs, c, W, denom) >= set(D.ADJACENT[:5] + D.ADJACENT[5:{1: 6, 2: 7, 4: 7, 8: 5}[denom]]), cus
            assert {r.pic[0] for r in live if r.units >= 3 * c.S} == set(D.IC.MODES) == {r.pic[0] for r in live if r.units <= 5}, "all four modes, long and short"
            assert any(r.units >= 3 * c.S and D.render_grid(r.pic, denom)[5] >= 3 and r.sizes[:2] == [K["unit"]] * 2 for r in live), "a long picture wider than two full runs"
        refused = [k for k, r in enumerate(recs) if r.sizes is None]
        if kernel == "transform":
            assert refused and all(0 < k < len(recs) - 1 and (recs[k - 1].sizes and recs[k + 1].sizes) for k in refused), "refused entries sit among those that are OK"
            assert len({recs[k].pic for k in refused}) == (2 if form == "turned" else 1)
        else:
            assert not refused


def adjacency_by_the_transcription(recs, c, W, denom):
    """The entries of D.ADJACENT met along the kernels' own loop (`transcription`), each stated here on the pictures' numbers: a second walk beside
    D.adjacency_missing, which goes through D.wave_steps and D._kinds."""
    live = [r for r in recs if r.sizes is not None]
    walk, _most = transcription([r.units for r in live], c.S, W, False)
    base = [0]
    for r in live:
        base.append(base[-1] + r.units)
    steps = [((k, u - base[k]), (j, v - base[j])) for waves in walk for t in waves for (u, k), (v, j) in zip(t, t[1:])]
    assert sorted(steps) == sorted(D.wave_steps(recs, 0, "render", "any", S=c.S))

    def unit(k, lu):
        mode, w, h = live[k].pic; H, V = D.IC.HV[mode][0]
        rows = -(-h // (8 * V)); across = -(-w // (8 * H)); run = 8 if denom == 1 else 64 // (H * (8 // denom))
        my = lu // -(-across // run)
        if denom == 1:
            cw = -(-w // 2) if H == 2 else None                   # the chroma plane's width where chroma is upsampled horizontally
            filtered = H == 2 and cw > 2
        else:
            cw = -(-(w * (8 // denom)) // 16) if mode == "422" else None      # 4:2:2: nc = m samples per block
            filtered = mode == "422" and denom in (2, 4) and cw > 2
        return mode, my, rows, cw, filtered

    met = set()
    for a, b in steps:
        (ma, ya, ra, _ca, fa), (mb, yb, rb, cb, _fb) = unit(*a), unit(*b)
        interior = ma == "420" and ra >= 3 and 0 < ya < ra - 1
        met |= {name for name, hit in zip(D.ADJACENT, (ma != "grey" and mb == "grey", ma == "420" and mb == "444", ma == "422" and mb == "420",
                                                         interior and mb == "420" and rb >= 2 and yb == 0, interior and mb == "420" and rb >= 2 and yb == rb - 1,
                                                         fa and cb is not None and cb <= 2, fa and cb == 3)) if hit}
    return met


def test_render_sizes_are_the_unit_counts_of_the_plans():
    """js_ren_units / js_rs_units restated: mcu_ymax * ceil(mcu_xmax / run), run = JS_REN_RUN or 64 / (H m).  The GPU tests tie the counts to the batch's geometry."""
    for denom in (1, 2, 4, 8):
        shorts, longs, prelude = D.render_pictures(denom)
        assert set(prelude) <= set(shorts) | set(longs)
        for pic in shorts + longs + [(mode, w, h) for mode in D.IC.MODES for w, h in D.IC.SIZES + [(449, 33), (1025, 17)]]:
            mode, w, h = pic; H, V = D.IC.HV[mode][0]; m = 8 // denom
            mcu_xmax, mcu_ymax = (w + 8 * H - 1) // (8 * H), (h + 8 * V - 1) // (8 * V)
            run = 8 if denom == 1 else 64 // (H * m)
            sizes = D.render_sizes(pic) if denom == 1 else D.render_scaled_sizes(pic, denom)
            assert len(sizes) == mcu_ymax * ((mcu_xmax + run - 1) // run), (pic, denom)
            assert sum(sizes) == mcu_xmax * mcu_ymax * (1 if denom == 1 else H * m) and max(sizes) <= D.KERNELS["render" if denom == 1 else "render_scaled"]["unit"], (pic, denom)
            assert all(sizes[i] == sizes[i % (len(sizes) // mcu_ymax)] for i in range(len(sizes))), "every MCU row has the same runs"
    # the pictures the adjacency conditions name: chroma two samples wide at full size (3 and 4 pixels), two and three at 1/2 (8 and 9 pixels of 4:2:2)
    assert [D.render_chroma(p) for p in (("422", 4, 8), ("420", 3, 13), ("422", 5, 8))] == [(2, False), (2, False), (3, True)]
    assert [D.render_chroma(("422", w, 8), 2) for w in (8, 9)] == [(2, False), (3, True)] and D.render_chroma(("422", 16, 8), 4) == (2, False)
    assert D.render_chroma(("422", 200, 8), 8)[1] is False and D.render_chroma(("420", 200, 8), 2)[1] is False and not D.render_filters(8)


def test_the_forms_of_the_gpu_tests_are_all_here():
    assert sorted(D.BUILDERS) == [("coef_hist", "any"), ("coefs", "direct"), ("coefs", "tiled"), ("encode", "420"), ("encode", "422"), ("render", "any"),
                                  ("render_scaled", "2"), ("render_scaled", "4"), ("render_scaled", "8"), ("stats", "hist"), ("stats", "plain"),
                                  ("transform", "plain"), ("transform", "turned")]
    import transform_model as TM
    assert TM.OPS[D.TRANSFORM_FORMS["plain"]["op"]] not in TM.TRANSPOSING and TM.OPS[D.TRANSFORM_FORMS["turned"]["op"]] in TM.TRANSPOSING
    assert D.TRANSFORM_FORMS["turned"]["edge"] == "perfect" and D.TRANSFORM_FORMS["turned"]["crop"]
