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
    for kernel, form, most in (("encode", "any", 100), ("transform", "any", 3600), ("coefs", "direct", 4500), ("coefs", "tiled", 4500), ("stats", "hist", 400), ("coef_hist", "any", 100)):
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
        refused = [k for k, r in enumerate(recs) if r.sizes is None]
        if kernel == "transform":
            assert refused and all(0 < k < len(recs) - 1 and (recs[k - 1].sizes and recs[k + 1].sizes) for k in refused), "refused entries sit among those that are OK"
            assert len({recs[k].pic for k in refused}) == (2 if form == "turned" else 1)
        else:
            assert not refused


def test_the_forms_of_the_gpu_tests_are_all_here():
    assert sorted(D.BUILDERS) == [("coef_hist", "any"), ("coefs", "direct"), ("coefs", "tiled"), ("encode", "420"), ("encode", "422"), ("stats", "hist"), ("stats", "plain"),
                                  ("transform", "plain"), ("transform", "turned")]
    import transform_model as TM
    assert TM.OPS[D.TRANSFORM_FORMS["plain"]["op"]] not in TM.TRANSPOSING and TM.OPS[D.TRANSFORM_FORMS["turned"]["op"]] in TM.TRANSPOSING
    assert D.TRANSFORM_FORMS["turned"]["edge"] == "perfect" and D.TRANSFORM_FORMS["turned"]["crop"]
