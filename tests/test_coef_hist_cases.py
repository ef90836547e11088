"""CPU: the catalogue of tests/coef_hist_cases.py against the oracle.  Every case's claim -- a count in plain Python integers -- must hold for the rows
tests/coef_hist_model.py makes from the oracle's blocks, and each of six wrong models must be refused by the case named for it: slot 0 taken from the
arena, floor instead of truncating division, clamp at R - 1, zeros skipped and the zero bin not rebuilt, extrema seeded with 0, zig-zag applied the
wrong way round."""
import numpy as np
import pytest

import coef_hist_cases as HC
import coef_hist_model as HM
import coef_model as M


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


@pytest.fixture(scope="module")
def views(harness, oracles):
    return {c.name: HC.OracleView(harness, oracles, c.truth_data, c.decode_ac) for c in HC.built()}


def wrong_row(kind, view, c, R, quantised, zigzag):
    """The row a wrong implementation would give."""
    t = view.tensor(c).reshape(-1, 64).astype(np.int64); q = np.maximum(view.q(c), 1)
    if kind == "arena_slot_0":
        t = t.copy(); t[:, 0] = view.blocks[view.geo.arena_index(c)].reshape(-1, 64)[:, 0]
    x = t if not quantised else (t // q if kind == "floor_div" else np.sign(t) * (np.abs(t) // q))
    x = x[:, HC.POSITION if kind == "zigzag_wrong_way_round" else M.ZIGZAG] if zigzag else x
    nb = 2 * R + 1; hist = np.zeros((64, nb), np.uint32)
    lim = R - 1 if kind == "clamp_r_minus_1" else R
    np.add.at(hist, (np.broadcast_to(np.arange(64), x.shape), np.clip(x, -lim, lim) + R), 1)
    if kind == "zero_bin_not_rebuilt":
        hist[:, R] = 0
    mn, mx = x.min(0), x.max(0)
    if kind == "seed_0":
        mn, mx = np.minimum(mn, 0), np.maximum(mx, 0)
    return np.concatenate([hist.reshape(-1), mn.astype(np.int32).view(np.uint32), mx.astype(np.int32).view(np.uint32)])


class Swapped:
    def __init__(self, view, kind):
        self.view, self.kind = view, kind
        self.tensor, self.q = view.tensor, view.q

    def row(self, c, R, quantised=True, zigzag=False):
        return wrong_row(self.kind, self.view, c, R, quantised, zigzag)


WRONG = ["arena_slot_0", "floor_div", "clamp_r_minus_1", "zero_bin_not_rebuilt", "seed_0", "zigzag_wrong_way_round"]


def test_the_model_is_the_definition_on_a_hand_made_tensor():
    t = np.zeros((1, 2, 64), np.int16); t[0, 0, 0] = -7; t[0, 1, 0] = 9; t[0, 0, 8] = -1; t[0, 1, 8] = 300; t[0, 0, 63] = -32768; t[0, :, 5] = [-4, -6]
    q = np.full(64, 2); q[63] = 0
    r = HM.row_of_tensor(t, q, 2)
    assert r.shape == (HM.words(2),) == (448,) and r.dtype == np.uint32
    h, mn, mx = HM.fields(r, 2)
    assert h[0].tolist() == [1, 0, 0, 0, 1] and (mn[0], mx[0]) == (-3, 4), "-7 / 2 = -3, toward zero"
    assert h[8].tolist() == [0, 0, 1, 0, 1] and (mn[8], mx[8]) == (0, 150), "-1 / 2 = 0"
    assert h[63].tolist() == [1, 0, 1, 0, 0] and (mn[63], mx[63]) == (-32768, 0), "a divisor of 0 counts as 1"
    assert h[1].tolist() == [0, 0, 2, 0, 0] and int(h.sum()) == 128 and h[5].tolist() == [2, 0, 0, 0, 0] and (mn[5], mx[5]) == (-3, -2), "no seed shows"
    z = HM.row_of_tensor(t, q, 2, zigzag=True)
    assert HM.fields(z, 2)[0][2].tolist() == h[8].tolist(), "zig-zag position 2 is natural index 8"
    u = HM.row_of_tensor(t, q, 2, quantised=False)
    assert HM.fields(u, 2)[1][0] == -7 and HM.fields(u, 2)[2][8] == 300
    # the wrong models differ from the model, and only as they say
    class V:
        blocks = np.zeros((2, 64), np.int16); geo = M.Geometry([(1, 1)], 2, 1)
        tensor = staticmethod(lambda c: t); q = staticmethod(lambda c: q)
    assert np.array_equal(wrong_row("none", V, 0, 2, True, False), r) and np.array_equal(wrong_row("none", V, 0, 2, True, True), z)
    for kind in WRONG:
        assert any(not np.array_equal(wrong_row(kind, V, 0, 2, True, zz), HM.row_of_tensor(t, q, 2, zigzag=zz)) for zz in (False, True)), kind


def test_the_catalogue_holds_what_the_issue_lists():
    names = [c.name for c in HC.built()]
    for R in HC.RANGES:
        assert "clamp_edges_r%d" % R in names
    assert {"div_edges_dc_q1", "div_edges_dc_q3", "div_edges_dc_q255", "div_edges_ac_table_of_many_divisors", "div_table_with_a_zero_entry",
            "extrema_through_the_int16_wrap", "one_value_everywhere_64x64_blocks", "decode_ac_0_leaves_positions_1_to_63_in_the_zero_bin",
            "dc_constant_difference_1_no_restart", "dc_constant_difference_1_dri3", "dc_constant_difference_1_no_restart_progressive",
            "dc_constant_difference_1_dri3_progressive"} <= set(names)
    assert sorted(k for c in HC.built() for k in c.refuses) == sorted(WRONG), "every wrong model has exactly one case named for it"
    assert all(len(c.data) < 200000 for c in HC.built())


@pytest.mark.parametrize("fn", HC.CASES, ids=lambda f: f.__name__)
def test_every_claim_holds_for_the_model_over_the_oracle(views, fn):
    case = next(c for c in HC.built() if c.name == fn.__name__)
    case.claim(views[case.name])


def test_the_progressive_files_carry_the_coefficients_of_their_baseline_twins():
    import prog_codec as PC
    for c in HC.built():
        if c.truth_data is not c.data:
            a, b = PC.decode(c.data), PC.decode(c.truth_data)
            assert all(np.array_equal(x, y) for x, y in zip(a.coefs, b.coefs)), c.name


@pytest.mark.parametrize("kind", WRONG)
def test_each_wrong_model_is_refused_by_the_case_named_for_it(views, kind):
    case = next(c for c in HC.built() if kind in c.refuses)
    case.claim(views[case.name])
    with pytest.raises(AssertionError):
        case.claim(Swapped(views[case.name], kind))
