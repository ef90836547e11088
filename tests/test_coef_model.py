"""CPU: tests/coef_model.py, the numpy model the coefficient pack is compared with on the GPU, and its two inputs pinned to the oracle (itself
pinned to the compiled reference): the blocks are oracle_coefs() of a Full-IDCT decode; the cumulative DC of component c at block (bx, by)
is sample (by * 8 * ev, bx * 8 * eh) of the oracle's int16 plane of a decode_ac = 0 decode of the same file.  A plain int16-wrapping
running sum of slot 0 per component, restarted at every restart interval, must give the same grid, and the DC-only decode must leave
zeros in every AC slot.  (The reference's own block-DC maps are NOT used: for subsampled layouts its luma map is indexed with the wrong
MCU stride and overwrites itself.)"""
import numpy as np
import pytest

import coef_model as M

SIZES = [(1, 1), (8, 8), (9, 9), (16, 17), (17, 24), (72, 40), (520, 9), (1032, 17), (333, 217)]
LAYOUTS = {"444": dict(hs=1, vs=1), "422": dict(hs=2, vs=1), "420": dict(hs=2, vs=2), "440": dict(hs=1, vs=2), "grey": dict(gray=1)}
RESTARTS = [0, 1, 3]


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


def test_hand_made_420_arena_goes_where_the_grid_says():
    geo = M.Geometry([(2, 2), (1, 1), (1, 1)], 2, 1)
    assert (geo.bpm, geo.nblocks, geo.grid(0), geo.grid(1)) == (6, 12, (4, 2), (2, 1))
    assert geo.arena_index(0).tolist() == [[0, 1, 6, 7], [2, 3, 8, 9]] and geo.arena_index(1).tolist() == [[4, 10]] and geo.arena_index(2).tolist() == [[5, 11]]
    blocks = (np.arange(12)[:, None] * 100 + np.arange(64)[None, :]).astype(np.int16); cum = (-np.arange(12) - 1).astype(np.int16)
    t = M.coef_tensor(blocks, cum, geo, 0)
    assert t.shape == (2, 4, 64) and t[1, 2, 0] == -9 and t[1, 2, 63] == 863 and t[0, 1, 8] == 108
    z = M.coef_tensor(blocks, cum, geo, 0, zigzag=True)
    assert z[1, 2, 0] == -9 and z[1, 2, 2] == 808 and z[1, 2, 3] == 816 and z[1, 2, 63] == 863
    f = M.coef_tensor(blocks, cum, geo, 2, layout="freq", dtype=np.float32, zigzag=True)
    assert f.shape == (64, 1, 2) and f.dtype == np.float32 and f[0].tolist() == [[-6.0, -12.0]] and f[2].tolist() == [[508.0, 1108.0]]
    assert sorted(M.ZIGZAG) == list(range(64)) and M.ZIGZAG[:6] == [0, 1, 8, 16, 9, 2]
    assert M.running_dc(np.ones((12, 64), np.int16), geo, 1).tolist() == [1, 2, 3, 4, 1, 1] * 2
    assert M.running_dc(np.full((12, 64), 30000, np.int16), geo)[[0, 1, 2, 3]].tolist() == [30000, -5536, 24464, -11072]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_cumulative_dc_of_the_dc_only_planes_is_the_running_sum_of_the_arena(harness, oracles, layout):
    full, dc = oracles; grids = 0
    for k, (w, h) in enumerate(SIZES):
        for dri in RESTARTS:
            data = harness.synth_jpeg(width=w, height=h, quality=88, restart_interval=dri, seed=300 + 7 * k + dri, **LAYOUTS[layout])
            p = harness.drive(full, data); blocks = harness.oracle_coefs(full)
            harness.drive(dc, data); dcb = harness.oracle_coefs(dc)
            geo = M.geometry_of(p)
            assert blocks.shape == (geo.nblocks, 64) == dcb.shape, (layout, w, h, blocks.shape, geo.nblocks)
            assert not dcb[:, 1:].any(), "the DC-only decode leaves zeros in the AC slots"
            assert np.array_equal(dcb[:, 0], blocks[:, 0])
            cum = M.cum_from_planes(dc.planes(), geo); run = M.running_dc(blocks, geo, dri)
            for c in range(geo.ncomp):
                idx = geo.arena_index(c)
                assert np.array_equal(cum[idx], run[idx]), "%s %dx%d dri %d component %d: %d blocks differ" % (layout, w, h, dri, c, int((cum[idx] != run[idx]).sum()))
                grids += 1
    assert grids == len(SIZES) * len(RESTARTS) * (1 if layout == "grey" else 3)
