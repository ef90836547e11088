"""-m gpu: the back end's term rounds at every list length where their code takes another path.

idct_pair runs the terms of two blocks in lock step, max(nA, nB) steps, in rounds of sixteen that never read past the end of the lists: a tail per way
out of a round, a prologue per short list, one text for all four rounds (jsnoop_pair_round.h, PAIR_EXACT_ASM).  The paths are chosen by the AC counts of
the two blocks alone, so the pictures here are made of block pairs with chosen counts: every ordered pair (nA, nB) of the edge set E -- nothing, the
short lists, the first and last tail, both sides of every round's end, the longest list -- laid into the block pairs of consecutive MCUs (4:2:0:
(Y0, Y1), (Y2, Y3), (Cb, Cr)), the non-zero coefficients at seeded random positions with values in +-1..3, random DC, unit quantisers
(tests/prog_codec.py writes the files).  In the shuffled order a long list is followed by a short one in the same wave, with stale entries behind the new
end.  The other layouts run kernels <2..4> (4:4:4: the last pair has an idle half); next to a grayscale picture the batch takes the any-layout kernel
<0> and its four fast instances.

Everything is compared with the oracle: the whole DIB and the whole coefficient arena bit for bit, flags 0."""
import numpy as np
import pytest

import prog_codec as P

E = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 18, 20, 31, 32, 33, 36, 47, 48, 49, 52, 62, 63]
PAIRS = [(a, b) for a in E for b in E]
# luma sampling -> (MCUs across, MCUs down): room for all 529 pairs at (blocks per MCU + 1) / 2 pairs per MCU
LAYOUTS = {"420": ((2, 2), (16, 12)), "422": ((2, 1), (16, 17)), "440": ((1, 2), (16, 17)), "444": ((1, 1), (17, 16))}


class Picture:
    def __init__(self, name, frame, coefs, counts):
        self.name, self.frame, self.counts = name, frame, counts          # counts: AC coefficients per block, arena order
        self.file = P.encode_baseline(frame, coefs)
        self.dib = self.coefs = self.cks = None

    def answer(self, harness, oracle):
        if self.dib is None:
            import jpegsnoop_amd as J
            harness.drive(oracle, self.file)
            self.dib, self.coefs = oracle.dib(), harness.oracle_coefs(oracle)
            self.cks = J.dib_checksum_numpy(self.dib)
        return self


def block(rng, n):
    b = np.zeros(64, np.int16)
    b[0] = rng.integers(-100, 101)
    k = 1 + rng.choice(63, size=n, replace=False)                         # zig-zag positions of the AC coefficients
    b[k] = rng.choice([-3, -2, -1, 1, 2, 3], size=n)
    return b


def pair_picture(layout, shuffled):
    (H, V), (mx, my) = LAYOUTS[layout]
    fr = P.Frame(mx * 8 * H, my * 8 * V, [(H, V, 0), (1, 1, 1), (1, 1, 1)], {0: [1] * 64, 1: [1] * 64})
    rng = np.random.default_rng(7000 + sum(map(ord, layout)) + int(shuffled))
    pairs = list(PAIRS)
    if shuffled:
        rng.shuffle(pairs)
    blocks = fr.mcu_blocks(); nb = len(blocks); per_mcu = (nb + 1) // 2
    assert fr.mcu_x * fr.mcu_y * per_mcu >= len(pairs)
    coefs = fr.zeros(); counts = []
    for m in range(fr.mcu_x * fr.mcu_y):
        y0, x0 = divmod(m, fr.mcu_x)
        for j, (c, v, h) in enumerate(blocks):
            i = m * per_mcu + j // 2                                      # the pair this block is a half of
            n = pairs[i][j % 2] if i < len(pairs) else 0
            hh, vv = fr.hv[c]
            coefs[c][y0 * vv + v, x0 * hh + h] = block(rng, n)
            counts.append(n)
    return Picture("%s%s" % (layout, "_shuffled" if shuffled else ""), fr, coefs, np.array(counts))


def gray_picture():
    fr = P.Frame(64, 48, [(1, 1, 0)], {0: [1] * 64})
    rng = np.random.default_rng(7100)
    coefs = fr.zeros(); counts = []
    for m in range(fr.mcu_x * fr.mcu_y):
        n = E[m % len(E)]
        coefs[0][m // fr.mcu_x, m % fr.mcu_x] = block(rng, n); counts.append(n)
    return Picture("gray", fr, coefs, np.array(counts))


_PICTURES = {}


def picture(name):
    if name not in _PICTURES:
        _PICTURES[name] = gray_picture() if name == "gray" else pair_picture(name.split("_")[0], name.endswith("_shuffled"))
    return _PICTURES[name]


ALL = ["420", "420_shuffled", "422", "440", "444", "gray"]


def test_the_pictures_hold_every_pair_of_edge_counts(harness, oracle):
    """CPU: what the oracle decodes from the files has the AC counts the pictures were laid out with, and every pair of E x E sits in a block pair."""
    for name in ALL:
        p = picture(name).answer(harness, oracle)
        got = (p.coefs[:, 1:] != 0).sum(1)
        assert np.array_equal(got, p.counts), name
        assert len(p.file) < 40000
        if name != "gray":
            nb = len(p.frame.mcu_blocks()); per = (nb + 1) // 2
            c = p.counts.reshape(-1, nb)
            c = np.concatenate([c, np.full((len(c), 2 * per - nb), -1)], 1).reshape(-1, 2)      # (nA, nB) per pair, -1: the idle half
            have = {(int(a), int(b)) for a, b in c}
            if nb % 2 == 0:
                assert set(PAIRS) <= have and c.max() == 63, name
            else:                                                         # every second pair of the list sits in the pair with the idle half: nA alone
                assert set(PAIRS[0::2]) | {(a, -1) for a, _ in PAIRS[1::2]} <= have and c.max() == 63, name
    assert len(PAIRS) == 529 and picture("420").frame.mcu_x * picture("420").frame.mcu_y == 192


def check(b, pics, harness, oracle, what):
    """Image i of batch b is pics[i % len(pics)]."""
    sums = b.dib_checksums()
    for i in range(len(b)):
        p = pics[i % len(pics)].answer(harness, oracle); inf = b.info(i)
        assert inf["path"] == 1 and inf["flags"] == 0, (what, p.name, i, inf)
        assert int(sums[i]) == p.cks, (what, p.name, i, "DIB checksum")
        got = b.dib(i)
        assert got.shape == p.dib.shape and np.array_equal(got, p.dib), (what, p.name, i, "DIB differs in %d bytes" % int((got != p.dib).sum()))
        assert np.array_equal(b.coefs(i), p.coefs), (what, p.name, i, "coefficient arena")


def run_batch(names, copies, harness, oracle, what):
    import jpegsnoop_amd as J
    pics = [picture(n) for n in names]
    b = J.JpegBatch()
    try:
        for p in pics:
            b.add_jpeg(p.file)
        if copies > 1:
            b.tile(copies * len(pics))
        b.upload(); b.decode(); b.sync()
        check(b, pics, harness, oracle, what)
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["420", "420_shuffled", "422", "440", "444"])
def test_every_pair_of_edge_counts_in_the_one_layout_kernels(harness, oracle, name):
    """A batch of one layout: k_idct_color<1..4>.  Alone and as eight copies."""
    run_batch([name], 1, harness, oracle, name)
    run_batch([name], 8, harness, oracle, name + " x 8")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["420", "420_shuffled", "422", "440", "444"])
def test_every_pair_of_edge_counts_in_the_any_layout_kernel(harness, oracle, name):
    """Next to a grayscale picture the launch is k_idct_color<0>: the colour picture runs one of its four fast instances, the gray one its general path."""
    run_batch([name, "gray"], 1, harness, oracle, name + " + gray")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["420", "420_shuffled", "422", "440", "444"])
def test_every_pair_of_edge_counts_through_the_single_image_call(harness, oracle, gpu, name):
    p = picture(name).answer(harness, oracle)
    harness.drive(gpu, p.file)
    assert gpu.lib.jsnoop_last_path(gpu.h) == 1 and gpu.lib.jsnoop_last_flags(gpu.h) == 0, name
    got = gpu.dib()
    assert got.shape == p.dib.shape and np.array_equal(got, p.dib), (name, "DIB differs in %d bytes" % int((got != p.dib).sum()))
