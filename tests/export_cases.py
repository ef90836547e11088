"""Content cases of the JPEG export -- TEST INFRASTRUCTURE shared by tests/test_export_model.py (CPU: every case carries a census that its event is
where it was meant to be) and tests/test_gpu_export.py (the kernels, byte for byte against tests/export_model.py).

A case is a grey picture given block by block in decode order: every block a dict {zig-zag position: level} (position 0: the DC level itself, not
the difference), all multipliers 1, so the arena holds the levels.  `file` is prog_codec's baseline encoding (its own optimal tables): what the
library decodes before it exports.  Blocks are laid out ROW blocks to a block row; the grid is padded with empty blocks.

Bit lengths under the Annex K luminance tables: an empty block is DC category 0 (2 bits) + EOB (4 bits) = 6 bits; {1: 1} adds (0, 1) = 2 + 1 bits: 9;
{1: 2} adds (0, 2) = 2 + 2: 10.  With those three any bit position is reachable.  (0, 10) is the 16-bit code FF83: a level 1023 behind it makes
'11' + ten ones = twelve ones in a row from bit 14 of the symbol; a second 1023 behind it twenty-one."""
import export_model as EM
import prog_codec as PC

ROW = 64                                              # blocks per block row of a case's picture
TILE, SCAN, CHUNK, WINDOW = 256, 256, 4096, 8192      # the kernels' seams (include/jsnoop_gpu.h JSNOOP_EXPORT_*; the GPU test checks they are these)

EMPTY = {}
WORST = dict({z: (1023 if z % 2 else -1023) for z in range(1, 64)})        # 63 x (16 + 10) bits of AC
ONLY63 = {63: 1023}                                   # a run of 62: three ZRL, (14, 10), no EOB -- 2 + 33 + 16 + 10 = 61 bits ending in ten ones
ONLY62 = {62: -5}                                     # a run of 61: three ZRL, (13, 3), EOB
FF1 = {1: 1023}                                       # 2 + 16 + 10 + 4 = 32 bits; bits 16..27 of the block are ones
FF2 = {1: 1023, 2: 1023}                              # 2 + 26 + 26 + 4 = 58 bits; bits 16..48 hold '11' + ten ones + nine ones: 21 ones from bit 16


class Case:
    def __init__(self, name, blocks):
        self.name = name
        n = len(blocks); rows = -(-n // ROW); w = min(n, ROW)
        self.frame = PC.Frame(8 * w, 8 * rows, [(1, 1, 0)], {0: [1] * 64})
        assert self.frame.mcu_x == w and self.frame.mcu_y == rows
        self.nblocks = w * rows
        coefs = self.frame.zeros()
        for i, b in enumerate(blocks):
            for z, v in b.items():
                coefs[0][i // w, i % w, z] = v
        self.coefs = coefs
        self._memo = {}

    @property
    def file(self):
        if "file" not in self._memo:
            self._memo["file"] = PC.encode_baseline(self.frame, self.coefs)
        return self._memo["file"]

    def inputs(self):
        return EM.frame_inputs(self.frame, self.coefs)

    def model(self):
        """(tokens, un-stuffed bytes, bits, block ends, file) of the export of this case."""
        if "model" not in self._memo:
            arena, dccum, geo, qnat = self.inputs()
            lev, result, _ = EM.levels(arena, dccum, geo, qnat)
            assert result == EM.OK
            T = EM.tokens(lev, geo)
            u, bits = EM.unstuffed(T, EM.ANNEX_K)
            res, _d, f = EM.export_file(arena, dccum, geo, self.frame.width, self.frame.height, qnat)
            assert res == EM.OK
            self._memo["model"] = (T, u, bits, EM.block_ends(T, EM.ANNEX_K), f)
        return self._memo["model"]


def fill(bits):
    """Blocks of 6, 9 and 10 bits that make exactly `bits` bits (bits >= 12, or one of 0 6 9 10)."""
    for nine in (0, 1):
        for ten in (0, 1, 2):
            rest = bits - 9 * nine - 10 * ten
            if rest >= 0 and rest % 6 == 0:
                return [EMPTY] * (rest // 6) + [{1: 1}] * nine + [{1: 2}] * ten
    raise AssertionError(bits)


def dc_swing(n):
    """n worst-case blocks: every AC level +-1023, the DC level alternating 1023 / -1024 so that every difference but the first is +-2047."""
    return [{**WORST, 0: (1023 if i % 2 == 0 else -1024)} for i in range(n)]


def cases():
    out = []
    # five or more blocks share a 32-bit word; the total length runs through every residue mod 8 (no padding at 0)
    for n in range(20, 24):
        out.append(Case("empty_%d" % n, [EMPTY] * n))                                      # 6 n bits: residues 0 6 4 2
        out.append(Case("empty_%d_odd" % n, [EMPTY] * n + [{1: 1}]))                         # + 9: residues 1 7 5 3
    out.append(Case("worst_alone", dc_swing(1)))
    out.append(Case("worst_two", dc_swing(2)))
    out.append(Case("worst_overflows_window", dc_swing(64)))                               # 64 x 1658 bits = 13 264 bytes in one tile: past the 8 KiB window
    out.append(Case("worst_tile_and_one", dc_swing(TILE + 1)))
    out.append(Case("worst_past_a_scan_step_of_chunks", dc_swing(5248)))                     # 5248 x 1658 bits: 265 stuffing chunks, more than one scan step
    out.append(Case("runs_of_62", [ONLY63, ONLY62, EMPTY, ONLY63, ONLY63, ONLY62]))
    out.append(Case("no_eob_last", [EMPTY] * 3 + [ONLY63]))
    # a block that ends exactly on a byte, on a word, and on the end of a tile's range that is itself a word boundary
    out.append(Case("ends_on_byte", fill(16) + [EMPTY] * 3))                               # 6 + 10 = 16 bits behind block 1
    out.append(Case("ends_on_word", fill(32) + [EMPTY] * 3))
    out.append(Case("tile_ends_on_word", [EMPTY] * TILE + [FF1] + [EMPTY] * 3))                # 256 x 6 = 1536 = 48 words: the two tiles share no word
    # FF bytes of the un-stuffed stream at chosen places (byte k = bits 8 k .. 8 k + 7): a block FF1 / FF2 that starts at bit 8 k - 16
    for name, k, blk in (("ff_first_of_chunk", CHUNK, FF1), ("ff_last_of_chunk", CHUNK - 1, FF1), ("ff_across_chunk_edge", CHUNK - 1, FF2),
                         ("ff_first_of_second_chunk_edge", 2 * CHUNK, FF1)):
        out.append(Case(name, fill(8 * k - 16) + [blk] + [EMPTY] * 7))
    out.append(Case("ff_padded_last", fill(9) + [ONLY63]))                                  # 9 + 61 = 70 bits ending in ten ones: the last byte is six ones + two of padding
    return out


def check_census(case):
    """Asserts that the event the case is named after is where it was meant to be (in the model's un-stuffed stream)."""
    T, u, bits, ends, f = case.model()
    nm = case.name
    if nm.startswith("empty_"):
        n = int(nm.split("_")[1]); odd = nm.endswith("_odd")
        assert ends[:n] == [6 * (i + 1) for i in range(n)]
        assert case.nblocks == n + odd and bits == 6 * case.nblocks + (3 if odd else 0) and sum(1 for e in ends if e <= 32) >= 5
        return bits % 8
    if nm == "worst_alone":
        assert bits == 8 + 10 + 63 * 26 and len(u) == 207, (bits, len(u))            # the first difference is 1023: category 10, an 8-bit code
    if nm == "worst_two":
        assert ends[1] - ends[0] == 9 + 11 + 63 * 26 == 1658                          # the 2047 difference: the longest block there is
    if nm == "worst_overflows_window":
        assert ends[63] > 8 * WINDOW and case.nblocks <= TILE
    if nm == "worst_tile_and_one":
        assert case.nblocks > TILE
    if nm == "worst_past_a_scan_step_of_chunks":
        assert len(u) > (SCAN + 1) * CHUNK and case.nblocks == 5248
    if nm == "runs_of_62":
        zrl = [i for i, t in enumerate(T) if t[0] == 0 and t[2] == 0xF0]
        assert len(zrl) == 3 * 5
        assert ends[0] == 61 and ends[1] - ends[0] == 2 + 33 + PC._codes(EM.AC_LUM)[0xD3][1] + 3 + 4
    if nm == "no_eob_last":
        assert T[-2][2] == 0xEA and T[-1] == (1, 1023, 10)                             # the file's last symbol is the coefficient, not EOB
    if nm == "ends_on_byte":
        assert 16 in ends
    if nm == "ends_on_word":
        assert 32 in ends
    if nm == "tile_ends_on_word":
        assert ends[TILE - 1] % 32 == 0 and case.nblocks > TILE, ends[TILE - 1]
    if nm.startswith("ff_") and nm != "ff_padded_last":
        at = [i for i, b in enumerate(u) if b == 0xFF]
        want = {"ff_first_of_chunk": [CHUNK], "ff_last_of_chunk": [CHUNK - 1], "ff_across_chunk_edge": [CHUNK - 1, CHUNK], "ff_first_of_second_chunk_edge": [2 * CHUNK]}[nm]
        assert at == want, (at, want)
        assert len(u) > want[-1] + 1
    if nm == "ff_padded_last":
        assert bits % 8 != 0 and u[-1] == 0xFF and u[-2] != 0xFF and f.endswith(b"\xFF\x00\xFF\xD9")
    return bits % 8
