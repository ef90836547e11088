#!/usr/bin/env python3
"""CPU model of the steps the write pass takes (k_write2 / k_write_dc) on the bench pictures: no GPU.

    python tools/walk_steps_model.py [--seeds 1 33] [--width 1920 --height 1080] [--wl 7] [--bound 32]

A sequential Huffman walk over the un-stuffed scan of `oracle` synth pictures (4:2:0, q85: bench.py's) lists every symbol.  A lane per
sub-sequence of 32 << wl bits then walks as the kernels do -- from the first symbol boundary inside its range to the end of the block
that is open at the range's end -- and a step takes the AC symbol behind the first one, in the same block, when the rule lets it:

  pair rows  (the tables alone): first symbol AC and not EOB, its code within the 9-bit first level, and the second symbol's code
             inside the same 9-bit window: len1 + size1 + len2 <= 9
  own read   (what the kernels do): the pair rows, else a table read of its own at the bits behind the first symbol: first symbol
             DC or AC (not EOB), both codes within the first level, all four fields within --bound bits (JS_STEP_BITS)

Both only when the second symbol starts inside the lane's range and keeps the coefficient index inside the block.  Printed per seed
and rule: symbols, symbols per step, mean steps per lane, mean over the waves (64 lanes) of the slowest lane -- what a wave costs.
Uses oracle.harness only (profiles/r09_second_symbol.txt holds its output next to the measured kernel)."""
import argparse
import bisect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L1_BITS = 9


def lut16(table):
    """(counts, values) -> 65536 entries (length << 8 | symbol), 0 where no code matches."""
    counts, vals = table
    lut = [0] * 65536
    code = 0; k = 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            lo = code << (16 - ln)
            e = (ln << 8) | vals[k]
            for w in range(lo, lo + (1 << (16 - ln))):
                lut[w] = e
            code += 1; k += 1
        code <<= 1
    return lut


def symbols_of(data, H):
    """Every symbol of the first scan: (bit position, block, coefficient index before it, code length, size, index advance or 0 for EOB)."""
    p = H.parse_jpeg(data)
    assert p.sof == 0xC0 and not p.rst_en, "baseline without restart markers"
    raw = data[p.scan_start:p.scan_end].replace(b"\xFF\x00", b"\xFF") + b"\0" * 8
    hv = [(h, v) for _i, h, v, _t in p.comps] if len(p.comps) > 1 else [(1, 1)]
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    mcus = -(-p.x // (8 * hmax)) * -(-p.y // (8 * vmax))
    luts = {}
    order = []
    for c, (h, v) in enumerate(hv):
        _sel, td, ta = p.scan_comps[c]
        for key in ((0, td), (1, ta)):
            if key not in luts:
                luts[key] = lut16(p.dht[key])
        order += [(luts[(0, td)], luts[(1, ta)])] * (h * v)
    out = []; pos = 0; blk = 0
    frm = int.from_bytes
    for _m in range(mcus):
        for dc, ac in order:
            k = 0
            while k < 64:
                w = (frm(raw[pos >> 3:(pos >> 3) + 4], "big") >> (16 - (pos & 7))) & 0xFFFF
                e = (dc if k == 0 else ac)[w]
                ln = e >> 8; sym = e & 255
                assert ln, "no code at bit %d" % pos
                size = sym & 15
                if k == 0:
                    out.append((pos, blk, 0, ln, sym, 1)); pos += ln + sym; k = 1
                    continue
                eob = sym == 0
                adv = 0 if eob else (sym >> 4) + 1
                out.append((pos, blk, k, ln, size, adv)); pos += ln + size
                k = 64 if eob else k + adv
            blk += 1
    return out, pos


def steps_of(syms, total_bits, wl, rule, bound):
    """Steps of every lane under `rule` ("rows" / "read")."""
    sub = 32 << wl
    starts = [s[0] for s in syms]
    n = len(syms)
    lanes = []; visited = 0
    for i in range(-(-total_bits // sub)):
        own_end = min((i + 1) * sub, total_bits)
        j = bisect.bisect_left(starts, i * sub)
        steps = 0
        while j < n:
            pos, blk, k, ln, size, adv = syms[j]
            if pos >= own_end and (k == 0):
                break                                             # the block open at the end of the range is finished; nothing new starts
            take = 1
            if j + 1 < n and not (k and adv == 0) and ln <= L1_BITS:
                p2, blk2, k2, ln2, size2, adv2 = syms[j + 1]
                if blk2 == blk and p2 < own_end and k2 + max(adv2, 1) <= 64:
                    rows = k != 0 and ln + size + ln2 <= L1_BITS
                    if rows or (rule == "read" and ln2 <= L1_BITS and ln + size + ln2 + size2 <= bound):
                        take = 2
            j += take; steps += 1; visited += take
        lanes.append(steps)
    return lanes, visited


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 33])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--wl", type=int, default=7, help="sub-sequences of 32 << wl bits (7: 4096, the bench's)")
    ap.add_argument("--bound", type=int, default=32, help="bits one step may consume (JS_STEP_BITS)")
    a = ap.parse_args()
    from oracle import harness as H
    H.build(["oracle", "synth"])
    print("%-6s %-10s %10s %14s %16s %22s" % ("seed", "rule", "symbols", "symbols/step", "steps per lane", "slowest lane of a wave"))
    for seed in a.seeds:
        data = H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=a.quality, seed=seed)
        syms, bits = symbols_of(data, H)
        base = None
        for rule in ("rows", "read"):
            lanes, visited = steps_of(syms, bits, a.wl, rule, a.bound)
            waves = [max(lanes[w:w + 64]) for w in range(0, len(lanes), 64)]
            walked = sum(lanes)
            slow = sum(waves) / len(waves)
            print("%-6d %-10s %10d %14.3f %16.1f %22.1f%s" % (seed, rule, len(syms), visited / walked, walked / len(lanes), slow,
                                                              "" if base is None else "   (%+.1f %% wave steps)" % (100.0 * (slow / base - 1.0))))
            base = base or slow


if __name__ == "__main__":
    main()
