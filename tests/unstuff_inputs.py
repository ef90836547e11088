"""Inputs that put chosen bytes on the seams of the un-stuffing stage, each with a census that says so, shared by
tests/test_unstuff_seams_golden.py, tests/test_gpu_unstuff_seams.py and tests/golden/make_unstuff_seams.py.

The stage works on a grid anchored at `scan start & ~15` of the file: a thread owns 16 bytes of it, a wave 1 KiB, a workgroup a 4 KiB chunk,
the fused kernel a super-chunk of four chunks (16 KiB).  A scan byte at scan index i sits at grid position (scan_start & 15) + i, so a COM
segment of 16 + k bytes in front of SOF (pad_header) moves every byte of the scan over the grid without changing a pixel or a coefficient.
`census` counts, straight from the byte rules, how often an FF/00 pair or a restart marker meets a grid line; the `check_*` functions are the
conditions the tests assert ON THE CPU before they trust a GPU result -- a change of the generator that loses the coverage fails there."""
import numpy as np

PERIODS = (16, 1024, 4096, 16384)           # thread, wave, chunk (workgroup), super-chunk of four chunks
PATTERNS = ("FF|00", "FF|Dn", "FF Dn|", "|FF Dn")
PADS = tuple(range(16))

SEAM_KW = dict(seed=5, width=1920, height=1080, hs=2, vs=2, quality=95, restart_interval=2)
PLAIN_KW = dict(seed=5, width=1920, height=1080, hs=2, vs=2, quality=95)                      # the same picture without restart markers
END_KW = dict(width=320, height=240, seed=121, quality=90)                                   # scan_start 623, scan_len 32767
END_PADS = (1, 2, 3)                                                                         # (phase + scan_len) % 4096 = 4095, 0, 1
TINY_KWS = {"gray8": dict(width=8, height=8, gray=1), "c420_16": dict(width=16, height=16, hs=2, vs=2)}     # scans of 25 and 116 bytes
COUNT_KWS = [dict(width=w, height=h, seed=61, quality=92) for w, h in ((96, 64), (128, 96), (160, 112), (176, 144), (224, 160))]   # 1, 2, 3, 4, 5 chunks of 4 KiB
EDGE_SIZES = ((72, 48), (152, 24), (232, 16))                                                # 54, 57, 58 MCUs of 8 x 8
EDGE_DRI = 3
DAMAGE_PAD = 6
DAMAGES = {"ff_ff": (1, b"\xff\xff"), "ff_ff_00": (2, b"\xff\xff\x00"), "ff_ffd3": (1, b"\xff\xff\xd3"), "ffd3_ffd4": (2, b"\xff\xd3\xff\xd4"),
           "ff_d9": (1, b"\xff\xd9"), "ff_e0": (1, b"\xff\xe0")}                            # name -> (bytes in front of the seam, bytes written)
DAMAGE_SEAMS = {"4k": 4096 * 149, "16k": 16384 * 41}                                         # grid positions: a chunk seam that is no super-chunk seam, and one that is


def scan_range(data):
    """(scan_start, scan_end) by the byte rules: the scan ends at the first FF followed by neither 00 nor RSTn (or at the end of the file)."""
    a = np.frombuffer(data, np.uint8)
    pos = 2
    while a[pos + 1] != 0xDA:
        assert a[pos] == 0xFF, pos
        pos += 2 + (int(a[pos + 2]) << 8 | int(a[pos + 3]))
    s = pos + 2 + (int(a[pos + 2]) << 8 | int(a[pos + 3]))
    ff = np.flatnonzero(a[s:-1] == 0xFF) + s
    nx = a[ff + 1]
    end = ff[(nx != 0) & ((nx & 0xF8) != 0xD0)]
    return s, int(end[0]) if end.size else len(data)


def pad_header(data, k):
    """The same JPEG with a COM segment of 16 + k bytes (marker and length included) in front of SOF: scan_start moves by 16 + k."""
    assert 0 <= k < 16
    pos = 2
    while data[pos + 1] not in (0xC0, 0xC1, 0xC2):
        assert data[pos] == 0xFF and data[pos + 1] != 0xDA, pos
        pos += 2 + (data[pos + 2] << 8 | data[pos + 3])
    n = 16 + k
    com = b"\xff\xfe" + (n - 2).to_bytes(2, "big") + bytes((0x20 + i) & 0x7F for i in range(n - 4))
    return data[:pos] + com + data[pos:]


def census(data):
    """Where the scan's FF pairs meet the grid lines.  For each period P: counts of FF|00 and FF|Dn (the pair split by a line), FF Dn| (a marker
    ends on a line) and |FF Dn (one begins on it); then the start phase, (phase + scan_len) % 4096, the number of 4 KiB chunks and its residue mod 4."""
    s, e = scan_range(data)
    a = np.frombuffer(data, np.uint8)[s:e]
    phase = s & 15
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, np.int64)
    nx = a[ff + 1]
    g = ff + phase                                                  # grid position of the FF
    is00, isdn = nx == 0, (nx & 0xF8) == 0xD0
    out = {"scan_start": s, "scan_len": e - s, "phase": phase, "end_mod_4096": (phase + e - s) % 4096,
           "chunks": max(1, (phase + e - s + 4095) // 4096), "markers": int(isdn.sum())}
    out["chunks_mod_4"] = out["chunks"] % 4
    for P in PERIODS:
        split, after, before = (g + 1) % P == 0, (g + 2) % P == 0, (g % P == 0) & (g > 0)
        inside = g + 2 < phase + len(a)                             # a line with scan bytes behind it
        out[str(P)] = [int((split & is00).sum()), int((split & isdn).sum()), int((after & isdn & inside).sum()), int((before & isdn).sum())]
    return out


# ------------------------------------------------------------------------------------------------------------------- the sets
def seam_set(H):
    base = H.synth_jpeg(**SEAM_KW)
    return {"seam_p%02d" % k: pad_header(base, k) for k in PADS}


def plain_set(H):
    base = H.synth_jpeg(**PLAIN_KW)
    return {"plain_p%02d" % k: pad_header(base, k) for k in PADS}


def end_set(H):
    base = H.synth_jpeg(**END_KW)
    return {"end_p%02d" % k: pad_header(base, k) for k in END_PADS}


def end_all_pads(H):
    base = H.synth_jpeg(**END_KW)
    return {"end_p%02d" % k: pad_header(base, k) for k in PADS}


def tiny_set(H):
    return {"tiny_%s_p%02d" % (name, k): pad_header(H.synth_jpeg(**kw), k) for name, kw in TINY_KWS.items() for k in PADS}


def count_set(H):
    return {"count_%d" % (i + 1): H.synth_jpeg(**kw) for i, kw in enumerate(COUNT_KWS)}


def _dri_pos(data):
    pos = 2
    while data[pos + 1] != 0xDD:
        assert data[pos] == 0xFF and data[pos + 1] != 0xDA, pos
        pos += 2 + (data[pos + 2] << 8 | data[pos + 3])
    return pos + 4


def get_dri(data):
    pos = _dri_pos(data)
    return data[pos] << 8 | data[pos + 1]


def set_dri(data, dri):
    """Rewrites the two bytes of the DRI segment, so that every reader of the FILE sees the same interval."""
    pos = _dri_pos(data)
    return data[:pos] + dri.to_bytes(2, "big") + data[pos + 2:]


def edge_set(H):
    """Grayscale files encoded with a marker behind every MCU, announced as DRI 3: nmcu - 1 markers against a table sized for nmcu / 3."""
    return {"edge_%d" % ((w // 8) * (h // 8)): set_dri(H.synth_jpeg(width=w, height=h, gray=1, restart_interval=1, seed=70 + i, quality=85), EDGE_DRI)
            for i, (w, h) in enumerate(EDGE_SIZES)}


def edge_neighbour(H):
    return H.synth_jpeg(width=96, height=48, gray=1, restart_interval=1, seed=74, quality=85)


def damaged_set(H):
    base = pad_header(H.synth_jpeg(**SEAM_KW), DAMAGE_PAD)
    s, _ = scan_range(base)
    out = {}
    for sn, g in DAMAGE_SEAMS.items():
        at = s - (s & 15) + g                                       # file offset of the first byte behind the line
        for name, (front, b) in DAMAGES.items():
            out["bad_%s_%s" % (name, sn)] = base[:at - front] + b + base[at - front + len(b):]
    return out


def all_inputs(H):
    """name -> bytes of everything tests/golden/unstuff_seams.json records."""
    out = {}
    for part in (seam_set(H), plain_set(H), end_all_pads(H), tiny_set(H), count_set(H), edge_set(H), {"edge_neighbour": edge_neighbour(H)}, damaged_set(H)):
        out.update(part)
    out["end_base"] = H.synth_jpeg(**END_KW)
    return out


# ------------------------------------------------------------------------------------------------------------- the conditions
def check_seam_set(files):
    cs = [census(d) for d in files.values()]
    assert sorted(c["phase"] for c in cs) == list(range(16)), "all 16 start phases"
    for P in ("4096", "16384"):
        for j, pat in enumerate(PATTERNS):
            assert any(c[P][j] for c in cs), "no %s on a %s-byte seam under any pad" % (pat, P)
    return cs


def check_plain_set(files):
    cs = [census(d) for d in files.values()]
    assert sorted(c["phase"] for c in cs) == list(range(16))
    assert all(c["markers"] == 0 for c in cs)
    for P in ("4096", "16384"):
        assert any(c[P][0] for c in cs), "no FF|00 on a %s-byte seam under any pad" % P
    return cs


def check_end_set(files):
    cs = {k: census(d) for k, d in files.items()}
    assert [cs["end_p%02d" % k]["end_mod_4096"] for k in END_PADS] == [4095, 0, 1]
    assert cs["end_p02"]["chunks"] == 8 and cs["end_p01"]["chunks"] == 8 and cs["end_p03"]["chunks"] == 9      # on the line: a super-chunk line as well
    return cs


def check_tiny_set(files):
    cs = {k: census(d) for k, d in files.items()}
    for name, n in (("gray8", 25), ("c420_16", 116)):
        mine = [c for k, c in cs.items() if k.startswith("tiny_" + name)]
        assert sorted(c["phase"] for c in mine) == list(range(16)) and all(c["scan_len"] == n and c["chunks"] == 1 for c in mine), name
        threads = sorted(set((c["phase"] + n + 15) // 16 for c in mine))
        assert threads == ([2, 3] if n == 25 else [8, 9]), (name, threads)          # two or three threads' bytes; a few threads of one wave
    return cs


def check_count_set(files):
    cs = [census(d) for d in files.values()]
    assert [c["chunks"] for c in cs] == [1, 2, 3, 4, 5]
    assert sorted(set(c["chunks_mod_4"] for c in cs)) == [0, 1, 2, 3]
    return cs


def edge_seg_cap(nmcu, dri):
    """Entries of an image's interval table, restated from JsnoopBatch::upload (jpegsnoop_amd/csrc/jsnoop_host.cpp: want_seg = nmcu / DRI + 2,
    seg_cap = 2 * want_seg + 16); a stream with m markers needs m + 2 entries (interval 0, one per marker, the end sentinel)."""
    return 2 * (nmcu // dri + 2) + 16


def check_edge_set(files):
    sides = []
    for (w, h), d in zip(EDGE_SIZES, files.values()):
        nmcu = (w // 8) * (h // 8)
        c = census(d)
        assert c["markers"] == nmcu - 1, (w, h, c["markers"])
        need, cap = c["markers"] + 2, edge_seg_cap(nmcu, get_dri(d))                 # the interval the FILE announces
        sides.append((need > cap) - (need < cap))
    assert sides == [-1, 0, 1], sides                                # one entry to spare, fits exactly, one too many
    return sides


def check_damaged_set(H, files):
    """Every file is the padded seam file with exactly the named bytes written across the named grid line, inside the scan."""
    base = pad_header(H.synth_jpeg(**SEAM_KW), DAMAGE_PAD)
    s, e = scan_range(base)
    for name, d in files.items():
        kind, sn = name[4:name.rindex("_")], name[name.rindex("_") + 1:]
        front, b = DAMAGES[kind]
        g = DAMAGE_SEAMS[sn]
        lo = s - (s & 15) + g - front                               # file offset of the first byte written
        assert g % 4096 == 0 and (g % 16384 == 0) == (sn == "16k") and s < lo and lo + len(b) < e, name
        assert len(d) == len(base) and d[lo:lo + len(b)] == b and d[:lo] == base[:lo] and d[lo + len(b):] == base[lo + len(b):], name
        assert base[lo:lo + len(b)] != b, name                       # (bytes that were there already are no damage)
    assert len(files) == len(DAMAGES) * len(DAMAGE_SEAMS)


# ----------------------------------------------------------------------------------------------------------------- the records
def record(H, b, data):
    """What tests/golden/unstuff_seams.json keeps of one file decoded by backend b (digests and small numbers only)."""
    H.drive(b, data)
    r = {"sha256": H.hash_bytes(data)}
    dib = b.dib()
    if dib is None:
        r["preview"] = False
        return r
    r["dib"] = H.hash_bytes(dib)
    r["planes"] = [H.hash_bytes(p) if p is not None else None for p in b.planes()]
    r["mcu_map"] = H.hash_bytes(b.mcu_map())
    r["blk_dc"] = [H.hash_bytes(p) if p is not None else None for p in b.blk_dc()]
    r["status"] = {k: int(v) for k, v in b.status().items()}
    return r
