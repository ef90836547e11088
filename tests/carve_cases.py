"""The catalogue of containers behind tests/test_carve_cases.py (CPU) and tests/test_gpu_carve.py (GPU) -- TEST INFRASTRUCTURE.

Every case is a blob with the frames it must yield STATED BY CONSTRUCTION: the builder knows where it put each frame and how its walk must end, and
says so in `want` (a list of dicts holding the fields it vouches for; `start`, `end`, `status` and `parent` always).  Nothing in `want` comes from running
tests/carve_model.py -- the CPU test holds the model to it.  Real frames come from harness.synth_jpeg (libjpeg), tests/base_stream.py (a token-level
baseline writer) and tests/prog_codec.py; `mini` frames are structural only (their scan bytes are no entropy-coded data) and are marked not well-formed.
"""
from __future__ import annotations

import numpy as np

import base_stream as BS
import carve_model as M
import prog_cases as PC
import prog_codec as P


class Case:
    def __init__(self, name, blob, want, max_markers=None, wellformed=True, originals=None):
        self.name, self.blob, self.want, self.max_markers, self.wellformed = name, bytes(blob), want, max_markers, wellformed
        self.originals = originals            # AVI-like list: the frame WITH its DHT segments, the file a plain decoder needs for the same picture


def fr(start, end, status, parent=-1, **more):
    return dict(start=start, end=end, status=status, parent=parent, **more)


def seg(marker, payload=b""):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def junk(n, salt=0):
    """n bytes without FF."""
    return bytes((i * 7 + 1 + salt) % 251 for i in range(n))


DQT = seg(0xDB, bytes([0]) + bytes(range(1, 65)))
SOF = seg(0xC0, bytes([8, 0, 9, 0, 17, 1, 1, 0x11, 0]))                   # 17 x 9, one component
DHT = seg(0xC4, bytes([0]) + bytes([0, 1] + [0] * 14) + bytes([0]))
SOS = seg(0xDA, bytes([1, 1, 0, 0, 63, 0]))
SOI, EOI = b"\xFF\xD8", b"\xFF\xD9"


def mini(scan=b"\x12\x34\x56", pre=b"", mid=b""):
    """A structurally complete frame: SOI [pre] DQT SOF0 DHT [mid] SOS scan EOI."""
    return SOI + pre + DQT + SOF + DHT + mid + SOS + scan + EOI


MINI = mini()
MINI_FIELDS = dict(sof_code=0xC0, precision=8, width=17, height=9, components=1, scans=1, markers=6, seen=M.DQT | M.DHT, reason=0,
                   sos_pos=len(SOI + DQT + SOF + DHT), scan_start=len(SOI + DQT + SOF + DHT + SOS))


def mini_at(off, parent=-1, body=MINI, **over):
    f = dict(MINI_FIELDS); f["sos_pos"] += off; f["scan_start"] += off; f.update(over)
    return fr(off, off + len(body), M.OK, parent, **f)


def without_dht_avi1(data):
    """A Motion-JPEG frame as an AVI holds it: APP0 'AVI1', no DHT (the decoder imports the standard tables), everything else as in `data`."""
    out, pos = [], 2
    while data[pos + 1] != 0xDA:
        ln = data[pos + 2] * 256 + data[pos + 3]
        out.append((data[pos + 1], bytes(data[pos + 4:pos + 2 + ln]))); pos += 2 + ln
    segs = [(m, (b"AVI1" + b"\0" * 10) if m == 0xE0 else b) for m, b in out if m != 0xC4]
    assert any(m == 0xE0 for m, _ in segs)
    return SOI + b"".join(seg(m, b) for m, b in segs) + bytes(data[pos:])


def base_stream_frame(dri):
    """A 2 x 2 MCU grey frame written token by token (tests/base_stream.py), with restart markers every `dri` MCUs."""
    frame = P.Frame(16, 16, [(1, 1, 0)], {0: PC.Q0})
    tabs = {(0, 0): P.flat_table(list(range(12)), 4), (1, 0): P.flat_table([0x00, 0x02, 0x11, 0xF0], 3)}
    blocks = [[40 * (k + 1), 3, 0, -1] + [0] * 60 for k in range(4)]
    return BS.write(frame, tabs, [(0, 0)], blocks, dri=dri).file


_BUILT = None


def build_all(H):
    """Every case, built once per process.  H: oracle/harness.py with the synth library built."""
    global _BUILT
    if _BUILT is not None:
        return _BUILT
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    J = H.synth_jpeg(width=48, height=32, hs=2, vs=2, quality=85, seed=7)
    J2 = H.synth_jpeg(width=40, height=24, hs=2, vs=1, quality=70, seed=8)
    TH = H.synth_jpeg(width=16, height=16, hs=1, vs=1, quality=60, seed=9)
    real = lambda off, data, w, h, parent=-1, **more: fr(off, off + len(data), M.OK, parent, width=w, height=h, scans=1, sof_code=0xC0, components=3, **more)

    add("bare_file", J, [real(0, J, 48, 32)])
    for k in (1, 3, 15, 1023):
        add("junk_%d_in_front" % k, junk(k) + J, [real(k, J, 48, 32)])
    add("two_files_back_to_back", J + J2, [real(0, J, 48, 32), real(len(J), J2, 40, 24)])

    app1 = lambda inner, pad: seg(0xE1, b"Exif\0\0" + junk(pad) + inner)
    thumbed = SOI + app1(TH, 5) + J[2:]
    t_at = 2 + 4 + 6 + 5
    add("exif_thumbnail", thumbed, [real(0, thumbed, 48, 32), real(t_at, TH, 16, 16, parent=0)])
    inner = SOI + app1(TH, 3) + J2[2:]                                      # a thumbnail that carries a thumbnail
    outer = SOI + app1(inner, 5) + J[2:]
    add("thumbnail_inside_thumbnail", outer,
        [real(0, outer, 48, 32), real(t_at, inner, 40, 24, parent=0), real(t_at + 2 + 4 + 6 + 3, TH, 16, 16, parent=1)])

    frames = [H.synth_jpeg(width=32, height=16 + 8 * k, hs=2, vs=2, quality=80, seed=20 + k) for k in range(3)]
    mj = [without_dht_avi1(f) for f in frames]
    blob = bytearray(b"RIFF" + (0).to_bytes(4, "little") + b"AVI LIST" + junk(24) + b"movi"); want = []
    for k, f in enumerate(mj):
        blob += b"00dc" + len(f).to_bytes(4, "little")
        want.append(real(len(blob), f, 32, 16 + 8 * k, seen=M.DQT | M.AVI1))
        blob += f + junk(1 + 2 * k, salt=k)                                 # odd paddings: no frame starts on a multiple of anything
    blob += b"idx1" + junk(16)
    add("avi_like_avi1_frames_without_dht", blob, want, wellformed=False, originals=frames)

    pf = PC.frame_of("2x2", 24, 16); script = PC.script_standard(3)
    assert len(script) == 10
    prog = P.encode_progressive(pf, PC.noise(pf, 5), script)
    add("progressive_ten_scans", prog, [fr(0, len(prog), M.OK, width=24, height=16, scans=10, sof_code=0xC2, components=3)])

    rst = H.synth_jpeg(width=48, height=32, hs=2, vs=2, quality=85, restart_interval=1, seed=11)
    assert b"\xFF\xD0" in rst and b"\xFF\xD4" in rst                    # six MCUs: RST0 .. RST4
    add("restart_markers", junk(7) + rst, [real(7, rst, 48, 32, seen=M.DQT | M.DHT | M.DRI)])
    bsf = base_stream_frame(1)
    assert bsf.count(b"\xFF\xD0") == 1 and bsf.count(b"\xFF\xD2") == 1
    add("restart_markers_token_writer", bsf, [fr(0, len(bsf), M.OK, width=16, height=16, scans=1, components=1, seen=M.DQT | M.DHT | M.DRI)])

    m = mini(scan=b"\x12\xFF\x00")
    add("stuffed_ff00_before_eoi", m, [mini_at(0, body=m)], wellformed=False)
    m = mini(scan=b"\xFF\x00\xFF\xD3\xFF\x00\x00\xFF\xD4\x77")
    add("stuffing_and_rst_inside_scan", m, [mini_at(0, body=m)], wellformed=False)
    m = SOI + b"\xFF\xFF\xFF" + DQT + SOF + DHT + b"\xFF" + SOS + b"\x12" + b"\xFF\xFF" + EOI      # (the FF run in front of EOI: every FF FF is a terminator)
    add("fill_bytes_before_markers", m, [fr(0, len(m), M.OK, markers=6, scans=1, sos_pos=len(SOI + DQT + SOF + DHT) + 4, scan_start=len(SOI + DQT + SOF + DHT + SOS) + 4)],
        wellformed=False)
    m = mini(pre=seg(0xFE, b"ab\xFF\xD9cd"))
    add("com_holding_eoi", m, [fr(0, len(m), M.OK, markers=7, scans=1)], wellformed=False)
    m = mini(pre=seg(0xFE, b"ab\xFF\xD8\xFF\x41cd"))
    add("com_holding_soi", m, [fr(0, len(m), M.OK, markers=7), fr(8, 11, M.STOPPED, 0, reason=M.UNKNOWN_MARKER, detail_pos=11, detail_byte=0x41, markers=2)], wellformed=False)

    cut = lambda name, n, **more: add(name, MINI[:n], [fr(0, n, M.NO_EOI, **more)], wellformed=False)
    cut("truncated_inside_a_header", len(SOI) + 20, markers=2, scans=0)            # inside DQT: its length passes the end
    cut("truncated_inside_scan_data", len(MINI) - 4, markers=5, scans=1)
    cut("truncated_after_the_final_ff", len(MINI) - 1, markers=5, scans=1)          # the last byte is FF: B(n) = 00 makes it no terminator
    m = SOI + DQT + b"\xFF"
    add("last_byte_ff_where_a_marker_belongs", m, [fr(0, len(m), M.NO_EOI, markers=2)], wellformed=False)
    for ln in (0, 1):
        m = SOI + b"\xFF\xE0" + bytes([0, ln]) + junk(6)
        add("length_%d" % ln, m, [fr(0, 4, M.STOPPED, reason=M.BAD_LENGTH, detail_pos=4, detail_byte=ln, markers=2)], wellformed=False)
    m = SOI + b"\xFF\xE0\x00\x10" + junk(3)
    add("length_past_the_end", m, [fr(0, len(m), M.NO_EOI, markers=2)], wellformed=False)
    for code in (0x00, 0x80):
        m = SOI + DQT + bytes([0xFF, code]) + junk(4)
        at = len(SOI + DQT) + 1
        add("ff_%02x_where_a_marker_belongs" % code, m, [fr(0, at, M.STOPPED, reason=M.UNKNOWN_MARKER, detail_pos=at, detail_byte=code, markers=3, seen=M.DQT)], wellformed=False)
    m = SOI + DQT + b"\x55" + junk(4)
    add("not_a_marker", m, [fr(0, len(SOI + DQT), M.STOPPED, reason=M.NOT_A_MARKER, detail_pos=len(SOI + DQT), detail_byte=0x55, markers=2)], wellformed=False)
    m = SOI + DQT + b"\xFF\xD3" + SOF + EOI
    add("rst_between_segments", m, [fr(0, len(SOI + DQT) + 1, M.STOPPED, reason=M.RST_OUTSIDE_SCAN, detail_pos=len(SOI + DQT) + 1, detail_byte=0xD3, markers=3)], wellformed=False)
    m = SOI + DQT + SOF + EOI
    add("eoi_without_sos", m, [fr(0, len(m), M.NO_SOS, markers=4, scans=0, sof_code=0xC0, width=17)], wellformed=False)
    m = SOI + seg(0x01, b"xy") + EOI                                              # TEM: the reference reads a length there
    add("tem_has_a_length", m, [fr(0, len(m), M.NO_SOS, markers=3)], wellformed=False)

    add("n_0", b"", [], wellformed=False)
    add("n_1", b"\xFF", [], wellformed=False)
    add("n_2", b"\xFF\xD8", [], wellformed=False)
    add("n_3", b"\xFF\xD8\xFF", [fr(0, 3, M.NO_EOI, markers=1)], wellformed=False)
    add("soi_ff_ends_exactly_at_n", junk(21) + b"\xFF\xD8\xFF", [fr(21, 24, M.NO_EOI, markers=1)], wellformed=False)
    add("soi_ff_one_short", junk(21) + b"\xFF\xD8", [], wellformed=False)

    MM = 8                                                                       # k pairs FF D8, then FF D9: candidate j walks k - j SOIs and the EOI
    for k in (MM - 2, MM - 1, MM, MM + 3):
        m = SOI * k + EOI; want = []
        for j in range(k):
            if k - j + 1 <= MM:
                want.append(fr(2 * j, len(m), M.NO_SOS, markers=k - j + 1, seen=M.SOI_AGAIN if k - j >= 2 else 0))
            else:                                                                 # marker MM + 1 is the SOI of pair j + MM, or the EOI where j + MM == k
                want.append(fr(2 * j, 2 * (j + MM) + 1, M.LIMIT, detail_pos=2 * (j + MM) + 1, detail_byte=0xD9 if j + MM == k else 0xD8, markers=MM + 1,
                               seen=M.SOI_AGAIN))
        add("soi_run_of_%d_with_max_markers_%d" % (k, MM), m, want, max_markers=MM, wellformed=False)

    add("ff_4096", b"\xFF" * 4096, [], wellformed=False)
    _BUILT = cases
    return cases


ALPHABET = bytes([0xFF, 0xD8, 0xD9, 0xDA, 0x00, 0xD0, 0xC0, 0x02, 0x10])
RANDOM_MAX_MARKERS = 3                  # SOI, SOS, EOI still fit: with this cap the model ends 21 of the 4232 walks below in LIMIT and 12 in OK
RANDOM_FRAMES_AND_LIMITS = (4232, 21)   # counted with tests/carve_model.py, which the case catalogue pins
_RANDOM = None


def random_blobs(count=300, seed=20261019):
    """Seeded blobs over an alphabet that makes markers dense; lengths 0 .. 2499."""
    global _RANDOM
    if _RANDOM is None or len(_RANDOM) != count:
        rng = np.random.default_rng(seed)
        w = np.array([6, 4, 3, 2, 3, 1, 2, 1, 2], float); w /= w.sum()
        _RANDOM = [bytes(np.frombuffer(ALPHABET, np.uint8)[rng.choice(len(ALPHABET), size=int(rng.integers(0, 2500)), p=w)]) for _ in range(count)]
    return _RANDOM
