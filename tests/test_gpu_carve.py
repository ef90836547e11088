"""GPU: jsnoop_carve_run against tests/carve_model.py -- every comparison exact.

Every container of tests/carve_cases.py and 300 seeded random blobs go through where = 0 (host bytes, the library's upload) and where = 1 (a torch tensor on
the device): the frame table equals the model's field for field, the records read back from device memory equal the model's words, and the two position
lists T and S read back equal the model's.  Seams: a 600-byte frame and the bare patterns FF D8 FF, FF D9, FF 00 FF D9 slid byte by byte across a lane's
16-byte edge, a wave's edge, a round's edge, a tile's edge, the start of the last partial tile and the end of the blob, for blob lengths of one tile +- 1 and three
tiles + 5 and device pointers 0, 1, 3 and 15 bytes off an aligned base (geometry from capi.CARVE_*).  What a placed pattern must yield is the model's table of
the pattern alone, moved: the background is zero bytes, which are no FF and stop a walk, so copies of the pattern at different edges of one blob do not see
each other.  (The frame's full slide runs for three tiles + 5; the one-tile lengths slide it over its first and last 24 positions at each edge, where its
SOI and EOI cross.)  Then: tiles without a mark, a tile that is all marks, more candidates than one walk workgroup, positions past 2^31, the scratch refusal,
and carve -> job end to end against the oracle, in Python and through the C++ wrapper."""
import os
import subprocess

import numpy as np
import pytest

import carve_cases as CC
import carve_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "carve_demo")


@pytest.fixture(scope="module")
def J():
    import jpegsnoop_amd
    jpegsnoop_amd.load()
    return jpegsnoop_amd


@pytest.fixture(scope="module")
def cases(harness):
    return CC.build_all(harness)


@pytest.fixture(scope="module")
def carve(J):
    c = J.Carve(0, max_scratch_bytes=1 << 30)
    yield c
    c.close()


def on_device(blob, off=0):
    """`blob` as a uint8 tensor whose first byte lies `off` bytes behind a 256-byte boundary."""
    import torch
    base = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda:0")
    assert base.data_ptr() % 256 == 0
    t = base[off:off + len(blob)]
    if len(blob):
        t.copy_(torch.from_numpy(np.frombuffer(blob, np.uint8).copy()))
    return t


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def check(carve, data, want, term, cand, what):
    assert carve.run(data) == len(want), what
    assert carve.frames() == want, what
    assert carve.totals() == (len(term), len(cand)), what
    assert u32(carve.frames_to_torch()).tolist() == [M.words(f) for f in want], what
    t, s = carve.lists_to_torch()
    assert u32(t).tolist() == term and u32(s).tolist() == cand, what


def test_every_case_through_host_bytes_and_device_tensors(carve, cases):
    for c in cases:
        mm = c.max_markers or M.MAX_MARKERS
        carve.set_spec(max_markers=c.max_markers, max_scratch_bytes=1 << 30)
        want = M.table(c.blob, mm); term, cand = M.lists(c.blob)
        check(carve, c.blob, want, term, cand, (c.name, "host"))
        check(carve, on_device(c.blob, 5), want, term, cand, (c.name, "device"))


def test_random_blobs_through_host_bytes_and_device_tensors(carve):
    carve.set_spec(max_markers=CC.RANDOM_MAX_MARKERS, max_scratch_bytes=1 << 30)
    for k, b in enumerate(CC.random_blobs()):
        want = M.table(b, CC.RANDOM_MAX_MARKERS); term, cand = M.lists(b)
        check(carve, b, want, term, cand, (k, "host"))
        check(carve, on_device(b, k % 16), want, term, cand, (k, "device"))


# ---------------------------------------------------------------------------------------------------------------------------------- seams
FRAME600 = CC.mini(scan=CC.junk(600 - len(CC.MINI)) + b"\x12\x34\x56")
PATTERNS = {"frame600": FRAME600, "soi_ff": b"\xFF\xD8\xFF", "eoi": b"\xFF\xD9", "ff00_eoi": b"\xFF\x00\xFF\xD9"}
_PLACED = {}


def placed(name, start, n):
    """What the pattern yields at `start` of an n-byte blob of zeros: (frames, T, S).  The model runs on the pattern with the few zero bytes a walk can still
    read behind it, cut at the blob's end; positions move by `start`, and an end of n (NO_EOI) is only taken from a run that ended at the blob's end."""
    pat = PATTERNS[name]
    room = min(len(pat) + 4, n - start)
    key = (name, room)
    if key not in _PLACED:
        small = (pat + b"\0" * 4)[:room]
        _PLACED[key] = (M.table(small), M.lists(small))
    frames, (term, cand) = _PLACED[key]
    out = []
    for f in frames:
        g = dict(f, start=f["start"] + start, end=f["end"] + start)
        assert f["status"] != M.NO_EOI or start + room == n
        if f["status"] in (M.STOPPED, M.LIMIT):
            g["detail_pos"] += start
        if f["scans"]:
            g["sos_pos"] += start; g["scan_start"] += start
        out.append(g)
    return out, [t + start for t in term], [s + start for s in cand]


def edges_of(n, head):
    """The seams of an n-byte blob `head` bytes behind a 16-byte boundary, as blob positions (a position e: the byte at e opens the next unit)."""
    from jpegsnoop_amd import capi
    end = head + n
    v = {capi.CARVE_LANE, capi.CARVE_WAVE, 4 * capi.CARVE_WAVE, capi.CARVE_TILE, (end - 1) // capi.CARVE_TILE * capi.CARVE_TILE, end}
    return sorted(e - head for e in v if 0 < e - head <= n)


def slide(carve, name, n, head, steps):
    pat = PATTERNS[name]; L = len(pat)
    edges = edges_of(n, head)
    for s in steps:
        groups = []                                                # copies of one blob keep L + 4 bytes apart; a copy that would not goes into a blob of its own
        for e in edges:
            start = e - L - 1 + s
            if 0 <= start < n:
                g = next((g for g in groups if start >= g[-1] + L + 4), None)
                g.append(start) if g is not None else groups.append([start])
        for g in groups:
            blob = bytearray(n); want, term, cand = [], [], []
            for start in g:
                blob[start:start + L] = pat[:n - start]
                f, t, c = placed(name, start, n)
                want += f; term += t; cand += c
            check(carve, on_device(bytes(blob), head), want, term, cand, (name, n, head, s, g))


@pytest.mark.parametrize("head", [0, 1, 3, 15])
def test_bare_patterns_slide_across_every_seam(carve, head):
    from jpegsnoop_amd import capi
    carve.set_spec(max_scratch_bytes=1 << 30)
    for n in (capi.CARVE_TILE - 1, capi.CARVE_TILE, capi.CARVE_TILE + 1, 3 * capi.CARVE_TILE + 5):
        for name in ("soi_ff", "eoi", "ff00_eoi"):
            slide(carve, name, n, head, range(len(PATTERNS[name]) + 3))


@pytest.mark.parametrize("head", [0, 1, 3, 15])
def test_a_600_byte_frame_slides_across_every_seam(carve, head):
    from jpegsnoop_amd import capi
    assert len(FRAME600) == 600 and M.table(FRAME600)[0]["status"] == M.OK
    carve.set_spec(max_scratch_bytes=1 << 30)
    slide(carve, "frame600", 3 * capi.CARVE_TILE + 5, head, range(603))
    for n in (capi.CARVE_TILE - 1, capi.CARVE_TILE, capi.CARVE_TILE + 1):
        slide(carve, "frame600", n, head, list(range(24)) + list(range(579, 603)))


def test_tiles_without_a_mark_a_tile_of_marks_and_many_candidates(carve):
    from jpegsnoop_amd import capi
    T = capi.CARVE_TILE
    carve.set_spec(max_markers=8, max_scratch_bytes=1 << 30)
    blob = bytearray(4 * T + 100)                                  # tile 0 empty, tile 1 all FF, tile 2 empty, tile 3 FF D8 pairs, a short tail
    blob[T:2 * T] = b"\xFF" * T
    blob[3 * T:4 * T] = b"\xFF\xD8" * (T // 2)
    blob = bytes(blob)
    term = list(range(T, 2 * T - 1)) + list(range(3 * T, 4 * T, 2))           # the FF run's last byte is followed by 00; every FF of a pair by D8
    cand = list(range(3 * T, 4 * T - 2, 2))
    assert len(cand) > capi.CARVE_WALK
    want = []
    for p in cand:                                                 # by construction: eight SOIs, the ninth marker is over the cap -- or the run ends in 00 first
        left = (4 * T - p) // 2                                    # pairs from p on
        if left > 8:
            want.append(dict(dict.fromkeys(M.FIELDS, 0), start=p, end=p + 17, status=M.LIMIT, detail_pos=p + 17, detail_byte=0xD8, seen=M.SOI_AGAIN, markers=9, parent=-1))
        else:
            want.append(dict(dict.fromkeys(M.FIELDS, 0), start=p, end=4 * T, status=M.STOPPED, reason=M.NOT_A_MARKER, detail_pos=4 * T, seen=M.SOI_AGAIN if left > 1 else 0,
                             markers=left, parent=-1))
    check(carve, on_device(blob, 3), want, term, cand, "marks")
    assert carve.frames()[-1] == want[-1] and want[-1]["start"] == 4 * T - 4 and want[-1]["markers"] == 2


def test_positions_past_2_to_the_31_come_back_unsigned(carve):
    import torch
    n = (1 << 31) + 8192
    carve.set_spec(max_scratch_bytes=1 << 30)
    big = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    frame = torch.from_numpy(np.frombuffer(FRAME600, np.uint8).copy()).cuda()
    a, b = (1 << 31) - 300, n - 600                                # one frame across offset 2^31, one ending at n
    big[a:a + 600] = frame; big[b:b + 600] = frame
    fa, ta, ca = placed("frame600", a, n); fb, tb, cb = placed("frame600", b, n)
    assert fb[0]["end"] == n and fb[0]["status"] == M.OK and fa[0]["start"] < (1 << 31) < fa[0]["end"]
    want, term, cand = [], [], []                                  # a mark every 16 MiB in front of them: every step of the prefix sums over the tile counts carries
    for j in range(128):
        name = ("soi_ff", "eoi")[j & 1]; at = (j << 24) + 4096 + j
        pat = torch.from_numpy(np.frombuffer(PATTERNS[name], np.uint8).copy()).cuda()
        big[at:at + len(pat)] = pat
        f, t, c = placed(name, at, n)
        want += f; term += t; cand += c
    assert len(want) == 64 and len(term) == 128                    # FF D8 FF 00: one terminator, one candidate; FF D9: one terminator
    check(carve, big, want + fa + fb, term + ta + tb, cand + ca + cb, "2^31")
    del big


def test_scratch_over_budget_is_refused_and_nothing_is_touched(carve, cases):
    ff = b"\xFF" * 4096
    t = on_device(ff, 0)
    c = next(c for c in cases if c.name == "exif_thumbnail")
    carve.set_spec(max_scratch_bytes=1 << 30)
    want = M.table(c.blob); term, cand = M.lists(c.blob)
    check(carve, c.blob, want, term, cand, "before")
    carve.set_spec(max_scratch_bytes=8192)                         # the terminator list alone needs 4 x 4095 bytes
    for data in (t, ff):
        with pytest.raises(RuntimeError, match="exceed max_scratch_bytes 8192"):
            carve.run(data)
        assert carve.frames() == want                              # the last table stands
    assert bytes(t.cpu().numpy()) == ff
    carve.set_spec(max_scratch_bytes=100)                          # a host blob's copy alone is over this budget: refused before anything is allocated
    with pytest.raises(RuntimeError, match="copy 4096.* exceed max_scratch_bytes 100"):
        carve.run(ff)
    assert carve.frames() == want
    carve.set_spec(max_scratch_bytes=1 << 30)
    check(carve, t, [], list(range(4095)), [], "all FF")
    check(carve, on_device(c.blob, 7), want, term, cand, "after")


def test_a_host_pointer_is_no_device_blob_and_the_default_budget_works(J, carve, cases):
    import ctypes as C
    from jpegsnoop_amd import capi
    lib = J.load()
    c = next(c for c in cases if c.name == "two_files_back_to_back")
    buf = (C.c_uint8 * len(c.blob)).from_buffer_copy(c.blob)
    spec = capi.CarveSpec(); lib.jsnoop_carve_spec_defaults(C.byref(spec))
    assert lib.jsnoop_carve_run(carve._h, C.byref(spec), buf, len(c.blob), 1) == -1 and b"is not memory of device 0" in lib.jsnoop_last_error()
    assert lib.jsnoop_carve_run(carve._h, C.byref(spec), buf, len(c.blob), 2) == -1 and b"where = 2" in lib.jsnoop_last_error()
    carve.set_spec()                                               # max_scratch_bytes 0: half of the device's free memory
    want = M.table(c.blob); term, cand = M.lists(c.blob)
    check(carve, c.blob, want, term, cand, "default budget")
    f = capi.CarveFrame(); f.struct_size = 12
    assert lib.jsnoop_carve_frame(carve._h, 1, C.byref(f)) == 0 and (f.struct_size, f.start, f.end, f.status) == (12, want[1]["start"], want[1]["end"], 0)
    assert lib.jsnoop_carve_frame(carve._h, 2, C.byref(f)) == -1 and b"out of range" in lib.jsnoop_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------- end to end
def oracle_dib(harness, oracle, data):
    harness.drive(oracle, data)
    return oracle.dib().copy()


def frame_files(c, frames):
    """Per OK frame the file a plain decoder needs for the same picture: blob[start:end] itself, or for the AVI-like case the frame with its DHT segments
    (an AVI1 frame has none: the decoder imports the standard tables, which are the ones the frame was coded with)."""
    ok = [f for f in frames if f["status"] == M.OK]
    if c.originals:
        assert len(ok) == len(c.originals)
        return ok, c.originals
    return ok, [c.blob[f["start"]:f["end"]] for f in ok]


@pytest.mark.parametrize("name", ["avi_like_avi1_frames_without_dht", "exif_thumbnail", "thumbnail_inside_thumbnail"])
def test_carve_to_job_decodes_every_frame_like_the_oracle(J, carve, cases, harness, oracle, name):
    c = next(c for c in cases if c.name == name)
    carve.set_spec(max_scratch_bytes=1 << 30)
    carve.run(c.blob)
    frames = carve.frames()
    ok, files = frame_files(c, frames)
    job = J.JpegJob(devices=[0])
    idx = job.add_carved(c.blob, frames)
    assert idx == list(range(len(ok))) and len(ok) == len(c.want)
    dibs = {}
    stats = job.run(lambda r: dibs.__setitem__(r.index, (r.status, r.batch.dib(r.image) if r.batch else None)) and None)
    assert stats["files"] == len(idx) and stats["ok"] == len(idx)
    for k, data in enumerate(files):
        assert dibs[k][0] == "ok" and np.array_equal(dibs[k][1], oracle_dib(harness, oracle, data)), (name, k)
    job.close()


def test_extract_all_through_the_cpp_wrapper(J, cases, harness, oracle, tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "carve_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir(); dst.mkdir()
    use = [next(c for c in cases if c.name == n) for n in ("avi_like_avi1_frames_without_dht", "exif_thumbnail")]
    for k, c in enumerate(use):
        (src / ("%d_%s.jpg" % (k, c.name))).write_bytes(c.blob)
    out = subprocess.check_output([EXE, str(src), str(dst)], text=True).strip().splitlines()
    assert out[0] == "listed 2", out
    want_lines, files = [], []
    for k, c in enumerate(use):
        rel = "%d_%s.jpg" % (k, c.name)
        tab = M.table(c.blob)
        for i, f in enumerate(tab):
            want_lines.append("frame %s k=%d start=%d end=%d status=%d parent=%d size=%dx%d" % (rel, i + 1, f["start"], f["end"], f["status"], f["parent"], f["width"], f["height"]))
        ok, ff = frame_files(c, tab)
        files += [(rel, tab.index(f) + 1, data) for f, data in zip(ok, ff)]
    nf = len(want_lines)
    assert out[1:1 + nf] == want_lines
    assert out[1 + nf] == "processed ok=%d files=%d refused=0 unreadable=0" % (len(files), len(files)), out
    assert out[-1] == "jobrun rc=0 wrote=1", out
    lines = sorted((l for l in out[2 + nf:-1]), key=lambda l: int(l.split()[1]))
    assert len(lines) == len(files)
    for j, (rel, k, data) in enumerate(files):
        dib = oracle_dib(harness, oracle, data)
        assert lines[j] == "file %d from=%s k=%d status=0 kind=1 size=%dx%d" % (j, rel, k, dib.shape[1], dib.shape[0]), lines[j]
        assert (dst / ("%d.dib" % j)).read_bytes() == dib.tobytes(), (rel, k)
        assert (dst / ("%s.%06d.txt" % (rel, k))).exists()
