"""The carve contract in plain Python -- TEST INFRASTRUCTURE, the definition jsnoop_carve_run and jsnoop_carve_host are held to.

Written from the contract, not from the library: "next terminator" is a linear scan over the bytes, there are no lists to search, and `parent` is the
quadratic search its sentence describes.  `table(blob)` gives one dict per candidate (ascending start) with the fields of JsnoopCarveFrame;
`words(frame)` packs one the way a record lies in device memory; `lists(blob)` gives the terminator and candidate positions.
"""
from __future__ import annotations

OK, NO_SOS, NO_EOI, STOPPED, LIMIT = 0, 1, 2, 3, 4
NOT_A_MARKER, RST_OUTSIDE_SCAN, BAD_LENGTH, UNKNOWN_MARKER = 1, 2, 3, 4
SOI_AGAIN, DQT, DHT, DRI, AVI1 = 1, 2, 4, 8, 16
MAX_MARKERS = 4096
SOF_CODES = frozenset(range(0xC0, 0xD0)) - {0xC4, 0xC8, 0xCC}
FIELDS = ("start", "end", "status", "reason", "detail_pos", "detail_byte", "seen", "sof_code", "precision", "width", "height", "components",
          "sos_pos", "scan_start", "scans", "markers", "parent")


def is_terminator(b, i):
    n = len(b)
    if i >= n or b[i] != 0xFF:
        return False
    x = b[i + 1] if i + 1 < n else 0
    return x != 0x00 and not 0xD0 <= x <= 0xD7


def is_candidate(b, p):
    return p + 3 <= len(b) and b[p] == 0xFF and b[p + 1] == 0xD8 and b[p + 2] == 0xFF


def lists(b):
    return [i for i in range(len(b)) if is_terminator(b, i)], [p for p in range(len(b)) if is_candidate(b, p)]


def walk(b, p, max_markers=MAX_MARKERS):
    n = len(b)
    B = lambda i: b[i] if i < n else 0
    f = dict.fromkeys(FIELDS, 0)
    f.update(start=p, parent=-1)

    def done(status, end, reason=0, at=0, byte=0):
        f.update(status=status, end=end, reason=reason, detail_pos=at, detail_byte=byte, seen=seen, scans=scans, markers=markers)
        return f
    pos, markers, scans, seen = p, 0, 0, 0
    while True:
        if pos >= n:
            return done(NO_EOI, n)
        if B(pos) != 0xFF:
            return done(STOPPED, pos, NOT_A_MARKER, pos, B(pos))
        pos += 1
        code = B(pos); pos += 1
        while code == 0xFF:
            code = B(pos); pos += 1
        if pos > n:
            return done(NO_EOI, n)
        markers += 1
        if markers > max_markers:
            return done(LIMIT, pos - 1, 0, pos - 1, code)
        if code == 0xD8:
            if markers > 1:
                seen |= SOI_AGAIN
            continue
        if code == 0xD9:
            return done(OK if scans else NO_SOS, pos)
        if 0xD0 <= code <= 0xD7:
            return done(STOPPED, pos - 1, RST_OUTSIDE_SCAN, pos - 1, code)
        if 0xC0 <= code <= 0xFE or code == 0x01:
            ln = B(pos) * 256 + B(pos + 1)
            if ln < 2:
                return done(STOPPED, pos, BAD_LENGTH, pos, ln)
            if pos + ln > n:
                return done(NO_EOI, n)
            if code in SOF_CODES and not f["sof_code"]:
                f.update(sof_code=code, precision=B(pos + 2), height=B(pos + 3) * 256 + B(pos + 4), width=B(pos + 5) * 256 + B(pos + 6), components=B(pos + 7))
            seen |= {0xDB: DQT, 0xC4: DHT, 0xDD: DRI}.get(code, 0)
            if code == 0xE0 and bytes(B(pos + 2 + k) for k in range(4)) == b"AVI1":
                seen |= AVI1
            fpos = pos - 2                                            # the FF in front of the code
            pos += ln
            if code == 0xDA:
                scans += 1
                if scans == 1:
                    f.update(sos_pos=fpos, scan_start=pos)
                while pos < n and not is_terminator(b, pos):          # the least terminator >= pos
                    pos += 1
                if pos >= n:
                    return done(NO_EOI, n)
            continue
        return done(STOPPED, pos - 1, UNKNOWN_MARKER, pos - 1, code)


def table(b, max_markers=MAX_MARKERS):
    b = bytes(b)
    frames = [walk(b, p, max_markers) for p in range(len(b)) if is_candidate(b, p)]
    for k, f in enumerate(frames):
        holds = [j for j in range(k) if frames[j]["status"] == OK and frames[j]["start"] <= f["start"] < frames[j]["end"]]
        f["parent"] = max(holds, key=lambda j: frames[j]["start"]) if holds else -1
    return frames


def words(f):
    """The 16 words of a record in device memory (JSNOOP_CARVE_REC_WORDS; no parent)."""
    return [f["start"], f["end"], f["status"] | f["reason"] << 8 | (f["detail_byte"] & 255) << 16 | f["seen"] << 24, f["detail_pos"],
            f["sof_code"] | f["precision"] << 8 | f["components"] << 16, f["width"] | f["height"] << 16, f["sos_pos"], f["scan_start"], f["scans"], f["markers"],
            0, 0, 0, 0, 0, 0]
