"""A plain JPEG codec (ITU-T T.81 Annex F sequential, Annex G progressive, Huffman) in Python / numpy -- TEST INFRASTRUCTURE.

Written from the standard as a second derivation of what jpegsnoop_amd/csrc/jsnoop_progressive.hip computes: deliberately
sequential and simple (one symbol at a time, one block at a time), nothing of the kernels' structure.  The refinement coder
follows T.81 G.1.2.3 (Figures G.7 - G.9) in the reading libjpeg's jcphuff.c / jdphuff.c give it.

Conventions
* A frame is plain data: `Frame(width, height, comps, qtabs)`, comps = [(H, V, Tq), ...] for 1 or 3 components, qtabs =
  {Tq: 64 quantiser values in ZIG-ZAG order}.  A frame of ONE component has one block per MCU whatever H, V it declares
  (T.81 A.2.3: a scan of one component is not interleaved), so its grid is ceil(X / 8) x ceil(Y / 8).
* Coefficients: one int16 array [blocks_y, blocks_x, 64] per component in ZIG-ZAG order (index k = the position Ss..Se speak
  of; natural index = ZIGZAG[k]) over the PADDED grid (whole MCUs: mcu_y * V rows of mcu_x * H blocks).  Non-interleaved scans
  code the top-left `coded(c)` part of that grid only (A.2.3); what they leave alone stays as earlier scans left it.
* A script is a list of scans; a scan is a tuple (components, Ss, Se, Ah, Al) or a dict with those keys (`comps ss se ah al`)
  plus the optional `dri` (restart interval in force from this scan on; a DRI segment is written when it changes), `dc_tab` /
  `ac_tab` ((counts[16], symbols) tables handed in instead of the optimal ones, or a function of the scan's symbol
  frequencies that returns one; dc_tab is a list per scan component), `dc_ids`
  / `ac_id` (table destinations 0..3) and `extra_dht` (list of (class, id, table) segments written in front of the scan).
  Two hooks write IRREGULAR streams token by token (tests/prog_damage_cases.py): `tokens` (a function of the scan's token list
  that returns the list to code instead; the optimal tables are made from what it returns, so a symbol no encoder would write
  still gets a code) and `bytes` (a function of the scan's entropy-coded bytes, RSTn markers included, that returns the bytes
  to write instead).
* `decode(file)` -> Decoded: frame, coefficient arrays as a conforming decoder holds them at EOI, and one event record per
  scan (see `decode`).  It asserts on the first irregular symbol: it is the STRICT mode.
* `decode(file, lenient=True)` -> what a decoder that goes on after damage holds at EOI, by the rules in front of
  `_decode_scan_lenient` (T.81 Annex G plus the damage contract of DESIGN.md 4.5), with the record of what went wrong where.
"""
from __future__ import annotations

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34,
          27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
          58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _cdiv(a, b):
    return -(-a // b)


class Frame:
    def __init__(self, width, height, comps, qtabs):
        self.width, self.height = int(width), int(height)
        self.comps = [tuple(int(x) for x in c) for c in comps]
        self.qtabs = {int(k): [int(x) for x in v] for k, v in qtabs.items()}
        assert len(self.comps) in (1, 3) and all(1 <= h <= 4 and 1 <= v <= 4 for h, v, _ in self.comps)
        self.ncomp = len(self.comps)
        # sampling that takes part in the MCU: a lone component is never interleaved
        self.hv = [(1, 1)] if self.ncomp == 1 else [(h, v) for h, v, _ in self.comps]
        self.hmax = max(h for h, _ in self.hv); self.vmax = max(v for _, v in self.hv)
        self.mcu_x = _cdiv(self.width, 8 * self.hmax); self.mcu_y = _cdiv(self.height, 8 * self.vmax)

    def grid(self, c):
        """(blocks_y, blocks_x) of component c's padded grid."""
        h, v = self.hv[c]
        return self.mcu_y * v, self.mcu_x * h

    def coded(self, c):
        """(nby, nbx): the part of the grid a non-interleaved scan of component c codes (A.2.3)."""
        h, v = self.hv[c]
        return _cdiv(_cdiv(self.height * v, self.vmax), 8), _cdiv(_cdiv(self.width * h, self.hmax), 8)

    def zeros(self):
        return [np.zeros(self.grid(c) + (64,), np.int16) for c in range(self.ncomp)]

    def coded_mask(self, c):
        m = np.zeros(self.grid(c), bool); nby, nbx = self.coded(c); m[:nby, :nbx] = True
        return m

    def mcu_blocks(self):
        """[(component, v, h)] of the blocks of one MCU in coding order (A.2.2)."""
        return [(c, v, h) for c in range(self.ncomp) for v in range(self.hv[c][1]) for h in range(self.hv[c][0])]


# ------------------------------------------------------------------------------------------------------------ Huffman tables
def optimal_table(freq):
    """T.81 K.2 (Figures K.1 - K.4): code lengths from symbol frequencies, limited to 16 bits; one code point is reserved so
    that no code is all ones.  Returns (counts[16], symbols)."""
    f = {int(s): int(n) for s, n in freq.items() if n > 0}
    if not f:
        f = {0: 1}
    f[256] = 1
    codesize = {s: 0 for s in f}; others = {s: -1 for s in f}
    while True:
        live = [s for s in f if f[s] > 0]
        if len(live) < 2:
            break
        c1 = min(live, key=lambda s: (f[s], -s))
        c2 = min((s for s in live if s != c1), key=lambda s: (f[s], -s))
        f[c1] += f[c2]; f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]; codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]; codesize[c2] += 1
    bits = [0] * 300
    for s, n in codesize.items():
        bits[n] += 1
    i = max(k for k in range(300) if bits[k])
    while i > 16:                                     # Figure K.3: Adjust_BITS
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                      # the reserved code point
    syms = [s for _n, s in sorted((codesize[s], s) for s in codesize if s != 256)]
    return bits[1:17], syms


def ladder_table(symbols, first_len=1, ladder=8):
    """A legal but lopsided table: symbols[0 .. ladder-1] get one code each of first_len, first_len + 1, ... bits, every
    further symbol a 16-bit code (first_len = 9 and ladder = 0..: only long codes)."""
    counts = [0] * 16; n = min(ladder, len(symbols)); ln = first_len
    for _ in range(n):
        counts[ln - 1] += 1; ln += 1
    assert ln <= 16 or n == len(symbols)
    counts[15] += len(symbols) - n
    return counts, list(symbols)


def flat_table(symbols, length):
    """Every symbol a code of `length` bits."""
    counts = [0] * 16; counts[length - 1] = len(symbols)
    assert len(symbols) < (1 << length)
    return counts, list(symbols)


def _codes(table):
    """(counts, symbols) -> {symbol: (code, length)} (Annex C)."""
    counts, syms = table
    out = {}; code = 0; k = 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            assert code < (1 << ln), "over-subscribed Huffman table"
            out[syms[k]] = (code, ln); code += 1; k += 1
        code <<= 1
    return out


_LUT_CACHE = {}


def _lut16(table):
    """16-bit look-ahead: list of 65536 entries (length << 8 | symbol), 0 where no code matches."""
    key = (tuple(table[0]), tuple(table[1]))
    lut = _LUT_CACHE.get(key)
    if lut is None:
        a = np.zeros(65536, np.int32)
        for s, (code, ln) in _codes(table).items():
            a[code << (16 - ln): (code + 1) << (16 - ln)] = (ln << 8) | s
        lut = a.tolist()
        if len(_LUT_CACHE) > 400:
            _LUT_CACHE.clear()
        _LUT_CACHE[key] = lut
    return lut


# ------------------------------------------------------------------------------------------------------------------- encoder
class _Bits:
    """MSB-first bit writer with byte stuffing (B.1.1.5); the final byte is padded with ones (F.1.2.3)."""

    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0

    def put(self, v, n):
        if not n:
            return
        self.acc = (self.acc << n) | (v & ((1 << n) - 1)); self.n += n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _dht(cls, ident, table):
    counts, syms = table
    return _seg(0xC4, bytes([cls << 4 | ident]) + bytes(counts) + bytes(syms))


def _head(frame, sof, com_len):
    out = bytearray(b"\xFF\xD8")
    if com_len is not None:
        assert com_len >= 0
        out += _seg(0xFE, bytes((i * 7 + 1) % 251 % 255 for i in range(com_len)))     # (no FF inside)
    for tq, q in sorted(frame.qtabs.items()):
        big = max(q) > 255
        out += _seg(0xDB, bytes([(16 if big else 0) | tq]) + (b"".join(x.to_bytes(2, "big") for x in q) if big else bytes(q)))
    p = bytes([8]) + frame.height.to_bytes(2, "big") + frame.width.to_bytes(2, "big") + bytes([frame.ncomp])
    for c, (h, v, tq) in enumerate(frame.comps):
        p += bytes([c + 1, h << 4 | v, tq])
    return out + _seg(sof, p)


def _norm_scan(s):
    if isinstance(s, dict):
        d = dict(s)
    else:
        comps, ss, se, ah, al = s
        d = dict(comps=comps, ss=ss, se=se, ah=ah, al=al)
    d["comps"] = [int(c) for c in ([d["comps"]] if np.isscalar(d["comps"]) else d["comps"])]
    return d


def _category(a):
    return int(a).bit_length()


# tokens of a scan: (0, table slot, symbol) | (1, value, nbits) | (2, restart number, 0) | (3, bits to drop, 0): see _emit
def _scan_tokens(frame, coefs, sc, ri, max_corr=937):
    ss, se, ah, al, comps = sc["ss"], sc["se"], sc["ah"], sc["al"], sc["comps"]
    T = []
    rst = [0]

    def restart():
        T.append((2, rst[0] & 7, 0)); rst[0] += 1

    if ss == 0:                                                                   # ---- DC (G.1.2.1)
        assert se == 0
        if len(comps) > 1:
            units = frame.mcu_x * frame.mcu_y
            def blocks(u):
                my, mx = divmod(u, frame.mcu_x)
                for slot, c in enumerate(comps):
                    h, v = frame.hv[c]
                    for y in range(v):
                        for x in range(h):
                            yield slot, c, my * v + y, mx * h + x
        else:
            nby, nbx = frame.coded(comps[0]); units = nby * nbx
            def blocks(u):
                yield 0, comps[0], u // nbx, u % nbx
        pred = [0] * len(comps)
        for u in range(units):
            if ri and u and u % ri == 0:
                restart(); pred = [0] * len(comps)
            for slot, c, by, bx in blocks(u):
                v = int(coefs[c][by, bx, 0]) >> al                                 # arithmetic shift (G.1.2.1)
                if ah == 0:
                    d = v - pred[slot]; pred[slot] = v
                    n = _category(abs(d)); assert n <= 11, "DC difference out of range"
                    T.append((0, slot, n))
                    if n:
                        T.append((1, d if d >= 0 else d - 1, n))
                else:
                    T.append((1, v & 1, 1))
        return T

    assert len(comps) == 1 and 1 <= ss <= se <= 63
    c = comps[0]; nby, nbx = frame.coded(c); units = nby * nbx
    band = coefs[c][:nby, :nbx, ss:se + 1].astype(np.int32).reshape(units, se - ss + 1)
    mag = np.abs(band) >> al                                                      # AC point transform: towards zero (G.1.2.2)
    busy = (mag != 0).any(1)
    eobrun = 0; be = []                                                          # pending run and its buffered correction bits

    def emit_eobrun():
        nonlocal eobrun, be
        if eobrun:
            n = eobrun.bit_length() - 1
            T.append((0, 0, n << 4))
            if n:
                T.append((1, eobrun & ((1 << n) - 1), n))
            eobrun = 0
        for b in be:
            T.append((1, b, 1))
        be = []

    for u in range(units):
        if ri and u and u % ri == 0:
            emit_eobrun(); restart()
        if not busy[u]:
            eobrun += 1
            if eobrun == 0x7FFF:
                emit_eobrun()
            continue
        row = band[u]; m = mag[u]
        if ah == 0:                                                               # ---- AC first (G.1.2.2)
            r = 0
            for i in range(se - ss + 1):
                t = int(m[i])
                if not t:
                    r += 1; continue
                if eobrun:
                    emit_eobrun()
                while r > 15:
                    T.append((0, 0, 0xF0)); r -= 16
                n = _category(t); assert n <= 10
                T.append((0, 0, (r << 4) | n))
                T.append((1, t if row[i] >= 0 else ~t, n))
                r = 0
            if r:
                eobrun += 1
                if eobrun == 0x7FFF:
                    emit_eobrun()
        else:                                                                     # ---- AC refinement (G.1.2.3)
            ones = np.nonzero(m == 1)[0]
            eob = int(ones[-1]) if len(ones) else -1                              # last newly non-zero coefficient
            r = 0; br = []
            for i in range(se - ss + 1):
                t = int(m[i])
                if not t:
                    r += 1; continue
                while r > 15 and i <= eob:
                    emit_eobrun(); T.append((0, 0, 0xF0)); r -= 16
                    for b in br:
                        T.append((1, b, 1))
                    br = []
                if t > 1:
                    br.append(t & 1); continue
                emit_eobrun()
                T.append((0, 0, (r << 4) | 1)); T.append((1, 0 if row[i] < 0 else 1, 1))
                for b in br:
                    T.append((1, b, 1))
                br = []; r = 0
            if r or br:
                eobrun += 1; be += br
                if eobrun == 0x7FFF or len(be) > max_corr:
                    emit_eobrun()
    emit_eobrun()
    return T


def _emit(tokens, tables):
    """tokens -> list of interval byte strings (between them: RSTn).  Token kind 3 (tests/prog_damage_cases.py) CUTS the interval:
    (3, n, 0) drops the last n bits written and what is then left of a begun byte (the interval ends on a whole byte, without
    the padding ones), and every further token of the interval."""
    codes = [_codes(t) if t is not None else None for t in tables]
    ivs = []; w = _Bits(); wrote = []; dead = False
    for kind, a, b in tokens:
        if kind == 2:
            if not dead:
                w.flush()
            ivs.append((bytes(w.out), a)); w = _Bits(); wrote = []; dead = False
        elif dead:
            continue
        elif kind == 3:
            keep = max(0, sum(n for _v, n in wrote) - a) // 8 * 8
            w = _Bits(); dead = True
            for v, n in wrote:
                n2 = min(n, keep); w.put(v >> (n - n2), n2); keep -= n2
        else:
            v, n = codes[a][b] if kind == 0 else (a, b)
            w.put(v, n); wrote.append((v & ((1 << n) - 1), n))
    if not dead:
        w.flush()
    ivs.append((bytes(w.out), None))
    out = bytearray()
    for data, r in ivs:
        out += data
        if r is not None:
            out += bytes([0xFF, 0xD0 + r])
    return bytes(out)


def _freq(tokens, nslots):
    f = [dict() for _ in range(nslots)]
    for kind, a, b in tokens:
        if kind == 0:
            f[a][b] = f[a].get(b, 0) + 1
    return f


def encode_progressive(frame, coefs, script, com_len=None, max_corr=937):
    out = bytearray(_head(frame, 0xC2, com_len))
    ri = 0
    for s in script:
        sc = _norm_scan(s)
        want = sc.get("dri")
        if want is not None and want != ri:
            ri = int(want); out += _seg(0xDD, ri.to_bytes(2, "big"))
        tokens = _scan_tokens(frame, coefs, sc, ri, max_corr)
        if sc.get("tokens") is not None:
            tokens = list(sc["tokens"](tokens))
        ns = len(sc["comps"]); dc = sc["ss"] == 0
        for cls, ident, tab in sc.get("extra_dht", []):
            out += _dht(cls, ident, tab)
        tables = [None] * ns; ids = [0] * ns
        if dc and sc["ah"] == 0:
            freq = _freq(tokens, ns); given = sc.get("dc_tab") or [None] * ns
            ids = list(sc.get("dc_ids") or range(ns))
            for i in range(ns):
                tables[i] = optimal_table(freq[i]) if given[i] is None else (given[i](freq[i]) if callable(given[i]) else given[i])
                out += _dht(0, ids[i], tables[i])
        elif not dc:
            freq = _freq(tokens, 1)
            given = sc.get("ac_tab")
            tables[0] = optimal_table(freq[0]) if given is None else (given(freq[0]) if callable(given) else given); ids = [sc.get("ac_id", 0)]
            out += _dht(1, ids[0], tables[0])
        p = bytes([ns])
        for i, c in enumerate(sc["comps"]):
            p += bytes([c + 1, (ids[i] << 4) if dc else ids[i]])
        p += bytes([sc["ss"], sc["se"], sc["ah"] << 4 | sc["al"]])
        ecs = _emit(tokens, tables)
        if sc.get("bytes") is not None:
            ecs = bytes(sc["bytes"](ecs))
        out += _seg(0xDA, p) + ecs
    return bytes(out + b"\xFF\xD9")


def encode_baseline(frame, coefs, dri=0):
    """Sequential SOF0 file of the same coefficients: one scan of all components (Annex F)."""
    T = []
    units = frame.mcu_x * frame.mcu_y; blocks = frame.mcu_blocks(); pred = [0] * frame.ncomp; nr = 0
    for u in range(units):
        if dri and u and u % dri == 0:
            T.append((2, nr & 7, 0)); nr += 1; pred = [0] * frame.ncomp
        my, mx = divmod(u, frame.mcu_x)
        for c, y, x in blocks:
            h, v = frame.hv[c]
            blk = coefs[c][my * v + y, mx * h + x]
            d = int(blk[0]) - pred[c]; pred[c] = int(blk[0])
            n = _category(abs(d)); assert n <= 11
            T.append((0, 2 * c, n))
            if n:
                T.append((1, d if d >= 0 else d - 1, n))
            r = 0
            nzk = np.nonzero(blk[1:])[0]
            last = 0
            for i in nzk:
                k = int(i) + 1; r = k - last - 1; last = k
                while r > 15:
                    T.append((0, 2 * c + 1, 0xF0)); r -= 16
                t = int(blk[k]); n = _category(abs(t)); assert n <= 10
                T.append((0, 2 * c + 1, (r << 4) | n)); T.append((1, t if t >= 0 else t - 1, n))
            if last != 63:
                T.append((0, 2 * c + 1, 0))
    # components 1 and 2 share tables (ids 1), component 0 has its own (ids 0)
    def slot(i):
        return i if i < 2 else (i % 2) + 2
    T = [(k, slot(a), b) if k == 0 else (k, a, b) for k, a, b in T]
    freq = _freq(T, 4)
    tabs = [optimal_table(freq[i]) for i in range(4)]
    out = bytearray(_head(frame, 0xC0, None))
    if dri:
        out += _seg(0xDD, int(dri).to_bytes(2, "big"))
    ntab = 1 if frame.ncomp == 1 else 2
    for t in range(ntab):
        out += _dht(0, t, tabs[2 * t]) + _dht(1, t, tabs[2 * t + 1])
    p = bytes([frame.ncomp])
    for c in range(frame.ncomp):
        t = 0 if c == 0 else 1
        p += bytes([c + 1, t << 4 | t])
    out += _seg(0xDA, p + bytes([0, 63, 0])) + _emit(T, tabs)
    return bytes(out + b"\xFF\xD9")


# ------------------------------------------------------------------------------------------------------------------- decoder
class _Reader:
    """Bits of one restart interval, MSB first, stuffing already removed; past the end: zeros, counted."""

    def __init__(self, data):
        self.v = int.from_bytes(data + b"\0" * 8, "big"); self.total = (len(data) + 8) * 8; self.len = len(data) * 8; self.pos = 0

    def peek16(self):
        sh = self.total - self.pos - 16
        return (self.v >> sh) & 0xFFFF if sh >= 0 else 0

    def bits(self, n):
        if not n:
            return 0
        sh = self.total - self.pos - n; self.pos += n
        return (self.v >> sh) & ((1 << n) - 1) if sh >= 0 else 0


class _Chunked:
    """The same over a long interval, without one huge integer shift per call."""

    def __init__(self, data):
        self.d = data + b"\0" * 16; self.len = len(data) * 8; self.pos = 0

    def peek16(self):
        i = self.pos >> 3
        return (int.from_bytes(self.d[i:i + 3], "big") >> (8 - (self.pos & 7))) & 0xFFFF if i + 3 <= len(self.d) else 0

    def bits(self, n):
        if not n:
            return 0
        i = self.pos >> 3; sh = 40 - (self.pos & 7) - n; self.pos += n
        return (int.from_bytes(self.d[i:i + 5], "big") >> sh) & ((1 << n) - 1) if i + 5 <= len(self.d) else 0


def _extend(v, n):
    return v - (1 << n) + 1 if v < (1 << (n - 1)) else v              # F.2.2.1


class Decoded:
    def __init__(self):
        self.frame = None; self.sof = 0; self.coefs = None; self.scans = []; self.dht_defs = []


def _split_intervals(f, start):
    """Entropy-coded data from `start`: [(file offset, unstuffed bytes, end offset)] per restart interval, offsets of the
    FF 00 pairs, offset of the marker that ends the scan."""
    ivs = []; ff00 = []; cur = bytearray(); s0 = start; q = start; n = len(f)
    while q < n:
        b = f[q]
        if b != 0xFF:
            cur.append(b); q += 1; continue
        nx = f[q + 1] if q + 1 < n else 0xD9
        if nx == 0:
            ff00.append(q); cur.append(0xFF); q += 2
        elif 0xD0 <= nx <= 0xD7:
            ivs.append((s0, bytes(cur), q)); cur = bytearray(); q += 2; s0 = q
        elif nx == 0xFF:
            q += 1
        else:
            break
    ivs.append((s0, bytes(cur), q))
    return ivs, ff00, q


def decode(f, lenient=False, variant=None):
    """Decodes a SOF0 / SOF2 Huffman file sequentially.  Returns Decoded with .frame, .coefs and .scans: per scan a dict
    comps ss se ah al dri, start / end (file offsets of the entropy data), intervals [(start, end)], ff00 [file offsets],
    eobruns [(unit the run starts on, length as coded, i.e. including that block)], eob_after_coefs (EOBn symbols read after at
    least one coefficient of the same block), zrl [(unit, position k before the ZRL, position after it)], stretches [(correction bits, kind,
    unit)] with kind 'sym' / 'zrl' (read while a (run, 1) symbol / a ZRL is worked off) or 'tail' (after EOBn / inside a run), max_code
    (longest Huffman code used), code_lens (histogram 1..16), dc_ids / ac_ids (table destinations), units, overrun.

    lenient=True (SOF2 only; the file may end anywhere behind its first SOS): nothing in the entropy-coded data is refused.  Decoded
    gains .flagged (what JSNOOP_FLAG_BAD_CODE must say) and per scan: units, want (intervals the scan needs), stops [(interval,
    unit, reason)] with reason 'no_code' / 'dc_category' / 'run_past_se' / 'refine_s', overran [(interval, unit, what was being
    read when the first bit that was never there was consumed: 'code' / 'value' / 'sign' / 'correction' / 'eob_length' / 'dc_bit')], missing / surplus (interval counts), irregular [(interval, unit, what)] for what is accepted: 'dc_wide'
    (category 12..15), 'zrl_out' (a ZRL that leaves the band), 'run_out' (a refinement run longer than the zeros left),
    'bit_set' (a correction bit on a coefficient whose bit Al is set), 'eobrun_cut' (an end-of-band run that outlasts its
    interval).  `variant` names one deliberately WRONG reading of the contract (tests/test_prog_damage_cases.py shows that the
    catalogue refuses each): 'stop_scan', 'discard_block', 'refuse_dc12', 'flag_surplus', 'no_flag_missing', 'carry_eobrun'."""
    D = Decoded(); n = len(f); assert f[:2] == b"\xFF\xD8"
    if lenient:
        D.flagged = False
    dht = {}; qt = {}; ri = 0; pos = 2; frame = None
    while pos + 4 <= n:
        assert f[pos] == 0xFF, "marker expected at %d" % pos
        while f[pos + 1] == 0xFF:
            pos += 1
        m = f[pos + 1]; pos += 2
        if m == 0xD9:
            break
        ln = int.from_bytes(f[pos:pos + 2], "big"); seg = f[pos + 2:pos + ln]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15; i += 1
                if pq:
                    qt[tq] = [int.from_bytes(seg[i + 2 * k:i + 2 * k + 2], "big") for k in range(64)]; i += 128
                else:
                    qt[tq] = list(seg[i:i + 64]); i += 64
        elif m in (0xC0, 0xC1, 0xC2):
            assert seg[0] == 8
            comps = [(seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
            ids = [seg[6 + 3 * c] for c in range(seg[5])]
            frame = Frame(int.from_bytes(seg[3:5], "big"), int.from_bytes(seg[1:3], "big"), comps, qt)
            D.frame = frame; D.sof = m; D.coefs = frame.zeros()
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15; counts = list(seg[i + 1:i + 17]); tot = sum(counts)
                dht[(tc, th)] = (counts, list(seg[i + 17:i + 17 + tot])); i += 17 + tot
                D.dht_defs.append((tc, th, dht[(tc, th)]))
        elif m == 0xDD:
            ri = int.from_bytes(seg[:2], "big")
        elif m == 0xDA:
            frame.qtabs = dict(qt)
            ns = seg[0]
            sc = dict(comps=[ids.index(seg[1 + 2 * i]) for i in range(ns)], ss=seg[1 + 2 * ns], se=seg[2 + 2 * ns],
                      ah=seg[3 + 2 * ns] >> 4, al=seg[3 + 2 * ns] & 15, dri=ri,
                      dc_ids=[seg[2 + 2 * i] >> 4 for i in range(ns)], ac_ids=[seg[2 + 2 * i] & 15 for i in range(ns)])
            start = pos + ln
            if lenient:
                assert D.sof == 0xC2
                ivs, end = _split_intervals_lenient(f, start)
                sc.update(start=start, end=end, intervals=[(a, e) for a, _d, e in ivs])
                _decode_scan_lenient(D, sc, [d for _a, d, _e in ivs], dht, variant)
                D.scans.append(sc)
                pos = end; continue
            ivs, ff00, end = _split_intervals(f, start)
            sc.update(start=start, end=end, ff00=ff00, intervals=[(a, e) for a, _d, e in ivs])
            _decode_scan(D, sc, [d for _a, d, _e in ivs], dht)
            D.scans.append(sc)
            pos = end; continue
        pos += ln
    return D


def _decode_scan(D, sc, ivs, dht):
    frame, coefs = D.frame, D.coefs
    ss, se, ah, al, comps = sc["ss"], sc["se"], sc["ah"], sc["al"], sc["comps"]
    ev = dict(eobruns=[], eob_after_coefs=0, zrl=[], stretches=[], max_code=0, code_lens=[0] * 17, overrun=0)
    sc.update(ev)
    lens = sc["code_lens"]
    seq = D.sof != 0xC2
    if seq:
        assert ss == 0 and se == 63 and ah == 0 and al == 0
    inter = len(comps) > 1
    if inter or (seq and frame.ncomp > 1):
        assert len(comps) == frame.ncomp or not seq
        units = frame.mcu_x * frame.mcu_y
    else:
        nby, nbx = frame.coded(comps[0]); units = nby * nbx
    sc["units"] = units
    ri = sc["dri"] or units
    assert len(ivs) >= _cdiv(units, ri), "fewer restart intervals than the scan needs"
    dc_lut = [_lut16(dht[(0, i)]) if (ss == 0 and ah == 0) else None for i in sc["dc_ids"]]
    ac_lut = [_lut16(dht[(1, i)]) if se > 0 else None for i in sc["ac_ids"]]

    def huff(r, lut):
        e = lut[r.peek16()]
        assert e, "no Huffman code matches"
        ln = e >> 8; r.pos += ln; lens[ln] += 1
        return e & 255

    def unit_blocks(u):
        if inter or (seq and frame.ncomp > 1):
            my, mx = divmod(u, frame.mcu_x)
            for slot, c in enumerate(comps):
                h, v = frame.hv[c]
                for y in range(v):
                    for x in range(h):
                        yield slot, coefs[c][my * v + y, mx * h + x]
        else:
            yield 0, coefs[comps[0]][u // nbx, u % nbx]

    hist_any = None
    if ss > 0 and ah:
        c = comps[0]
        hist_any = (coefs[c][:nby, :nbx, ss:se + 1] != 0).any(2).reshape(-1)
    p1, m1 = 1 << al, -(1 << al)
    for iv in range(_cdiv(units, ri)):
        data = ivs[iv]
        r = _Reader(data) if len(data) < 512 else _Chunked(data)
        u0, u1 = iv * ri, min(units, iv * ri + ri)
        pred = [0] * len(comps); eobrun = 0
        u = u0
        while u < u1:
            if ss > 0 and eobrun and (not ah or not hist_any[u]):      # a block inside an end-of-band run with nothing to read
                if ah:
                    eobrun -= 1; u += 1
                else:
                    hop = min(eobrun, u1 - u); eobrun -= hop; u += hop
                continue
            for slot, blk in unit_blocks(u):
                if ss == 0:
                    if ah == 0:                                        # DC first / sequential DC (F.2.2.1, G.1.2.1)
                        s = huff(r, dc_lut[slot]); assert s <= 11
                        pred[slot] += _extend(r.bits(s), s) if s else 0
                        blk[0] = np.int16(pred[slot] << al)
                    elif r.bits(1):
                        blk[0] |= np.int16(p1)
                if seq:                                                # sequential AC (F.2.2.2)
                    k = 1; lut = ac_lut[slot]
                    while k <= 63:
                        rs = huff(r, lut); rr, s = rs >> 4, rs & 15
                        if s == 0:
                            if rr != 15:
                                break
                            k += 16; continue
                        k += rr; assert k <= 63
                        blk[k] = _extend(r.bits(s), s); k += 1
                elif ss > 0 and ah == 0:                               # AC first (G.1.2.2)
                    k = ss; lut = ac_lut[0]
                    while k <= se:
                        rs = huff(r, lut); rr, s = rs >> 4, rs & 15
                        if s:
                            k += rr; assert k <= se, "run beyond the band"
                            blk[k] = _extend(r.bits(s), s) * (1 << al); k += 1
                        elif rr == 15:
                            sc["zrl"].append((u, k, k + 16)); k += 16
                        else:
                            eobrun = (1 << rr) + r.bits(rr)
                            sc["eobruns"].append((u, eobrun))
                            if k > ss:
                                sc["eob_after_coefs"] += 1
                            eobrun -= 1
                            break
                elif ss > 0:                                           # AC refinement (G.1.2.3)
                    k = ss; lut = ac_lut[0]
                    if not eobrun:
                        while k <= se:
                            rs = huff(r, lut); rr, s = rs >> 4, rs & 15
                            newv = 0
                            if s:
                                assert s == 1
                                newv = p1 if r.bits(1) else m1
                            elif rr != 15:
                                eobrun = (1 << rr) + r.bits(rr)
                                sc["eobruns"].append((u, eobrun))
                                if k > ss:
                                    sc["eob_after_coefs"] += 1
                                break
                            k0 = k
                            nb = 0
                            while k <= se:
                                v = int(blk[k])
                                if v:
                                    nb += 1
                                    if r.bits(1) and not (v & p1):
                                        blk[k] = v + (p1 if v >= 0 else m1)
                                else:
                                    rr -= 1
                                    if rr < 0:
                                        break
                                k += 1
                            sc["stretches"].append((nb, "sym" if s else "zrl", u))
                            if not s:
                                sc["zrl"].append((u, k0, k + 1))
                            if newv:
                                assert k <= se, "new coefficient beyond the band"
                                blk[k] = newv
                            k += 1
                    if eobrun:
                        nb = 0
                        while k <= se:
                            v = int(blk[k])
                            if v:
                                nb += 1
                                if r.bits(1) and not (v & p1):
                                    blk[k] = v + (p1 if v >= 0 else m1)
                            k += 1
                        if nb:
                            sc["stretches"].append((nb, "tail", u))
                        eobrun -= 1
            u += 1
        if r.pos > r.len:
            sc["overrun"] += 1
    sc["max_code"] = max((l for l in range(17) if lens[l]), default=0)


# ------------------------------------------------------------------------------------------- the decoder that goes on after damage
def _split_intervals_lenient(f, start):
    """Entropy-coded data from `start`, whatever it holds: [(file offset, bytes with the stuffing removed, end offset)] per
    restart interval and the offset where the scan ends (a marker that is neither RSTn nor stuffing, or the end of the file).
    FF 00 is the data byte FF (B.1.1.5).  Fill bytes precede MARKERS (B.1.1.2): the FF bytes in front of an RSTn or of the
    marker that ends the scan belong to neither interval; FF bytes in front of FF 00, or at the very end of a cut file, precede
    no marker and are data."""
    ivs = []; cur = bytearray(); s0 = q = start; n = len(f)
    while q < n:
        if f[q] != 0xFF:
            cur.append(f[q]); q += 1; continue
        e = q
        while e < n and f[e] == 0xFF:
            e += 1
        nx = f[e] if e < n else None
        if nx is None:
            cur += b"\xFF" * (e - q); q = e
        elif nx == 0:
            cur += b"\xFF" * (e - q); q = e + 1
        elif 0xD0 <= nx <= 0xD7:
            ivs.append((s0, bytes(cur), q)); cur = bytearray(); q = e + 1; s0 = q
        else:
            ivs.append((s0, bytes(cur), q)); return ivs, e - 1
    ivs.append((s0, bytes(cur), q))
    return ivs, q


class _Stop(Exception):
    pass


def _book(table):
    """(code lengths in use, {(length, code): symbol}) (Annex C): a damaged file is small and brings tables of its own, a dictionary
    costs less to build than the 16-bit look-ahead table of the strict mode."""
    codes = {(ln, code): sym for sym, (code, ln) in _codes(table).items()}
    return sorted({ln for ln, _c in codes}), codes


def _w16(v):
    return ((int(v) + 0x8000) & 0xFFFF) - 0x8000


def _decode_scan_lenient(D, sc, ivs, dht, variant=None):
    """One progressive scan of a file that may be damaged.  The rules (T.81 Annex G, and for what G leaves open the contract of
    DESIGN.md 4.5):
    * the unit of failure is the (scan, restart interval) pair.  Inside an interval decoding STOPS at a code that matches nothing
      (16 bits are consumed), a DC category above 15, an AC-first symbol whose run carries k past Se, a refinement symbol with
      s not in {0, 1}.  What was stored before the stop stays -- in a refinement block the corrections of the earlier symbols of
      that block too --, the units behind it keep what earlier scans left, the other intervals and scans go on;
    * past the end of an interval's bytes the reader delivers zero bits and decoding goes on; the interval OVERRAN when it
      consumed one of them.  An end-of-band run that outlasts its interval is dropped;
    * accepted: DC categories 12..15; a ZRL that leaves the band (the block ends); a refinement (run, 1) that finds fewer than
      run + 1 zero-history positions (its correction bits are spent, the new value is dropped);
    * every store wraps to int16: pred * (1 << Al), extend(bits(s), s) * (1 << Al); a correction bit leaves a coefficient alone
      when its bit Al is already set;
    * fewer intervals than the scan needs: the missing units are untouched, the file is flagged; surplus intervals are ignored
      and not flagged.
    The file is flagged when an interval stopped or overran or a scan lacks intervals."""
    frame, coefs = D.frame, D.coefs
    ss, se, ah, al, comps = sc["ss"], sc["se"], sc["ah"], sc["al"], sc["comps"]
    inter = len(comps) > 1
    if inter:
        units = frame.mcu_x * frame.mcu_y
    else:
        nby, nbx = frame.coded(comps[0]); units = nby * nbx
    ri = sc["dri"] or units
    want = _cdiv(units, ri)
    sc.update(units=units, want=want, stops=[], overran=[], irregular=[], missing=max(0, want - len(ivs)), surplus=max(0, len(ivs) - want))
    if sc["missing"] and variant != "no_flag_missing":
        D.flagged = True
    if sc["surplus"] and variant == "flag_surplus":
        D.flagged = True
    dc_lut = [_book(dht[(0, i)]) if (ss == 0 and ah == 0) else None for i in sc["dc_ids"]]
    ac_lut = _book(dht[(1, sc["ac_ids"][0])]) if se > 0 else None
    p1, m1 = 1 << al, -(1 << al)
    dc_max = 11 if variant == "refuse_dc12" else 15

    at = [0, 0]                                                        # interval and unit being decoded

    def over(r, what):
        if r.pos > r.len and not (sc["overran"] and sc["overran"][-1][0] == at[0]):
            sc["overran"].append((at[0], at[1], what)); D.flagged = True

    def huff(r, book):
        p = r.peek16()
        for ln in book[0]:
            sym = book[1].get((ln, p >> (16 - ln)))
            if sym is not None:
                r.pos += ln; over(r, "code")
                return sym
        r.pos += 16; over(r, "code")
        raise _Stop("no_code")

    def take(r, n, what):
        v = r.bits(n); over(r, what)
        return v

    def unit_blocks(u):
        if inter:
            my, mx = divmod(u, frame.mcu_x)
            for slot, c in enumerate(comps):
                h, v = frame.hv[c]
                for y in range(v):
                    for x in range(h):
                        yield slot, coefs[c][my * v + y, mx * h + x]
        else:
            yield 0, coefs[comps[0]][u // nbx, u % nbx]

    def correct(r, blk, k, iv, u):
        v = int(blk[k])
        if take(r, 1, "correction"):
            if v & p1:
                sc["irregular"].append((iv, u, "bit_set"))
            else:
                blk[k] = _w16(v + (p1 if v >= 0 else m1))

    eobrun = 0
    for iv in range(min(want, len(ivs))):
        data = ivs[iv]
        r = _Reader(data) if len(data) < 512 else _Chunked(data)
        u0, u1 = iv * ri, min(units, iv * ri + ri)
        pred = [0] * len(comps)
        if variant != "carry_eobrun":
            eobrun = 0
        u = u0; entry = None
        try:
            while u < u1:
                at[0], at[1] = iv, u
                if ss > 0 and eobrun and ah == 0:                      # AC first: the blocks of an end-of-band run are not coded
                    hop = min(eobrun, u1 - u); eobrun -= hop; u += hop
                    continue
                for slot, blk in unit_blocks(u):
                    entry = (blk, blk.copy())
                    if ss == 0 and ah == 0:                            # DC first (G.1.2.1)
                        s = huff(r, dc_lut[slot])
                        if s > dc_max:
                            raise _Stop("dc_category")
                        if s > 11:
                            sc["irregular"].append((iv, u, "dc_wide"))
                        pred[slot] += _extend(take(r, s, "value"), s) if s else 0
                        blk[0] = _w16(pred[slot] * (1 << al))
                    elif ss == 0:                                      # DC refinement
                        if take(r, 1, "dc_bit"):
                            blk[0] = _w16(int(blk[0]) | p1)
                    elif ah == 0:                                      # AC first (G.1.2.2)
                        k = ss
                        while k <= se:
                            rs = huff(r, ac_lut); rr, s = rs >> 4, rs & 15
                            if s:
                                k += rr
                                if k > se:
                                    raise _Stop("run_past_se")
                                blk[k] = _w16(_extend(take(r, s, "value"), s) * (1 << al)); k += 1
                            elif rr == 15:
                                if k + 16 > se + 1:
                                    sc["irregular"].append((iv, u, "zrl_out"))
                                k += 16
                            else:
                                eobrun = (1 << rr) + take(r, rr, "eob_length") - 1
                                break
                    else:                                              # AC refinement (G.1.2.3)
                        k = ss
                        if eobrun and not blk[ss:se + 1].any():        # inside a run, nothing to correct
                            eobrun -= 1
                            continue
                        if not eobrun:
                            while k <= se:
                                rs = huff(r, ac_lut); rr, s = rs >> 4, rs & 15
                                newv = 0
                                if s:
                                    if s != 1:
                                        raise _Stop("refine_s")
                                    newv = p1 if take(r, 1, "sign") else m1
                                elif rr != 15:
                                    eobrun = (1 << rr) + take(r, rr, "eob_length")
                                    break
                                while k <= se:                         # pass rr zero-history positions, correct the others on the way
                                    if blk[k]:
                                        correct(r, blk, k, iv, u)
                                    else:
                                        rr -= 1
                                        if rr < 0:
                                            break
                                    k += 1
                                if k > se:
                                    sc["irregular"].append((iv, u, "run_out" if s else "zrl_out"))
                                elif newv:
                                    blk[k] = newv
                                k += 1
                        if eobrun:
                            while k <= se:
                                if blk[k]:
                                    correct(r, blk, k, iv, u)
                                k += 1
                            eobrun -= 1
                u += 1
            if eobrun:
                sc["irregular"].append((iv, u1 - 1, "eobrun_cut"))
        except _Stop as e:
            sc["stops"].append((iv, u, e.args[0])); D.flagged = True
            if variant == "discard_block":
                entry[0][...] = entry[1]
            if variant == "stop_scan":
                break


# ------------------------------------------------------------------------------------------- what the decoder leaves behind
def arena(frame, coefs, clear_dc=True):
    """The coefficient arena of jpegsnoop_amd for these coefficients: one row of 64 per block in MCU decode order, NATURAL
    order inside the row, dequantised in wrapping int16 arithmetic ((int16)(coef * Q)).  Slot 0: zero (what the progressive
    finalize pass leaves: the DC goes to a separate array) or, with clear_dc=False, the dequantised DC itself."""
    rows = []
    nat = np.array(ZIGZAG)
    for c, y, x in frame.mcu_blocks():
        h, v = frame.hv[c]
        q = np.array(frame.qtabs[frame.comps[c][2]], np.int64)
        blk = coefs[c][y::v, x::h].astype(np.int64) * q                          # [mcu_y, mcu_x, 64] zig-zag
        out = np.zeros_like(blk); out[..., nat] = blk
        rows.append(out)
    a = np.stack(rows, 2).reshape(-1, 64)                                        # [mcu_y, mcu_x, blocks per MCU, 64]
    a = (a & 0xFFFF).astype(np.uint16).view(np.int16).copy()
    if clear_dc:
        a[:, 0] = 0
    return a


def baseline_dc_diffs(frame, coefs):
    """Per arena row: the DC difference the sequential coder writes for that block (predictor per component, MCU order)."""
    blocks = frame.mcu_blocks(); out = np.zeros(frame.mcu_x * frame.mcu_y * len(blocks), np.int64); pred = [0] * frame.ncomp; i = 0
    for my in range(frame.mcu_y):
        for mx in range(frame.mcu_x):
            for c, y, x in blocks:
                h, v = frame.hv[c]; d = int(coefs[c][my * v + y, mx * h + x, 0])
                out[i] = d - pred[c]; pred[c] = d; i += 1
    return out
