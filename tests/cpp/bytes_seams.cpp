// js_next_ff / js_scan_end (jpegsnoop_amd/csrc/jsnoop_bytes.h) against a byte-at-a-time restatement of what their comments promise, at the seams
// of their sixteen-byte steps: buffers of 0..80 bytes, start offsets 0..17, a run of FF at every position followed by each of 00, D0, D7, CF, D8,
// D9, FF and by the end of the buffer (len 0, 1 and 2 among them).  Every buffer is followed by guard bytes that would change the answer if they
// were looked at.  Built twice by tests/test_bytes_seams.py: as is, and with -U__SSE2__ (the byte loops alone).
// Prints "sse2=<0|1> cases=<n> mismatches=<m>"; exit status 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "jsnoop_bytes.h"

static size_t plain_next_ff(const uint8_t* f, size_t q, size_t n)
{
    for (; q < n; q++) if (f[q] == 0xFF) return q;
    return q;
}
static uint32_t plain_scan_end(const uint8_t* f, uint32_t q, size_t len)
{
    for (; (size_t)q + 1 < len; q++) {
        const uint8_t a = f[q], b = f[q + 1];
        if (a != 0xFF) continue;
        if (b == 0x00) continue;                                  // a stuffed FF
        if (b >= 0xD0 && b <= 0xD7) continue;                     // RSTn
        return q;                                                 // any other marker (FF FF included) ends the entropy-coded data
    }
    return (uint32_t)len;                                         // the last byte has no successor inside the buffer: never a marker
}

static unsigned long long g_cases = 0, g_bad = 0;

static void check(const uint8_t* f, size_t len, const char* what)
{
    for (uint32_t q = 0; q <= 17; q++) {
        const size_t a = js_next_ff(f, q, len), b = plain_next_ff(f, q, len);
        const uint32_t c = js_scan_end(f, q, len), d = plain_scan_end(f, q, len);
        g_cases += 2;
        if (a != b) { if (g_bad++ < 20) printf("js_next_ff  %s len=%zu q=%u: %zu, want %zu\n", what, len, q, a, b); }
        if (c != d) { if (g_bad++ < 20) printf("js_scan_end %s len=%zu q=%u: %u, want %u\n", what, len, q, c, d); }
    }
}

int main()
{
    static const uint8_t follow[7] = { 0x00, 0xD0, 0xD7, 0xCF, 0xD8, 0xD9, 0xFF };
    static const uint8_t fill_guard[3][2] = { { 0x11, 0x00 }, { 0x00, 0xFF }, { 0xD0, 0xD9 } };
    static const unsigned runs[8] = { 1, 2, 3, 15, 16, 17, 18, 33 };
    const size_t GUARD = 48;
    std::vector<uint8_t> arena(80 + GUARD);
    char what[96];
    for (size_t len = 0; len <= 80; len++)
        for (int fg = 0; fg < 3; fg++) {
            uint8_t* f = arena.data();
            auto reset = [&] { memset(f, fill_guard[fg][0], len); memset(f + len, fill_guard[fg][1], GUARD); };
            reset();
            check(f, len, "no FF");
            for (size_t p = 0; p < len; p++)
                for (unsigned r : runs) {
                    if (p + r > len) continue;
                    if (p + r == len) {                                        // the run ends the buffer
                        reset(); memset(f + p, 0xFF, r);
                        snprintf(what, sizeof what, "fill=%02x guard=%02x FFx%u at %zu, end", fill_guard[fg][0], fill_guard[fg][1], r, p);
                        check(f, len, what);
                        continue;
                    }
                    for (uint8_t x : follow) {
                        reset(); memset(f + p, 0xFF, r); f[p + r] = x;
                        snprintf(what, sizeof what, "fill=%02x guard=%02x FFx%u at %zu, then %02x", fill_guard[fg][0], fill_guard[fg][1], r, p, x);
                        check(f, len, what);
                    }
                }
        }
    // dense random mixtures of the bytes the rules look at
    static const uint8_t alphabet[8] = { 0xFF, 0xFF, 0x00, 0xD0, 0xD7, 0xD9, 0x11, 0xCF };
    uint32_t lcg = 12345u;
    for (int it = 0; it < 20000; it++) {
        lcg = lcg * 1664525u + 1013904223u;
        const size_t len = (lcg >> 8) % 81;
        uint8_t* f = arena.data();
        for (size_t i = 0; i < len + GUARD; i++) { lcg = lcg * 1664525u + 1013904223u; f[i] = alphabet[(lcg >> 13) & 7]; }
        snprintf(what, sizeof what, "random %d", it);
        check(f, len, what);
    }
#if defined(__SSE2__)
    const int sse2 = 1;
#else
    const int sse2 = 0;
#endif
    printf("sse2=%d cases=%llu mismatches=%llu\n", sse2, g_cases, g_bad);
    return g_bad ? 1 : 0;
}
