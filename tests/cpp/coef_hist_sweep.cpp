// Host-only program: the binning of jsnoop_batch_pack_coef_hist (jpegsnoop_amd/csrc/jsnoop_coef_bin.h, the text k_coef_hist compiles for the device) swept
// exhaustively.  Every int16 value v against every divisor q = 1 .. 65535 must give C's v / q through the reciprocal; q = 0 counts as 1; every quotient in
// -32768 .. 32767 against every range R = 1 .. 127 must land in clamp(x, -R, R) + R; the small division that finds a block inside its MCU must be exact for
// every sum the kernel can meet; the row length must be 64 (2 R + 1) + 128.  tests/test_coef_hist_abi.py builds it -O2 and runs it.  Prints "ok" and
// returns 0, or the first value that failed.
#include <cstdio>
#include <cstdint>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include "../../jpegsnoop_amd/csrc/jsnoop_coef_bin.h"

// divisors q0 .. q1 - 1; *bad = the first (v, q) that failed, if any
static void sweep_div(uint32_t q0, uint32_t q1, std::atomic<uint64_t>* bad)
{
    for (uint32_t q = q0; q < q1; q++) {
        const uint32_t m = js_chist_recip(q);
        for (int32_t v = -32768; v <= 32767; v++)
            if (js_chist_div(v, m) != v / (int32_t)q) { bad->store((uint64_t)q << 32 | (uint32_t)v); return; }
    }
}

int main()
{
    {
        const uint32_t nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        std::atomic<uint64_t> bad(0);
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < nt; t++) th.emplace_back(sweep_div, 1u + (uint32_t)(65535ull * t / nt), 1u + (uint32_t)(65535ull * (t + 1) / nt), &bad);
        for (auto& x : th) x.join();
        if (bad.load()) {
            const int32_t v = (int32_t)(uint32_t)bad.load(); const uint32_t q = (uint32_t)(bad.load() >> 32);
            printf("FAILED: %d / %u = %d, the reciprocal %u gives %d\n", v, q, v / (int32_t)q, js_chist_recip(q), js_chist_div(v, js_chist_recip(q))); return 1;
        }
    }
    if (js_chist_recip(0) != js_chist_recip(1)) { printf("FAILED: a divisor of 0 must count as 1\n"); return 1; }
    for (int32_t r = 1; r <= 127; r++) {
        if (js_chist_words((uint32_t)r) != 64u * (2u * (uint32_t)r + 1u) + 128u) { printf("FAILED: row length for R = %d\n", r); return 1; }
        for (int32_t x = -32768; x <= 32767; x++) {
            const int32_t c = x < -r ? -r : (x > r ? r : x);
            const uint32_t got = js_chist_bin(x, r);
            if (got != (uint32_t)(c + r) || got > 2u * (uint32_t)r) { printf("FAILED: bin of %d under R = %d is %u\n", x, r, got); return 1; }
        }
    }
    for (uint32_t hv = 1; hv <= 16; hv++)
        for (uint32_t t = 0; t < 96; t++)
            if (js_chist_small_div(t, 65536u / hv + 1u) != t / hv) { printf("FAILED: %u / %u\n", t, hv); return 1; }
    printf("ok\n");
    return 0;
}
