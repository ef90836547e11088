// Host-only program: the host side of jsnoop_carve_run (jpegsnoop_amd/csrc/jsnoop_carve_check.h) without a device -- spec import, every refusal with its text,
// the sizes of lists and scratch (the all-FF blob: 4 n bytes of terminators), the budget check, the walk on hand-made blobs, records <-> frames, the parent pass on
// hand-made tables and the choice of frames a job takes.  tests/test_carve_abi.py builds it with the address and undefined-behaviour sanitizers and runs it.
// "table <hex>" prints the frames of a blob, one line each, for the comparison with tests/carve_model.py.  Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/jsnoop_carve_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)
static bool said(const char* what) { return g_err.find(what) != std::string::npos; }

static JsCarveRec rec(uint32_t start, uint32_t end, uint32_t status) { JsCarveRec r; memset(&r, 0, sizeof r); r.w[0] = start; r.w[1] = end; r.w[2] = status; return r; }

int main(int argc, char** argv)
{
    if (argc > 2 && !strcmp(argv[1], "table")) {               // "table <hex> [max_markers]"
        std::vector<uint8_t> b; const char* h = argv[2];
        for (size_t k = 0; h[k] && h[k + 1]; k += 2) { unsigned v; sscanf(h + k, "%2x", &v); b.push_back((uint8_t)v); }
        std::vector<uint32_t> term, cand; std::vector<JsCarveRec> recs; std::vector<int32_t> parent;
        js_carve_host_table(b.data(), b.size(), argc > 3 ? (uint32_t)atoi(argv[3]) : JS_CARVE_MAX_MARKERS, &term, &cand, &recs);
        js_carve_parents(recs.data(), recs.size(), &parent);
        for (size_t k = 0; k < recs.size(); k++) {
            JsnoopCarveFrame f; js_carve_frame_of(recs[k], parent[k], &f);
            printf("%u %u %d %d %u %u %u %u %u %u %u %u %u %u %u %u %d\n", f.start, f.end, f.status, f.reason, f.detail_pos, f.detail_byte, f.seen, f.sof_code, f.precision, f.width, f.height,
                   f.components, f.sos_pos, f.scan_start, f.scans, f.markers, f.parent);
        }
        printf("T"); for (uint32_t t : term) printf(" %u", t);
        printf("\n");
        return 0;
    }
    CHECK(sizeof(JsnoopCarveSpec) == 16 && sizeof(JsnoopCarveFrame) == 72 && sizeof(JsCarveRec) == 64);

    // spec: defaults, shorter accepted, longer and NULL refused, max_markers 0 = the default
    JsnoopCarveSpec def; memset(&def, 0xEE, sizeof def); js_carve_spec_defaults(&def);
    CHECK(def.struct_size == 16 && def.max_markers == 4096 && def.max_scratch_bytes == 0);
    JsnoopCarveSpec in = def, s;
    in.max_markers = 7; in.max_scratch_bytes = 1234; CHECK(js_carve_import_spec(&in, &s) == 0 && s.max_markers == 7 && s.max_scratch_bytes == 1234);
    in.struct_size = 8; CHECK(js_carve_import_spec(&in, &s) == 0 && s.max_markers == 7 && s.max_scratch_bytes == 0 && s.struct_size == 16);
    in.struct_size = 4; CHECK(js_carve_import_spec(&in, &s) == 0 && s.max_markers == 4096);
    in.struct_size = 16; in.max_markers = 0; CHECK(js_carve_import_spec(&in, &s) == 0 && s.max_markers == 4096);
    in.struct_size = 24; CHECK(js_carve_import_spec(&in, &s) == -1 && said("struct_size 24"));
    in.struct_size = 0; CHECK(js_carve_import_spec(&in, &s) == -1);
    CHECK(js_carve_import_spec(nullptr, &s) == -1 && said("spec is NULL"));

    // the blob
    const uint8_t one[1] = { 0xFF };
    CHECK(js_carve_check_blob(nullptr, 0, 0) == 0 && js_carve_check_blob(one, 1, 1) == 0);
    CHECK(js_carve_check_blob(nullptr, 1, 0) == -1 && said("blob is NULL"));
    CHECK(js_carve_check_blob(one, 1ull << 32, 0) == -1 && said("positions are 32 bits"));
    CHECK(js_carve_check_blob(one, (1ull << 32) - 1, 1) == 0);
    CHECK(js_carve_check_blob(one, 1, 2) == -1 && said("where = 2"));

    // sizes: tiles count from the 16-byte boundary below the blob; the all-FF blob has n - 1 terminators and needs 4 bytes for each
    CHECK(js_carve_tiles(0, 7) == 0 && js_carve_tiles(1, 0) == 1 && js_carve_tiles(JS_CARVE_TILE, 0) == 1 && js_carve_tiles(JS_CARVE_TILE, 1) == 2 && js_carve_tiles(JS_CARVE_TILE - 15, 15) == 1);
    CHECK(js_carve_tiles((1ull << 32) - 1, 15) == (1ull << 32) / JS_CARVE_TILE + 1);
    {
        std::vector<uint8_t> ff(4096, 0xFF); std::vector<uint32_t> term, cand; std::vector<JsCarveRec> recs;
        js_carve_host_table(ff.data(), ff.size(), 4096, &term, &cand, &recs);
        CHECK(term.size() == 4095 && cand.empty() && recs.empty() && term[0] == 0 && term[4094] == 4094);
        const JsCarveSizes z = js_carve_sizes(4096, 0, term.size(), 0, 1);
        CHECK(z.term_list == 4u * 4095u && z.cand_list == 0 && z.recs == 0 && z.copy == 0 && z.counts == 32 && z.total == 4u * 4095u + 32u);
        CHECK(js_carve_sizes(4096, 0, term.size(), 0, 0).total == z.total + 4096);
        CHECK(js_carve_check_budget(z, z.total) == 0);
        CHECK(js_carve_check_budget(z, z.total - 1) == -1 && said("exceed max_scratch_bytes 16411") && said("lists 16380"));
        const JsCarveSizes big = js_carve_sizes((1ull << 32) - 1, 0, (1ull << 32) - 2, (1ull << 31) - 1, 1);      // no 32-bit overflow anywhere
        CHECK(big.term_list == 4ull * ((1ull << 32) - 2) && big.recs == 64ull * ((1ull << 31) - 1) && big.total > (1ull << 37));
    }

    // the walk on hand-made blobs (tests/carve_model.py has the whole catalogue; here: the shapes of the record)
    {
        const uint8_t b[] = { 0x11, 0xFF, 0xD8, 0xFF, 0xC0, 0x00, 0x0B, 0x08, 0x01, 0x02, 0x03, 0x04, 0x03, 0, 0, 0, 0xFF, 0xDA, 0x00, 0x02, 0x55, 0xFF, 0x00, 0xFF, 0xD9, 0x22 };
        std::vector<uint32_t> term, cand; std::vector<JsCarveRec> recs;
        js_carve_host_table(b, sizeof b, 4096, &term, &cand, &recs);
        CHECK(cand.size() == 1 && cand[0] == 1 && recs.size() == 1);
        CHECK(term == (std::vector<uint32_t>{ 1, 3, 16, 23 }));
        JsnoopCarveFrame f; js_carve_frame_of(recs[0], -1, &f);
        CHECK(f.struct_size == 72 && f.start == 1 && f.end == 25 && f.status == JSNOOP_CARVE_OK && f.reason == 0 && f.detail_pos == 0 && f.seen == 0);
        CHECK(f.sof_code == 0xC0 && f.precision == 8 && f.height == 0x0102 && f.width == 0x0304 && f.components == 3 && f.sos_pos == 16 && f.scan_start == 20 && f.scans == 1 && f.markers == 4);
        for (uint32_t k = 10; k < JS_CARVE_REC_WORDS; k++) CHECK(recs[0].w[k] == 0);
        js_carve_host_table(b, sizeof b, 3, &term, &cand, &recs);                    // the fourth marker is over the cap
        js_carve_frame_of(recs[0], -1, &f);
        CHECK(f.status == JSNOOP_CARVE_LIMIT && f.markers == 4 && f.detail_pos == 24 && f.detail_byte == 0xD9 && f.end == 24);
        js_carve_host_table(b, sizeof b - 3, 4096, &term, &cand, &recs);             // cut behind the stuffed FF 00: the scan has no terminator
        js_carve_frame_of(recs[0], -1, &f);
        CHECK(f.status == JSNOOP_CARVE_NO_EOI && f.end == sizeof b - 3 && f.scans == 1);
        js_carve_host_table(b, 0, 4096, &term, &cand, &recs);
        CHECK(term.empty() && cand.empty() && recs.empty());
    }

    // the guarded copy of one frame
    {
        const JsCarveRec r = rec(5, 9, JSNOOP_CARVE_NO_SOS);
        union { JsnoopCarveFrame f; uint8_t raw[sizeof(JsnoopCarveFrame)]; } u;
        memset(&u, 0xA5, sizeof u); u.f.struct_size = 0; CHECK(js_carve_export_frame(r, 3, &u.f) == 0 && u.f.struct_size == 72 && u.f.parent == 3 && u.f.start == 5 && u.f.status == JSNOOP_CARVE_NO_SOS);
        memset(&u, 0xA5, sizeof u); u.f.struct_size = 12; CHECK(js_carve_export_frame(r, 3, &u.f) == 0 && u.f.struct_size == 12 && u.f.end == 9 && u.raw[12] == 0xA5 && u.raw[71] == 0xA5);
        u.f.struct_size = 76; CHECK(js_carve_export_frame(r, 3, &u.f) == -1 && said("struct_size 76"));
        u.f.struct_size = 4; CHECK(js_carve_export_frame(r, 3, &u.f) == -1);
        CHECK(js_carve_export_frame(r, 3, nullptr) == -1 && said("out is NULL"));
    }

    // parents: the innermost earlier OK frame that holds the start
    {
        const uint32_t OK = JSNOOP_CARVE_OK, BAD = JSNOOP_CARVE_STOPPED;
        const JsCarveRec t[] = { rec(0, 100, OK), rec(5, 10, OK), rec(6, 50, OK), rec(7, 9, BAD), rec(20, 30, OK), rec(60, 70, BAD), rec(65, 200, OK), rec(99, 120, OK), rec(100, 110, OK),
                                 rec(150, 160, OK), rec(200, 210, OK), rec(205, 300, BAD), rec(206, 207, OK) };
        const int32_t want[] = { -1, 0, 1, 2, 2, 0, 0, 6, 7, 6, -1, 10, 10 };
        std::vector<int32_t> parent;
        js_carve_parents(t, sizeof t / sizeof t[0], &parent);
        for (size_t k = 0; k < parent.size(); k++) {
            int32_t slow = -1;                                    // the sentence itself: the latest-starting earlier OK frame with start <= s < end
            for (size_t j = 0; j < k; j++) if ((t[j].w[2] & 255u) == OK && t[j].w[0] <= t[k].w[0] && t[k].w[0] < t[j].w[1] && (slow < 0 || t[j].w[0] >= t[(size_t)slow].w[0])) slow = (int32_t)j;
            CHECK(parent[k] == want[k] && parent[k] == slow);
        }
        js_carve_parents(t, 0, &parent); CHECK(parent.empty());
    }

    // what a job takes
    {
        JsnoopCarveFrame fr[4]; memset(fr, 0, sizeof fr);
        fr[0].start = 0; fr[0].end = 10; fr[0].status = JSNOOP_CARVE_OK;
        fr[1].start = 2; fr[1].end = 20; fr[1].status = JSNOOP_CARVE_NO_EOI;
        fr[2].start = 4; fr[2].end = 5;  fr[2].status = JSNOOP_CARVE_STOPPED;
        fr[3].start = 12; fr[3].end = 20; fr[3].status = JSNOOP_CARVE_OK;
        std::vector<int64_t> pick;
        CHECK(js_carve_pick(fr, 4, 20, 0, &pick) == 0 && pick == (std::vector<int64_t>{ 0, 3 }));
        CHECK(js_carve_pick(fr, 4, 20, 1, &pick) == 0 && pick == (std::vector<int64_t>{ 0, 1, 3 }));
        CHECK(js_carve_pick(fr, 4, 19, 0, &pick) == -1 && said("frame 3 [12, 20) lies outside the blob of 19 bytes"));
        CHECK(js_carve_pick(fr, 3, 19, 0, &pick) == 0 && pick.size() == 1);            // the NO_EOI frame past the end is not looked at unless asked for
        CHECK(js_carve_pick(nullptr, 1, 19, 0, &pick) == -1 && js_carve_pick(fr, -1, 19, 0, &pick) == -1 && js_carve_pick(nullptr, 0, 0, 0, &pick) == 0);
    }
    printf("ok\n");
    return 0;
}
