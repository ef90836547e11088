// carve_demo.cpp -- "extract all" through the C++ wrapper (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CarveBlob on every listed file, one line per frame
//   frame <relative path> k=<n> start=<n> end=<n> status=<n> parent=<n> size=<w>x<h>
// then DoBatchFileProcessAll(bExtractAll = true) (one report per carved frame under dirDst) and the same list through JobRun(bExtractAll = true), where
// every decoded frame's DIB goes to <dirDst>/<job index>.dib and gets a line
//   file <job index> from=<relative path> k=<frame number> status=<n> kind=<n> size=<x>x<y>
//   carve_demo dirSrc dirDst
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: carve_demo dirSrc dirDst\n"); return 2; }
    try {
        CJPEGsnoopCoreGpu core;
        const unsigned n = core.GenBatchFileList(argv[1], true);
        printf("listed %u\n", n);
        for (unsigned i = 0; i < n; i++) {
            std::vector<uint8_t> blob; std::vector<JsnoopCarveFrame> frames;
            if (FILE* fp = fopen(core.GetBatchFileInfo(i).c_str(), "rb")) { uint8_t tmp[4096]; size_t m; while ((m = fread(tmp, 1, sizeof tmp, fp)) > 0) blob.insert(blob.end(), tmp, tmp + m); fclose(fp); }
            if (!CJPEGsnoopCoreGpu::CarveBlob(blob.data(), blob.size(), frames)) { printf("carve_failed %s\n", jsnoop_last_error()); return 1; }
            for (size_t k = 0; k < frames.size(); k++)
                printf("frame %s k=%zu start=%u end=%u status=%d parent=%d size=%ux%u\n", core.GetBatchFileEntry(i)->strRel.c_str(), k + 1, frames[k].start, frames[k].end,
                       frames[k].status, frames[k].parent, frames[k].width, frames[k].height);
        }
        const std::vector<int> devices(1, 0);
        JsnoopJobStats st; st.struct_size = sizeof st;
        const int nok = core.DoBatchFileProcessAll(true, argv[2], devices, &st, true);
        if (nok < 0) { printf("job_failed %s\n", jsnoop_last_error()); return 1; }
        printf("processed ok=%d files=%d refused=%d unreadable=%d\n", nok, st.files, st.refused, st.unreadable);
        bool wrote = true;
        const int rc = core.JobRun([&](const JsnoopJobFile& f) {
            const CJPEGsnoopCoreGpu::CarvedInfo* ci = core.GetCarvedEntry((unsigned)f.index);
            printf("file %d from=%s k=%u status=%d kind=%d size=%ux%u\n", f.index, ci ? core.GetBatchFileEntry(ci->nFileInd)->strRel.c_str() : "?", ci ? ci->nFrame : 0u, f.status, f.kind,
                   f.info16[2], f.info16[3]);
            if (f.status != JSNOOP_JOB_OK) return true;
            std::vector<uint8_t> dib((size_t)f.info16[2] * f.info16[3] * 4u);
            if (jsnoop_batch_read_dib(f.batch, f.image, dib.data())) { wrote = false; return true; }
            const std::string name = std::string(argv[2]) + "/" + std::to_string(f.index) + ".dib";
            FILE* fp = fopen(name.c_str(), "wb");
            if (!fp || fwrite(dib.data(), 1, dib.size(), fp) != dib.size()) wrote = false;
            if (fp) fclose(fp);
            return true;
        }, devices, nullptr, true);
        printf("jobrun rc=%d wrote=%d\n", rc, wrote ? 1 : 0);
        return rc == 0 && wrote ? 0 : 1;
    } catch (const std::exception& e) {
        printf("no_gpu %s\n", e.what());
        return 3;
    }
}
