// job_demo.cpp -- a folder through the whole-node batch loop of the C++ wrapper (jpegsnoop_amd/csrc/ImgDecodeGpu.h):
// GenBatchFileList -> DoBatchFileProcessAll (one report per file under dirDst), then the same list through JobRun, one
// line per file for the Python test:  file <relative path> status=<n> kind=<n> hash=<16 hex digits> size=<x>x<y>.
//   job_demo dirSrc dirDst [shards]        (shards: logical shards on device 0, default 2)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: job_demo dirSrc dirDst [shards]\n"); return 2; }
    const int shards = argc > 3 ? atoi(argv[3]) : 2;
    try {
        CJPEGsnoopCoreGpu core;
        const unsigned n = core.GenBatchFileList(argv[1], true);
        printf("listed %u first=%s\n", n, n ? core.GetBatchFileEntry(0)->strRel.c_str() : "");
        const std::vector<int> devices((size_t)(shards > 0 ? shards : 1), 0);
        JsnoopJobStats st; st.struct_size = sizeof st;
        const int nok = core.DoBatchFileProcessAll(true, argv[2], devices, &st);
        if (nok < 0) { printf("job_failed %s\n", jsnoop_last_error()); return 1; }
        printf("processed ok=%d files=%d refused=%d unreadable=%d shards=%d\n", nok, st.files, st.refused, st.unreadable, st.nshards);
        const int rc = core.JobRun([&](const JsnoopJobFile& f) {
            printf("file %s status=%d kind=%d hash=%016llx size=%ux%u\n", core.GetBatchFileEntry((unsigned)f.index)->strRel.c_str(), f.status, f.kind,
                   (unsigned long long)f.dib_hash, f.info16[2], f.info16[3]);
            return true;
        }, devices);
        printf("jobrun rc=%d\n", rc);
        return rc == 0 ? 0 : 1;
    } catch (const std::exception& e) {
        printf("no_gpu %s\n", e.what());
        return 3;
    }
}
