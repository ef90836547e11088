// The export with optimal Huffman tables through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CJPEGsnoopCoreGpu::BatchExportJpeg(files, bJfif,
// bOptimal = true) over every listed file, entry k read back and written to <out dir>/out<k>.jpg, and one line per entry -- "<k> <symbols of the table of
// slot 0> <slot 1> [<slot 2> <slot 3>]" from BatchExportTables -- for tests/test_gpu_export_opt.py.  usage: export_opt_demo outdir file...; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 3) { printf("usage: export_opt_demo outdir file...\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    CJPEGsnoopCoreGpu core;
    for (int a = 2; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb"); if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        if (core.BatchAddFile(buf.data(), buf.size()) < 0) { printf("refused %s: %s\n", argv[a], jsnoop_last_error()); return 2; }
    }
    if (!core.DoBatchProcess()) { printf("decode failed: %s\n", jsnoop_last_error()); return 2; }
    if (!core.BatchExportJpeg({}, true, true)) { printf("BatchExportJpeg failed: %s\n", jsnoop_last_error()); return 2; }
    for (int k = 0; k < core.BatchExportCount(); k++) {
        std::vector<uint8_t> file;
        if (!core.BatchReadExport(k, file)) { printf("BatchReadExport failed: %s\n", jsnoop_last_error()); return 2; }
        const std::string path = std::string(argv[1]) + "/out" + std::to_string(k) + ".jpg";
        FILE* f = fopen(path.c_str(), "wb"); if (!f) { printf("cannot write %s\n", path.c_str()); return 2; }
        const bool ok = fwrite(file.data(), 1, file.size(), f) == file.size(); fclose(f);
        if (!ok) return 2;
        printf("%d", k);
        uint8_t counts[16], symbols[256]; uint32_t nsym = 0, freq[256];
        for (int slot = 0; slot < 4 && core.BatchExportTables(k, slot, counts, symbols, nsym, freq); slot++) printf(" %u", nsym);
        printf("\n");
    }
    return 0;
}
