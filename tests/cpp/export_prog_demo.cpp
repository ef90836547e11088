// The progressive export through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CJPEGsnoopCoreGpu::BatchExportJpegProgressive(files, bJfif, nMode, nInterval)
// with the built-in script over every listed file, entry k read back and written to <out dir>/out<k>.jpg, and one line per entry -- "<k>" and per scan
// " <comps>:<Ri>:<Ss>:<SOS offset>" from BatchExportScanInfo; then the first file once more through the single-image class, CimgDecodeGpu::ExportJpegProgressive,
// to <out dir>/single.jpg -- for tests/test_gpu_export_prog.py.  usage: export_prog_demo outdir mode interval file...; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 5) { printf("usage: export_prog_demo outdir mode interval file...\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    const int mode = atoi(argv[2]); const unsigned interval = (unsigned)atoi(argv[3]);
    CJPEGsnoopCoreGpu core;
    std::vector<uint8_t> first;
    for (int a = 4; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb"); if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        if (a == 4) first = buf;
        if (core.BatchAddFile(buf.data(), buf.size()) < 0) { printf("refused %s: %s\n", argv[a], jsnoop_last_error()); return 2; }
    }
    if (!core.DoBatchProcess()) { printf("decode failed: %s\n", jsnoop_last_error()); return 2; }
    if (!core.BatchExportJpegProgressive({}, true, mode, interval)) { printf("BatchExportJpegProgressive failed: %s\n", jsnoop_last_error()); return 2; }
    for (int k = 0; k < core.BatchExportCount(); k++) {
        std::vector<uint8_t> file;
        if (!core.BatchReadExport(k, file)) { printf("BatchReadExport failed: %s\n", jsnoop_last_error()); return 2; }
        const std::string path = std::string(argv[1]) + "/out" + std::to_string(k) + ".jpg";
        FILE* f = fopen(path.c_str(), "wb"); if (!f) { printf("cannot write %s\n", path.c_str()); return 2; }
        const bool ok = fwrite(file.data(), 1, file.size(), f) == file.size(); fclose(f);
        if (!ok) return 2;
        printf("%d", k);
        for (int s = 0; s < core.BatchExportScanCount(k); s++) {
            JsnoopExportScan sc; uint32_t ri = 0; uint64_t ni = 0, sos = 0, nb = 0;
            if (!core.BatchExportScanInfo(k, s, sc, ri, ni, sos, nb)) { printf("BatchExportScanInfo failed: %s\n", jsnoop_last_error()); return 2; }
            printf(" %u:%u:%u:%llu", (unsigned)sc.comps, ri, (unsigned)sc.ss, (unsigned long long)sos);
        }
        printf("\n");
    }
    CwindowBufView view; view.pData = first.data(); view.nLen = first.size();
    CimgDecodeGpu dec(nullptr, &view);
    unsigned nStart = 0;
    if (!dec.WalkJfifHeader(nStart)) { printf("WalkJfifHeader failed: %s\n", jsnoop_last_error()); return 2; }
    dec.DecodeScanImg(nStart, true, false);
    if (!dec.ExportJpegProgressive(std::string(argv[1]) + "/single.jpg", mode, interval)) { printf("ExportJpegProgressive failed: %s\n", jsnoop_last_error()); return 2; }
    return 0;
}
