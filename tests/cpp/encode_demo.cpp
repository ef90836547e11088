// The encoder through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CJPEGsnoopCoreGpu::EncodeJpeg over two descriptions of one picture the program
// makes itself -- pixel (x, y) = (R, G, B) = ((7 x + 3 y) & 255, (x * y + 5) & 255, (x + 2 y * y) & 255) -- once as dense interleaved R, G, B and once as
// planar B, G, R with a row pitch of width + 5: both files go to <out dir>/out0.jpg and out1.jpg -- for tests/test_gpu_encode.py, which holds them against
// the model's file of the same pixels.  usage: encode_demo outdir width height quality subsampling; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc != 6) { printf("usage: encode_demo outdir width height quality subsampling\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    const unsigned w = (unsigned)atoi(argv[2]), h = (unsigned)atoi(argv[3]);
    const size_t pitch = w + 5u, plane = pitch * h;
    std::vector<uint8_t> a((size_t)w * h * 3), b(plane * 3, 0xEE);
    for (unsigned y = 0; y < h; y++) for (unsigned x = 0; x < w; x++) {
        const uint8_t px[3] = { (uint8_t)(7 * x + 3 * y), (uint8_t)(x * y + 5), (uint8_t)(x + 2 * y * y) };
        for (int c = 0; c < 3; c++) { a[((size_t)y * w + x) * 3 + c] = px[c]; b[(size_t)(2 - c) * plane + y * pitch + x] = px[c]; }
    }
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, a.size() + b.size()) != hipSuccess || hipMemcpy(d, a.data(), a.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + a.size(), b.data(), b.size(), hipMemcpyHostToDevice) != hipSuccess) { printf("device memory: failed\n"); return 2; }
    std::vector<JsnoopEncodeSrc> src(2, JsnoopEncodeSrc{});
    src[0].ptr = d; src[0].width = w; src[0].height = h; src[0].channels = 3;
    src[1] = src[0]; src[1].ptr = d + a.size(); src[1].layout = JSNOOP_ENCODE_PLANAR; src[1].order = JSNOOP_ENCODE_BGR; src[1].row_pitch = pitch;
    JsnoopEncodeSpec spec; jsnoop_encode_spec_defaults(&spec); spec.quality = atoi(argv[4]); spec.subsampling = atoi(argv[5]);
    std::vector<std::vector<uint8_t>> files;
    if (!CJPEGsnoopCoreGpu::EncodeJpeg(src, spec, files) || files.size() != 2) { printf("EncodeJpeg failed: %s\n", jsnoop_last_error()); return 2; }
    (void)hipFree(d);
    for (size_t k = 0; k < files.size(); k++) {
        const std::string path = std::string(argv[1]) + "/out" + std::to_string(k) + ".jpg";
        FILE* f = fopen(path.c_str(), "wb"); if (!f) { printf("cannot write %s\n", path.c_str()); return 2; }
        const bool ok = fwrite(files[k].data(), 1, files[k].size(), f) == files[k].size(); fclose(f);
        if (!ok) return 2;
        printf("%zu %zu\n", k, files[k].size());
    }
    return 0;
}
