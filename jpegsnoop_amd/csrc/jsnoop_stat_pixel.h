// jsnoop_stat_pixel.h -- the value part of one pixel of the bHistoEn / bStatClipEn colour path, shared by k_color_stats / k_clip_order
// (jsnoop_kernels.hip, one pixel per thread) and k_stats_batch / k_stats_order (jsnoop_stats.hip, eight pixels per lane): everything
// ConvertYCCtoRGB :4229-4326, CapYccRange :4341-4475 and CapRgbRange :4495-4601 compute from the three plane samples of a pixel.
// The loads are the callers' business; the arithmetic is here once, so that both doors give the same words by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct StatPix { int pre[3]; int clipv[3]; int fin[3]; int lim[3]; int rgb[3]; };

// o.pre holds the plane samples (Cb = Cr = 0 for a one-component scan, :4709-4715).  `shifted`: the pixel's MCU index is not below the shift origin;
// `im`: anything with the preview shift in shift_y / shift_cb / shift_cr (JsImage, JsStatRec).
template <class Shift>
__device__ __forceinline__ void stat_values(StatPix& o, bool shifted, const Shift& im)
{
    if (shifted) { o.pre[0] += im.shift_y; o.pre[1] += im.shift_cb; o.pre[2] += im.shift_cr; }                           // :4735-4739
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        o.clipv[c] = (o.pre[c] + 1024) / 8;                      // C division, truncates toward zero (:4265-4267)
        o.fin[c] = min(max(o.clipv[c], 0), 255);                 // CapYccRange
    }
    const float kr = 0.299f, kg = 0.587f, kb = 0.114f;
    const float cr_mul = 2 - 2 * kr, cb_mul = 2 - 2 * kb;
    const float fy = (float)(o.fin[0] - 128);
    float r = __fadd_rn(__fmul_rn((float)(o.fin[2] - 128), cr_mul), fy);
    float b = __fadd_rn(__fmul_rn((float)(o.fin[1] - 128), cb_mul), fy);
    float g = __fdiv_rn(__fsub_rn(__fsub_rn(fy, __fmul_rn(kb, b)), __fmul_rn(kr, r)), kg);
    r = __fadd_rn(r, 128.0f); b = __fadd_rn(b, 128.0f); g = __fadd_rn(g, 128.0f);
    o.lim[0] = (int)r; o.lim[1] = (int)g; o.lim[2] = (int)b;      // CapRgbRange truncates first, then range-checks the ints
    #pragma unroll
    for (int c = 0; c < 3; c++) o.rgb[c] = min(max(o.lim[c], 0), 255);
}
