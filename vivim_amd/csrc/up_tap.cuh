// up_tap.cuh -- the one tap function of bilinear upsampling (align_corners = False), shared by the upsampling kernels
// (upsample.hip) and the fused decode head (decode_head.hip): an output index becomes (i0, i1, l0, l1) with ATen's fp32 arithmetic.
#pragma once
#include "common.cuh"

namespace vivim {

struct UpTap {
    int i0, i1;
    float l0, l1;
};

// ATen's area_pixel_compute_source_index and the index / lambda lines after it, per axis, in fp32.  The fma is spelled out so
// that every kernel forms the same src whatever the compiler would contract: forward and backward are exact transposes.
__device__ __forceinline__ UpTap up_tap(int o, float r, int n_in) {
    float src = fmaf(r, (float)o + 0.5f, -0.5f);
    src = src < 0.0f ? 0.0f : src;
    UpTap t;
    t.i0 = min((int)src, n_in - 1);              // src < n_in - 0.5 for r <= 1: the min never binds, it keeps a read in range
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

}  // namespace vivim
