// up_tap.cuh -- the one tap function of bilinear upsampling (align_corners = False), shared by the upsampling kernels
// (upsample.hip), the fused decode head (decode_head.hip) and the training head's concat (head_concat.hip): an output index becomes
// (i0, i1, l0, l1) with ATen's fp32 arithmetic.  Below it, what the gather-form backwards share: which outputs tap an input index.
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

__device__ __forceinline__ bool up_hits(const UpTap& t, int i) { return t.i0 == i || t.i1 == i; }
__device__ __forceinline__ float up_weight(const UpTap& t, int i) { return (t.i0 == i ? t.l0 : 0.0f) + (t.i1 == i ? t.l1 : 0.0f); }

// Output indices that can tap input index i: exactly those with src in (i - 1, i + 1), o in (A, B) with
// A = ((2i - 1) n_out - n_in) / (2 n_in) and B = ((2i + 3) n_out - n_in) / (2 n_in); two more on either side cover the fp32
// rounding of src.  (2 n_in + 3) n_out fits 31 bits (host check).  Every output whose src is clamped to 0 names i0 = 0 and, with
// l1 = 0, i1 = 1: the window of i <= 1 starts at output 0.
__device__ __forceinline__ void up_window(int i, int n_in, int n_out, int& lo, int& hi) {
    const int a = ((2 * i - 1) * n_out - n_in) / (2 * n_in) - 2;
    const int b = ((2 * i + 3) * n_out - n_in) / (2 * n_in) + 2;
    lo = i <= 1 || a < 0 ? 0 : a;
    hi = b > n_out - 1 ? n_out - 1 : b;
}

}  // namespace vivim
