// seg_load.cuh -- how the segmentation kernels (seg_loss.hip, seg_metrics.hip) read their inputs: a thread takes E consecutive
// pixels (16 bytes of logits) of C channel rows plus the labels, in whole vectors where the host-side alignment verdict
// (sl_aligned16: base pointer and every stride) allows and element by element otherwise.  And the argument checks that the
// entry points of those two files share (check_seg_inputs).
#pragma once
#include <initializer_list>
#include <type_traits>
#include "capi.cuh"

namespace vivim {

// E consecutive pixels of C channel rows, widened to f32; pixels >= nv read as 0
template <typename T, int C, int E>
__device__ __forceinline__ void sl_load(const T* __restrict__ base, int64_t c_stride, int nv, bool vec, float (&x)[C][E]) {
    if (vec && nv >= E) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const RawK<T, E> r = load_vec<T, E>(base + c * c_stride, true);
            unpack<T, E>(r, x[c]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < E; ++k) x[c][k] = k < nv ? to_f32<T>(base[c * c_stride + k]) : 0.0f;
    }
}

__device__ __forceinline__ int sl_label64(uint32_t lo, uint32_t hi) { return hi == 0u && lo < 256u ? (int)lo : -1; }

// E labels as ints in [0, 256) or -1 (any other value, or a pixel >= nv): only compared with c afterwards
template <int E>
__device__ __forceinline__ void sl_labels(const void* __restrict__ target, int ttype, int64_t off, int nv, bool vec, int (&lab)[E]) {
    if (ttype == 0) {
        const int64_t* __restrict__ q = static_cast<const int64_t*>(target) + off;
        if (vec && nv >= E) {
#pragma unroll
            for (int i = 0; i < E / 2; ++i) {
                const u32x4 v = reinterpret_cast<const u32x4*>(q)[i];
                lab[2 * i] = sl_label64(v.x, v.y);
                lab[2 * i + 1] = sl_label64(v.z, v.w);
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int64_t v = k < nv ? q[k] : (int64_t)-1;
                lab[k] = v >= 0 && v < 256 ? (int)v : -1;
            }
        }
    } else {
        const uint8_t* __restrict__ q = static_cast<const uint8_t*>(target) + off;
        if (vec && nv >= E) {
#pragma unroll
            for (int i = 0; i < E / 4; ++i) {
                const uint32_t v = reinterpret_cast<const uint32_t*>(q)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) lab[4 * i + j] = (int)((v >> (8 * j)) & 255u);
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) lab[k] = k < nv ? (int)q[k] : -1;
        }
    }
}

// the host-side verdict: base 16-byte aligned and every stride a whole number of 16-byte vectors
static inline bool sl_aligned16(const void* q, int64_t elem_bytes, std::initializer_list<int64_t> strides) {
    if (reinterpret_cast<uintptr_t>(q) & 15) return false;
    for (int64_t s : strides)
        if ((s * elem_bytes) & 15) return false;
    return true;
}

constexpr int kSegMaxClasses = 8;    // the class switches of seg_loss.hip and seg_metrics.hip instantiate 2 .. 8

}  // namespace vivim

// the checks on logits, target and classes that the entry points of the segmentation loss (`name` "seg_loss") and metrics
// ("seg_metrics") share; the loss's gamma is refused where it always was, between the class count and the grid bound
template <class P> static int check_seg_inputs(const P* p, const char* name) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && (p->ttype == 0 || p->ttype == 1));
    VCHECK(p->batch > 0 && p->pixels > 0);
    if (p->classes < 2 || p->classes > vivim::kSegMaxClasses)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: %d classes: the kernels are built for 2 to %d classes", name, p->classes,
                    vivim::kSegMaxClasses);
    if constexpr (std::is_same<P, vivim_seg_loss_params>::value)
        if (p->gamma != 2.0f)
            return fail(VIVIM_ERR_UNSUPPORTED, "seg_loss: gamma = %g: the kernels are built for gamma = 2 only", (double)p->gamma);
    VCHECK((int64_t)p->batch * 64 <= INT32_MAX);                  // one workgroup index per (image, block)
    VCHECK(p->logits && aligned(p->logits, p->itype == VIVIM_F32 ? 4 : 2));
    VCHECK(p->target && aligned(p->target, p->ttype == 0 ? 8 : 1));
    return VIVIM_OK;
}
