// det.cuh -- the deterministic backward variants (vivim_*_bwd_det, include/vivim_hip.h).
//
// Every float gradient that the default kernels add up across workgroups with atomics is, in the deterministic variant,
// STORED by each contributing workgroup into its own slot of a caller-provided workspace: slot s of an output of n
// elements is ws[s * n, (s + 1) * n), in the output's logical row-major order, and s comes from the workgroup's
// coordinates (batch, segment, channel set, ...), never from its arrival.  det_reduce then adds the slots to the
// pre-zeroed output in slot order, one thread per element: out = ((out + ws[0]) + ws[1]) + ... -- the order depends on
// the shape alone.
#pragma once
#include <initializer_list>
#include "common.cuh"

namespace vivim {

template <bool DET> __device__ __forceinline__ void det_add(float* p, float v) {
    if constexpr (DET) *p = v; else atomicAdd(p, v);
}

// An output of up to four dimensions (unused leading ones have size 1), element strides.
struct DetOut {
    float* out;
    int64_t size[4];
    int64_t stride[4];
};
inline DetOut det_out(float* out, std::initializer_list<int64_t> sizes, std::initializer_list<int64_t> strides) {
    DetOut o{out, {1, 1, 1, 1}, {0, 0, 0, 0}};
    int k = 4 - (int)sizes.size();
    for (int64_t v : sizes) o.size[k++] = v;
    k = 4 - (int)strides.size();
    for (int64_t v : strides) o.stride[k++] = v;
    return o;
}
inline int64_t det_numel(const DetOut& o) { return o.size[0] * o.size[1] * o.size[2] * o.size[3]; }

// out[i] += sum over s < slots of ws[s * slot_stride + i], s ascending (det.hip); slot_stride 0: numel.
void det_reduce(const float* ws, int slots, const DetOut& o, hipStream_t stream, int64_t slot_stride = 0);

// What a *_det_dispatch reports to its entry point, where after_det_dispatch (capi.cuh) words the refusal: nothing was
// launched unless it is `ok`.
enum class Launch { ok, unsupported, bad_workspace };
// The slot workspace of a call: present, 16-byte aligned and of at least `need` bytes.
inline bool det_ws_ok(const void* ws, size_t bytes, size_t need) {
    return ws != nullptr && bytes >= need && reinterpret_cast<uintptr_t>(ws) % 16 == 0;
}

}  // namespace vivim
