// det.hip -- the fixed-order slot reduction of the deterministic backward variants (det.cuh).
#include "det.cuh"

namespace vivim {

__global__ void __launch_bounds__(256) det_reduce_kernel(const float* __restrict__ ws, int slots, int64_t n, int64_t sstride, DetOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t rest = i, off = 0;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const int64_t c = rest % o.size[k];
        rest /= o.size[k];
        off += c * o.stride[k];
    }
    float acc = o.out[off];
    for (int s = 0; s < slots; ++s) acc += ws[(int64_t)s * sstride + i];    // adjacent threads read adjacent floats
    o.out[off] = acc;
}

void det_reduce(const float* ws, int slots, const DetOut& o, hipStream_t stream, int64_t slot_stride) {
    const int64_t n = det_numel(o);
    if (n <= 0 || slots <= 0) return;
    hipLaunchKernelGGL(det_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, slots, n,
                       slot_stride ? slot_stride : n, o);
}

}  // namespace vivim
