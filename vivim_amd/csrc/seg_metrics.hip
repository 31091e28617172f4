// seg_metrics.hip -- validation metrics of a batch of logits on the device: argmax over the classes, the confusion counts
// (TP, FP, FN) of the prediction against the label map per (image, class), optionally the prediction map itself, and the six
// per-class metrics of the reference's MulticlassMetricsTracker accumulated into a caller-owned fp64 state
// (include/vivim_hip.h: vivim_seg_metrics_params; the eager composition is vivim_amd/seg_metrics.py: _eager_counts).
//
// Two launches, seg_loss.hip's tiling and slot pattern.  seg_metrics_count_kernel: a thread owns 16 bytes of consecutive pixels
// of all C channel rows plus the labels (seg_load.cuh), takes the first index of the maximum per pixel -- compared in f32, to
// which every logit type widens exactly; a NaN counts as the maximum and the first NaN wins, numpy.argmax's rule -- and counts
// per class three integers: prediction and label are c, prediction is c, label is c.  Integer wave sum, one LDS step across the
// workgroup's waves, and the workgroup STORES its 3 * C int32 into slot (image, block) of the workspace: no atomics, every
// workspace word written before it is read.  seg_metrics_finalize_kernel (one workgroup) adds the slots in slot order, writes
// counts[n][c] = {tp, fp, fn} and, when a state is given, adds for n = 0 .. N-1 in that order the six metrics of every class
// present in image n (tp + fn > 0) into state[c][0..5] and 1 into state[c][6], in fp64: the state is bit-repeatable.
// Labels are only ever COMPARED with the class index: a label outside [0, C) is a pixel of no class -- a false positive of the
// class predicted there and nothing else.
#include "seg_load.cuh"      // sl_load, sl_labels, sl_aligned16, check_seg_inputs: shared with seg_loss.hip

namespace vivim {

constexpr int kSmThreads = 256;      // 4 waves per workgroup
constexpr int kSmMaxBlocks = 64;     // workgroups per image (grid-stride loop beyond): keeps the finalise kernel tiny

static int sm_blocks_per_image(const vivim_seg_metrics_params& p) {
    const int64_t per_block = (int64_t)kSmThreads * vec_elems(p.itype);
    const int64_t b = (p.pixels + per_block - 1) / per_block;
    return (int)(b < kSmMaxBlocks ? b : kSmMaxBlocks);
}

static size_t seg_metrics_workspace_bytes(const vivim_seg_metrics_params& p) {
    return sizeof(int32_t) * (size_t)p.batch * sm_blocks_per_image(p) * (3 * p.classes);
}

// which of the three tensors a workgroup may move in whole vectors (host-side alignment verdicts, wave-uniform)
enum { kSmVecLogits = 1, kSmVecTarget = 2, kSmVecPred = 4 };

__device__ __forceinline__ int sm_wave_sum(int v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

template <typename T, int C>
__global__ void __launch_bounds__(kSmThreads) seg_metrics_count_kernel(const vivim_seg_metrics_params p, const int bpi, const int flags) {
    constexpr int E = 16 / (int)sizeof(T), NV = 3 * C, NW = kSmThreads / kWave;
    __shared__ int red[NW][NV];
    const int n = blockIdx.x / bpi, blk = blockIdx.x - n * bpi, HW = p.pixels;
    const T* __restrict__ xb = static_cast<const T*>(p.logits) + (int64_t)n * p.logits_batch_stride;
    const int64_t tb = (int64_t)n * p.target_batch_stride;
    uint8_t* __restrict__ pb = p.pred ? static_cast<uint8_t*>(p.pred) + (int64_t)n * p.pred_batch_stride : nullptr;
    int tp[C], np[C], ng[C];
#pragma unroll
    for (int c = 0; c < C; ++c) tp[c] = np[c] = ng[c] = 0;
    for (int64_t pix0 = ((int64_t)blk * kSmThreads + threadIdx.x) * E; pix0 < HW; pix0 += (int64_t)bpi * kSmThreads * E) {
        const int nv = (int)(HW - pix0 < E ? HW - pix0 : E);
        float x[C][E];
        int lab[E];
        sl_load<T, C, E>(xb + pix0, p.logits_c_stride, nv, (flags & kSmVecLogits) != 0, x);
        sl_labels<E>(p.target, p.ttype, tb + pix0, nv, (flags & kSmVecTarget) != 0, lab);
        uint32_t word[E / 4];                    // the E predictions, one byte each, little-endian
#pragma unroll
        for (int i = 0; i < E / 4; ++i) word[i] = 0u;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            float best = x[0][k];
            int arg = 0;
#pragma unroll
            for (int c = 1; c < C; ++c) {
                const float v = x[c][k];
                const bool take = v > best || (v != v && best == best);      // first maximum; a NaN is the maximum, the first NaN wins
                best = take ? v : best;
                arg = take ? c : arg;
            }
            const bool ok = k < nv;              // a tail lane holds logits 0 and label -1: it must count nothing
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool pc = ok && arg == c, lc = ok && lab[k] == c;
                tp[c] += pc && lc ? 1 : 0;
                np[c] += pc ? 1 : 0;
                ng[c] += lc ? 1 : 0;
            }
            word[k / 4] |= (uint32_t)arg << (8 * (k & 3));
        }
        if (pb) {
            uint8_t* __restrict__ q = pb + pix0;
            if ((flags & kSmVecPred) != 0 && nv >= E) {
                if constexpr (E == 4) {
                    *reinterpret_cast<uint32_t*>(q) = word[0];
                } else {
                    u32x2 w;
                    w.x = word[0];
                    w.y = word[1];
                    *reinterpret_cast<u32x2*>(q) = w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k)
                    if (k < nv) q[k] = (uint8_t)((word[k / 4] >> (8 * (k & 3))) & 255u);
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int a = sm_wave_sum(tp[c]), b = sm_wave_sum(np[c]), d = sm_wave_sum(ng[c]);
        if (lane == 0) {
            red[wave][c] = a;
            red[wave][C + c] = b;
            red[wave][2 * C + c] = d;
        }
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        int s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
        static_cast<int32_t*>(p.workspace)[(int64_t)blockIdx.x * NV + threadIdx.x] = s;      // slot (image, block)
    }
}

// one workgroup: thread t owns the (image, class) pairs t, t + 256, ... for the counts; then thread c < C walks the images in
// order and adds the metrics of class c into the state
__global__ void __launch_bounds__(kSmThreads) seg_metrics_finalize_kernel(const vivim_seg_metrics_params p, const int bpi) {
    const int C = p.classes, NV = 3 * C, tid = threadIdx.x;
    const int32_t* __restrict__ ws = static_cast<const int32_t*>(p.workspace);
    int32_t* counts = static_cast<int32_t*>(p.counts);
    for (int64_t i = tid; i < (int64_t)p.batch * C; i += kSmThreads) {
        const int64_t n = i / C;
        const int c = (int)(i - n * C);
        int tp = 0, np = 0, ng = 0;
        for (int b = 0; b < bpi; ++b) {
            const int32_t* __restrict__ s = ws + (n * bpi + b) * NV;
            tp += s[c];
            np += s[C + c];
            ng += s[2 * C + c];
        }
        counts[3 * i] = tp;
        counts[3 * i + 1] = np - tp;
        counts[3 * i + 2] = ng - tp;
    }
    if (p.state == nullptr) return;
    __syncthreads();                             // the counts of every image, written by this workgroup, are visible to it
    if (tid >= C) return;
    double* __restrict__ st = static_cast<double*>(p.state) + 7 * tid;
    double dice = st[0], jac = st[1], prec = st[2], rec = st[3], fm = st[4], spec = st[5], cnt = st[6];
    const int64_t HW = p.pixels;
    for (int64_t n = 0; n < p.batch; ++n) {
        const int32_t* q = counts + 3 * (n * C + tid);
        const int64_t tp = q[0], fp = q[1], fn = q[2];
        if (tp + fn == 0) continue;              // the class is not in this image's label map: the image says nothing about it
        const int64_t tn = HW - tp - fp - fn;
        const double pr = tp + fp == 0 ? 0.0 : (double)tp / (double)(tp + fp);
        const double rc = (double)tp / (double)(tp + fn);
        dice += 2.0 * (double)tp / (double)(2 * tp + fp + fn);
        jac += (double)tp / (double)(tp + fp + fn);
        prec += pr;
        rec += rc;
        fm += 2.0 * pr * rc / (pr + rc + 1e-5);
        spec += tp + fn == HW ? 0.0 : (double)tn / (double)(tn + fp);
        cnt += 1.0;
    }
    st[0] = dice;
    st[1] = jac;
    st[2] = prec;
    st[3] = rec;
    st[4] = fm;
    st[5] = spec;
    st[6] = cnt;
}

template <typename T, int C>
static void sm_launch(const vivim_seg_metrics_params& p, hipStream_t stream) {
    constexpr int E = 16 / (int)sizeof(T);
    const int bpi = sm_blocks_per_image(p);
    const dim3 grid((unsigned)((int64_t)p.batch * bpi)), block(kSmThreads);
    int flags = 0;
    if (sl_aligned16(p.logits, sizeof(T), {p.logits_batch_stride, p.logits_c_stride})) flags |= kSmVecLogits;
    if (sl_aligned16(p.target, p.ttype == 0 ? 8 : 1, {p.target_batch_stride})) flags |= kSmVecTarget;
    // a thread's E prediction bytes start at a multiple of E within the image: one E-byte store when the rows do as well
    if (p.pred && reinterpret_cast<uintptr_t>(p.pred) % E == 0 && p.pred_batch_stride % E == 0) flags |= kSmVecPred;
    hipLaunchKernelGGL((seg_metrics_count_kernel<T, C>), grid, block, 0, stream, p, bpi, flags);
    hipLaunchKernelGGL(seg_metrics_finalize_kernel, dim3(1), block, 0, stream, p, bpi);
}

template <typename T>
static bool sm_classes(const vivim_seg_metrics_params& p, hipStream_t stream) {
    switch (p.classes) {
        case 2: sm_launch<T, 2>(p, stream); return true;
        case 3: sm_launch<T, 3>(p, stream); return true;
        case 4: sm_launch<T, 4>(p, stream); return true;
        case 5: sm_launch<T, 5>(p, stream); return true;
        case 6: sm_launch<T, 6>(p, stream); return true;
        case 7: sm_launch<T, 7>(p, stream); return true;
        case 8: sm_launch<T, 8>(p, stream); return true;
    }
    return false;
}

static bool seg_metrics_dispatch(const vivim_seg_metrics_params& p, hipStream_t stream) {
    bool built = false;                  // false: no kernel for this class count
    return with_itype(p.itype, [&](auto t) { built = sm_classes<decltype(t)>(p, stream); }) && built;
}

}  // namespace vivim

extern "C" {

size_t vivim_seg_metrics_workspace_bytes(const vivim_seg_metrics_params* p) {
    return p && p->batch > 0 && p->pixels > 0 && p->classes > 0 && dtype_ok(p->itype) ? vivim::seg_metrics_workspace_bytes(*p) : 0;
}

int vivim_seg_metrics(const vivim_seg_metrics_params* p, void* stream) {
    if (int rc = check_seg_inputs(p, "seg_metrics")) return rc;
    VCHECK(p->counts && aligned(p->counts, 4));
    VCHECK(aligned(p->state, 8));         // NULL: not wanted (pred: any address)
    const size_t need = vivim::seg_metrics_workspace_bytes(*p);
    if (int rc = check_workspace("seg_metrics", "vivim_seg_metrics_workspace_bytes", p->workspace, p->workspace_bytes, 4, need)) return rc;
    return after_dispatch(vivim::seg_metrics_dispatch(*p, as_stream(stream)), "seg_metrics",
                          "seg_metrics not implemented for input type %d / %d classes", p->itype, p->classes);
}

}  // extern "C"
