// seg_loss.hip -- the train step's loss, 0.4 * class-balanced focal + 0.6 * Tversky over softmax(logits), forward and backward
// (include/vivim_hip.h: vivim_seg_loss_params; the eager composition is vivim_amd/train_step.py: recall_focused_loss).
//
// Three launches instead of several dozen ATen ops each way, no per-pixel tensor kept for autograd, and no cancellation:
//   * q_c = 1 - p_c is formed as (sum of the OTHER classes' exponentials) / (softmax denominator), never by subtraction, so
//     ln(q_c + eps) and q_c^2 keep their relative precision when p_c -> 1;
//   * the softmax backward is p_c * (q_c * g_c - sum_{k != c} p_k * g_k): no p_c * g_c - p_c * p_c * g_c.
// seg_loss_partial_kernel: a thread owns 16 bytes of consecutive pixels for all C channels (C loads of dwordx4 + the labels),
// accumulates the focal sum and the 3 * C Tversky sums (TP, FP, FN) of its image in registers; wave_sum, one LDS step across the
// workgroup's waves, and the workgroup STORES its 3 * C + 1 floats into slot (image, block) of the workspace (det.cuh's slot
// pattern: no float atomics, the order of every sum depends on the shape alone).  seg_loss_finalize_kernel adds the slots in
// slot order, writes the loss and, per (image, class), the two Tversky gradient factors the backward needs.
// seg_loss_bwd_kernel recomputes the softmax with the same tiling and writes dlogits in the logits' type.
// Labels are only ever COMPARED with the class index: a label outside [0, C) is a pixel that belongs to no class.
#include "seg_load.cuh"      // sl_load, sl_labels, sl_aligned16, check_seg_inputs: shared with seg_metrics.hip

namespace vivim {

constexpr int kSlThreads = 256;      // 4 waves per workgroup
constexpr int kSlMaxBlocks = 64;     // workgroups per image (grid-stride loop beyond): keeps the finalise kernel tiny

static int sl_blocks_per_image(const vivim_seg_loss_params& p) {
    const int64_t per_block = (int64_t)kSlThreads * vec_elems(p.itype);
    const int64_t b = (p.pixels + per_block - 1) / per_block;
    return (int)(b < kSlMaxBlocks ? b : kSlMaxBlocks);
}

static size_t seg_loss_workspace_bytes(const vivim_seg_loss_params& p) {
    return sizeof(float) * (size_t)p.batch * sl_blocks_per_image(p) * (3 * p.classes + 1);
}

// which of the three tensors a workgroup may move in whole 16-byte vectors (host-side alignment verdicts, wave-uniform)
enum { kSlVecLogits = 1, kSlVecTarget = 2, kSlVecDlogits = 4 };

// softmax of one pixel: p_c and q_c = 1 - p_c as the other classes' share of the denominator
template <int C>
__device__ __forceinline__ void sl_softmax(const float (&x)[C], float (&pr)[C], float (&qr)[C]) {
    float m = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float e[C], S = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        e[c] = fast_exp2((x[c] - m) * kLog2e);       // an exponential that underflows is p = 0: the + eps below covers it
        S += e[c];
    }
    const float r = 1.0f / S;                        // S >= 1: the maximum's own term
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float o = 0.0f;
#pragma unroll
        for (int k = 0; k < C; ++k)
            if (k != c) o += e[k];
        pr[c] = e[c] * r;
        qr[c] = o * r;
    }
}

template <typename T, int C>
__global__ void __launch_bounds__(kSlThreads) seg_loss_partial_kernel(const vivim_seg_loss_params p, const int bpi, const int flags) {
    constexpr int E = 16 / (int)sizeof(T), NV = 3 * C + 1, NW = kSlThreads / kWave;
    __shared__ float red[NW][NV];
    const int n = blockIdx.x / bpi, blk = blockIdx.x - n * bpi, HW = p.pixels;
    const T* __restrict__ xb = static_cast<const T*>(p.logits) + (int64_t)n * p.logits_batch_stride;
    const int64_t tb = (int64_t)n * p.target_batch_stride;
    float alpha[C];
#pragma unroll
    for (int c = 0; c < C; ++c) alpha[c] = static_cast<const float*>(p.alpha)[c];
    float phi = 0.0f, tp[C], fp[C], fn[C];
#pragma unroll
    for (int c = 0; c < C; ++c) tp[c] = fp[c] = fn[c] = 0.0f;
    for (int64_t pix0 = ((int64_t)blk * kSlThreads + threadIdx.x) * E; pix0 < HW; pix0 += (int64_t)bpi * kSlThreads * E) {
        const int nv = (int)(HW - pix0 < E ? HW - pix0 : E);
        float x[C][E];
        int lab[E];
        sl_load<T, C, E>(xb + pix0, p.logits_c_stride, nv, (flags & kSlVecLogits) != 0, x);
        sl_labels<E>(p.target, p.ttype, tb + pix0, nv, (flags & kSlVecTarget) != 0, lab);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            float xk[C], pr[C], qr[C];
#pragma unroll
            for (int c = 0; c < C; ++c) xk[c] = x[c][k];
            sl_softmax<C>(xk, pr, qr);
            const bool ok = k < nv;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool y = lab[k] == c;
                const float arg = y ? pr[c] : qr[c], w = y ? qr[c] : pr[c];
                const float f = alpha[c] * w * w * (-kLn2 * __builtin_amdgcn_logf(arg + p.eps));
                phi += ok ? f : 0.0f;
                tp[c] += ok && y ? pr[c] : 0.0f;
                fp[c] += ok && !y ? pr[c] : 0.0f;
                fn[c] += ok && y ? qr[c] : 0.0f;
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    phi = wave_sum(phi);
    if (lane == 0) red[wave][0] = phi;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a = wave_sum(tp[c]), b = wave_sum(fp[c]), d = wave_sum(fn[c]);
        if (lane == 0) {
            red[wave][1 + c] = a;
            red[wave][1 + C + c] = b;
            red[wave][1 + 2 * C + c] = d;
        }
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
        static_cast<float*>(p.workspace)[(int64_t)blockIdx.x * NV + threadIdx.x] = s;      // slot (image, block)
    }
}

// one workgroup: thread t owns the (image, class) pairs and the focal slots t, t + 256, ...; then a fixed LDS tree
__global__ void __launch_bounds__(kSlThreads) seg_loss_finalize_kernel(const vivim_seg_loss_params p, const int bpi, const float inv_npix,
                                                                       const float inv_nc) {
    __shared__ float red[2][kSlThreads];
    const int C = p.classes, NV = 3 * C + 1, tid = threadIdx.x;
    const float* __restrict__ ws = static_cast<const float*>(p.workspace);
    float* __restrict__ coef = static_cast<float*>(p.coef);
    float tv = 0.0f, phi = 0.0f;
    for (int64_t i = tid; i < (int64_t)p.batch * C; i += kSlThreads) {
        const int64_t n = i / C;
        const int c = (int)(i - n * C);
        float tp = 0.0f, fp = 0.0f, fn = 0.0f;
        for (int b = 0; b < bpi; ++b) {
            const float* __restrict__ s = ws + (n * bpi + b) * NV;
            tp += s[1 + c];
            fp += s[1 + C + c];
            fn += s[1 + 2 * C + c];
        }
        const float tps = tp + p.smooth;
        const float den = tp + p.tversky_alpha * fp + p.tversky_beta * fn + p.smooth;
        tv += tps / den;
        if (coef) {
            coef[2 * i] = (den - tps * (1.0f - p.tversky_beta)) / (den * den);       // d tv / d p_c where the pixel is of class c
            coef[2 * i + 1] = -tps * p.tversky_alpha / (den * den);                  // ... where it is not
        }
    }
    for (int64_t i = tid; i < (int64_t)p.batch * bpi; i += kSlThreads) phi += ws[i * NV];
    red[0][tid] = phi;
    red[1][tid] = tv;
    __syncthreads();
    for (int off = kSlThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0)
        *static_cast<float*>(p.loss) = p.focal_weight * (red[0][0] * inv_npix) + p.tversky_weight * (1.0f - red[1][0] * inv_nc);
}

// kf = focal_weight / (N * HW), kt = tversky_weight / (N * C)
template <typename T, int C>
__global__ void __launch_bounds__(kSlThreads) seg_loss_bwd_kernel(const vivim_seg_loss_params p, const int bpi, const int flags,
                                                                  const float kf, const float kt) {
    constexpr int E = 16 / (int)sizeof(T);
    const int n = blockIdx.x / bpi, blk = blockIdx.x - n * bpi, HW = p.pixels;
    const T* __restrict__ xb = static_cast<const T*>(p.logits) + (int64_t)n * p.logits_batch_stride;
    T* __restrict__ db = static_cast<T*>(p.dlogits) + (int64_t)n * p.dlogits_batch_stride;
    const int64_t tb = (int64_t)n * p.target_batch_stride;
    const float go = *static_cast<const float*>(p.grad_out);
    float alpha[C], g1[C], g0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        alpha[c] = kf * static_cast<const float*>(p.alpha)[c];
        g1[c] = kt * static_cast<const float*>(p.coef)[((int64_t)n * C + c) * 2];
        g0[c] = kt * static_cast<const float*>(p.coef)[((int64_t)n * C + c) * 2 + 1];
    }
    for (int64_t pix0 = ((int64_t)blk * kSlThreads + threadIdx.x) * E; pix0 < HW; pix0 += (int64_t)bpi * kSlThreads * E) {
        const int nv = (int)(HW - pix0 < E ? HW - pix0 : E);
        float x[C][E];
        int lab[E];
        sl_load<T, C, E>(xb + pix0, p.logits_c_stride, nv, (flags & kSlVecLogits) != 0, x);
        sl_labels<E>(p.target, p.ttype, tb + pix0, nv, (flags & kSlVecTarget) != 0, lab);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            float xk[C], pr[C], qr[C], g[C];
#pragma unroll
            for (int c = 0; c < C; ++c) xk[c] = x[c][k];
            sl_softmax<C>(xk, pr, qr);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool y = lab[k] == c;
                const float arg = (y ? pr[c] : qr[c]) + p.eps, w = y ? qr[c] : pr[c];
                // d/dp of the class's focal term with q = 1 - p: +t where the pixel is of class c, -t where it is not
                const float t = 2.0f * w * (kLn2 * __builtin_amdgcn_logf(arg)) - w * w * fast_rcp(arg);
                g[c] = alpha[c] * (y ? t : -t) - (y ? g1[c] : g0[c]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float o = 0.0f;
#pragma unroll
                for (int j = 0; j < C; ++j)
                    if (j != c) o = fmaf(pr[j], g[j], o);
                x[c][k] = go * (pr[c] * (qr[c] * g[c] - o));     // f32 all the way: rounded once, below
            }
        }
        if ((flags & kSlVecDlogits) != 0 && nv >= E) {
#pragma unroll
            for (int c = 0; c < C; ++c) store_vec<T, E>(db + c * p.dlogits_c_stride + pix0, true, x[c]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < E; ++k)
                    if (k < nv) db[c * p.dlogits_c_stride + pix0 + k] = from_f32<T>(x[c][k]);
        }
    }
}

template <typename T, int C>
static void sl_launch(const vivim_seg_loss_params& p, bool bwd, hipStream_t stream) {
    const int bpi = sl_blocks_per_image(p);
    const dim3 grid((unsigned)((int64_t)p.batch * bpi)), block(kSlThreads);
    int flags = 0;
    if (sl_aligned16(p.logits, sizeof(T), {p.logits_batch_stride, p.logits_c_stride})) flags |= kSlVecLogits;
    if (sl_aligned16(p.target, p.ttype == 0 ? 8 : 1, {p.target_batch_stride})) flags |= kSlVecTarget;
    if (!bwd) {
        hipLaunchKernelGGL((seg_loss_partial_kernel<T, C>), grid, block, 0, stream, p, bpi, flags);
        hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), block, 0, stream, p, bpi,
                           (float)(1.0 / ((double)p.batch * p.pixels)), (float)(1.0 / ((double)p.batch * p.classes)));
        return;
    }
    if (sl_aligned16(p.dlogits, sizeof(T), {p.dlogits_batch_stride, p.dlogits_c_stride})) flags |= kSlVecDlogits;
    hipLaunchKernelGGL((seg_loss_bwd_kernel<T, C>), grid, block, 0, stream, p, bpi, flags,
                       (float)((double)p.focal_weight / ((double)p.batch * p.pixels)),
                       (float)((double)p.tversky_weight / ((double)p.batch * p.classes)));
}

template <typename T>
static bool sl_classes(const vivim_seg_loss_params& p, bool bwd, hipStream_t stream) {
    switch (p.classes) {
        case 2: sl_launch<T, 2>(p, bwd, stream); return true;
        case 3: sl_launch<T, 3>(p, bwd, stream); return true;
        case 4: sl_launch<T, 4>(p, bwd, stream); return true;
        case 5: sl_launch<T, 5>(p, bwd, stream); return true;
        case 6: sl_launch<T, 6>(p, bwd, stream); return true;
        case 7: sl_launch<T, 7>(p, bwd, stream); return true;
        case 8: sl_launch<T, 8>(p, bwd, stream); return true;
    }
    return false;
}

static bool seg_loss_dispatch(const vivim_seg_loss_params& p, bool bwd, hipStream_t stream) {
    bool built = false;                  // false: no kernel for this class count
    return with_itype(p.itype, [&](auto t) { built = sl_classes<decltype(t)>(p, bwd, stream); }) && built;
}

}  // namespace vivim

// ---- the C entry points
// what the forward and the backward of the segmentation loss share
static int check_seg_loss(const vivim_seg_loss_params* p) {
    if (int rc = check_seg_inputs(p, "seg_loss")) return rc;
    VCHECK(p->alpha && aligned(p->alpha, 4));
    return VIVIM_OK;
}

extern "C" {

size_t vivim_seg_loss_workspace_bytes(const vivim_seg_loss_params* p) {
    return p && p->batch > 0 && p->pixels > 0 && p->classes > 0 && dtype_ok(p->itype) ? vivim::seg_loss_workspace_bytes(*p) : 0;
}

int vivim_seg_loss_fwd(const vivim_seg_loss_params* p, void* stream) {
    if (int rc = check_seg_loss(p)) return rc;
    VCHECK(p->loss && aligned(p->loss, 4));
    VCHECK(aligned(p->coef, 4));                                    // NULL: not wanted
    const size_t need = vivim::seg_loss_workspace_bytes(*p);
    if (int rc = check_workspace("seg_loss_fwd", "vivim_seg_loss_workspace_bytes", p->workspace, p->workspace_bytes, 4, need)) return rc;
    return after_dispatch(vivim::seg_loss_dispatch(*p, false, as_stream(stream)), "seg_loss_fwd",
                          "seg_loss_fwd not implemented for input type %d / %d classes", p->itype, p->classes);
}

int vivim_seg_loss_bwd(const vivim_seg_loss_params* p, void* stream) {
    if (int rc = check_seg_loss(p)) return rc;
    const uintptr_t ib = elem_bytes(p->itype);
    VCHECK(p->coef && aligned(p->coef, 4));
    VCHECK(p->grad_out && aligned(p->grad_out, 4));
    VCHECK(p->dlogits && aligned(p->dlogits, ib));
    return after_dispatch(vivim::seg_loss_dispatch(*p, true, as_stream(stream)), "seg_loss_bwd",
                          "seg_loss_bwd not implemented for input type %d / %d classes", p->itype, p->classes);
}

}  // extern "C"
