// optimizer.hip -- the optimizer end of the train step on the device: unscale, non-finite detection, global L2 norm, clipping,
// AdamW, the step counter and GradScaler's loss-scale policy, in a handful of launches and without a host synchronisation
// (include/vivim_hip.h: vivim_opt_step_params; the Python side is vivim_amd/optimizer.py: FusedStepAdamW).
//
// Three kernels.  opt_grad_stats_kernel and opt_adamw_kernel are multi-tensor: workgroup b of a launch looks up row
// first_block + b of the block map (tensor, chunk) -- a device table built once -- and works on VIVIM_OPT_CHUNK consecutive
// elements of that tensor.  What changes every step, the gradients' addresses, travels in the kernel arguments: a by-value
// table of at most VIVIM_OPT_MAX_TENSORS (pointer, element count) pairs, copied by the launch itself, so there is no staging
// buffer whose lifetime anyone has to manage; a longer parameter list is cut into several launches by the caller.
//   opt_grad_stats_kernel: x = g * inv_scale (inv_scale = 1 / loss scale from the record, a power of two: exact), a thread adds
//     its 16 squares in one fp32 chain, wave sum, one LDS step, and the workgroup STORES (sum, any non-finite g) into its own
//     slot of the workspace.  No atomics; every slot is written by exactly one workgroup of the step.
//   opt_finalise_kernel (one workgroup): adds the slots in fixed order in fp64, writes the norm, found_inf, the clip
//     coefficient and the factor every gradient is multiplied with, advances t and the two bias corrections unless the step
//     is skipped, and runs the loss-scale policy (halve on overflow; double after 2000 good steps).
//   opt_adamw_kernel: returns at once when found_inf is set; otherwise the decoupled-weight-decay update in fp32 with one
//     rounding per stored value.  16-byte accesses where the four addresses of a chunk allow, element accesses otherwise
//     (Mamba's per-direction Parameters are rows of a stacked buffer and need not be 16-byte aligned), and for a chunk's tail.
// A tensor whose gradient pointer is NULL is left out of the step: its slots are written as (0, 0), its state is not touched.
//
// Master weights (vivim_opt_mw_params): the two multi-tensor kernels are templates over the gradient's element type.  With a
// 16-bit type (fp16, bf16) the gradient is widened to fp32 exactly and opt_adamw_kernel updates an fp32 master with the fp32
// arithmetic unchanged, then stores p16 = RNE(master') into the model's parameter.  A thread still owns four consecutive
// elements per iteration (8-byte accesses of the 16-bit tensors), so the chain, wave and slot sums run in the fp32 kernels'
// order and the results are those of the fp32 route fed the widened gradients, bit for bit.  A launch is homogeneous: the
// caller orders its tables by type and no call straddles two.
#include <math.h>
#include <string.h>
#include "capi.cuh"

namespace vivim {

constexpr int kOptThreads = 256;                                       // 4 waves per workgroup
constexpr int kOptVec = 4;                                             // floats per 16-byte access
constexpr int kOptIters = VIVIM_OPT_CHUNK / (kOptThreads * kOptVec);   // accesses per thread and tensor
static_assert(kOptIters * kOptThreads * kOptVec == VIVIM_OPT_CHUNK, "a chunk is a whole number of 16-byte accesses per thread");
static_assert(kOptIters * kOptVec <= 256, "a thread's chain of additions is at most 256 long");
constexpr int kOptGrowthInterval = 2000;                               // GradScaler's growth_interval

// the record's words (include/vivim_hip.h)
enum { kOsScale = 0, kOsGrowth, kOsStep, kOsNorm, kOsFoundInf, kOsFactor, kOsBc1, kOsBc2s, kOsSkipped, kOsClip };

struct OptArgs {                       // the kernel arguments of the two multi-tensor kernels
    int32_t first_tensor, count, first_block, scaled;
    void* const* p;                    // device tables, one entry per tensor of the whole list; p has the gradient's type
    float* const* m;
    float* const* v;
    float* const* w;                   // the fp32 masters of 16-bit parameters (unused by the fp32 kernels)
    const int32_t* block_map;          // device: (tensor, chunk) per workgroup of the whole list
    uint32_t* state;
    float* workspace;
    float lr, omb1, b2, omb2, eps, decay;
    const void* g[VIVIM_OPT_MAX_TENSORS];       // this launch's tensors: first_tensor .. first_tensor + count - 1
    int64_t n[VIVIM_OPT_MAX_TENSORS];
};
static_assert(sizeof(OptArgs) <= 4096, "the by-value table must fit 4 KB of kernel arguments");

struct OptFinArgs {
    uint32_t* state;
    const float* workspace;
    int32_t total_blocks, scaled, has_max_norm, _pad;
    double max_norm, beta1, beta2;
};

// -> this workgroup's tensor of the launch (or -1), its first element and how many of the chunk exist
__device__ __forceinline__ int opt_locate(const OptArgs& a, int blk, int64_t& off, int& nb) {
    const int ti = __builtin_amdgcn_readfirstlane(a.block_map[2 * (int64_t)blk]);
    const int chunk = __builtin_amdgcn_readfirstlane(a.block_map[2 * (int64_t)blk + 1]);
    const int li = ti - a.first_tensor;
    if (li < 0 || li >= a.count || chunk < 0) return -1;             // a map row of another launch: nothing to do
    off = (int64_t)chunk * VIVIM_OPT_CHUNK;
    const int64_t rem = a.n[li] - off;
    if (rem <= 0 || a.g[li] == nullptr) return -1;
    nb = (int)(rem < VIVIM_OPT_CHUNK ? rem : VIVIM_OPT_CHUNK);
    return li;
}

// whether q takes one access of four elements: 16 bytes of fp32, 8 bytes of a 16-bit type
template <typename T> __device__ __forceinline__ bool opt_aligned(const T* q) {
    return (reinterpret_cast<uintptr_t>(q) & (kOptVec * sizeof(T) - 1)) == 0;
}

// fp32 <-> the 16-bit types.  Widening is exact.  Narrowing is round-to-nearest-even with torch's results in every bit: fp16
// through the hardware conversion (overflow gives inf, subnormals are rounded), bf16 in integer arithmetic (a NaN becomes 0x7fc0).
__device__ __forceinline__ float opt_widen(float x) { return x; }
__device__ __forceinline__ float opt_widen(f16_t x) { return static_cast<float>(x); }
__device__ __forceinline__ float opt_widen(bf16_t x) { return __uint_as_float((uint32_t)__builtin_bit_cast(uint16_t, x) << 16); }
template <typename T> __device__ __forceinline__ T opt_narrow(float x);
template <> __device__ __forceinline__ f16_t opt_narrow<f16_t>(float x) { return static_cast<f16_t>(x); }
template <> __device__ __forceinline__ bf16_t opt_narrow<bf16_t>(float x) {
    const uint32_t u = __float_as_uint(x);
    const uint16_t r = x != x ? (uint16_t)0x7fc0 : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    return __builtin_bit_cast(bf16_t, r);
}

// 4 consecutive elements from q[i..] as fp32: one access when `vec` and all four exist, else the existing ones; the rest read as 0
template <typename T>
__device__ __forceinline__ void opt_load4(const T* __restrict__ q, int i, int nb, bool vec, float (&x)[kOptVec]) {
    if (vec && i + kOptVec <= nb) {
        if constexpr (sizeof(T) == 4) {
            const float4 t = *reinterpret_cast<const float4*>(q + i);
            x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
        } else {
            union { u32x2 raw; T e[kOptVec]; } u;
            u.raw = *reinterpret_cast<const u32x2*>(q + i);
#pragma unroll
            for (int k = 0; k < kOptVec; ++k) x[k] = opt_widen(u.e[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kOptVec; ++k) x[k] = i + k < nb ? opt_widen(q[i + k]) : 0.0f;
    }
}

template <typename T>
__device__ __forceinline__ void opt_store4(T* __restrict__ q, int i, int nb, bool vec, const float (&x)[kOptVec]) {
    if constexpr (sizeof(T) == 4) {
        if (vec && i + kOptVec <= nb) {
            *reinterpret_cast<float4*>(q + i) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kOptVec; ++k)
                if (i + k < nb) q[i + k] = x[k];
        }
    } else {
        union { u32x2 raw; T e[kOptVec]; } u;
#pragma unroll
        for (int k = 0; k < kOptVec; ++k) u.e[k] = opt_narrow<T>(x[k]);
        if (vec && i + kOptVec <= nb) {
            *reinterpret_cast<u32x2*>(q + i) = u.raw;
        } else {
#pragma unroll
            for (int k = 0; k < kOptVec; ++k)
                if (i + k < nb) q[i + k] = u.e[k];
        }
    }
}

template <typename G>   // the gradient's element type: float, f16_t or bf16_t
__global__ void __launch_bounds__(kOptThreads) opt_grad_stats_kernel(const OptArgs a) {
    constexpr int NW = kOptThreads / kWave;
    __shared__ float red[NW];
    __shared__ int bad[NW];
    const int blk = a.first_block + (int)blockIdx.x, tid = threadIdx.x;
    int64_t off = 0;
    int nb = 0;
    const int li = opt_locate(a, blk, off, nb);
    float acc = 0.0f;
    int nonfinite = 0;
    if (li >= 0) {
        const float inv_scale = a.scaled ? 1.0f / reinterpret_cast<const float*>(a.state)[kOsScale] : 1.0f;
        const G* __restrict__ g = static_cast<const G*>(a.g[li]) + off;
        const bool vec = opt_aligned(g);
        float x[kOptIters][kOptVec];
#pragma unroll
        for (int it = 0; it < kOptIters; ++it) opt_load4(g, (it * kOptThreads + tid) * kOptVec, nb, vec, x[it]);
#pragma unroll
        for (int it = 0; it < kOptIters; ++it)
#pragma unroll
            for (int k = 0; k < kOptVec; ++k) {
                nonfinite |= (__float_as_uint(x[it][k]) & 0x7f800000u) == 0x7f800000u ? 1 : 0;     // inf or nan
                const float y = x[it][k] * inv_scale;
                acc = fmaf(y, y, acc);
            }
    }
    acc = wave_sum(acc);
    nonfinite = __any(nonfinite) ? 1 : 0;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    if (lane == 0) {
        red[wave] = acc;
        bad[wave] = nonfinite;
    }
    __syncthreads();
    if (tid == 0) {
        float s = red[0];
        int b = bad[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            s += red[w];
            b |= bad[w];
        }
        a.workspace[2 * (int64_t)blk] = s;                                   // slot blk: written, never added to
        reinterpret_cast<int32_t*>(a.workspace)[2 * (int64_t)blk + 1] = b;
    }
}

__device__ __forceinline__ double opt_ipow(double b, int t) {              // b^t by squaring: no libm, the same bits everywhere
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__global__ void __launch_bounds__(kOptThreads) opt_finalise_kernel(const OptFinArgs a) {
    __shared__ double sred[kOptThreads];
    __shared__ int bred[kOptThreads];
    const int tid = threadIdx.x;
    double s = 0.0;
    int b = 0;
#pragma unroll 8
    for (int i = tid; i < a.total_blocks; i += kOptThreads) {                // thread t: slots t, t + 256, ... in that order
        const float2 slot = reinterpret_cast<const float2*>(a.workspace)[i];  // (sum, flag): the workspace is 8-byte aligned
        s += (double)slot.x;
        b |= __float_as_int(slot.y);
    }
    sred[tid] = s;
    bred[tid] = b;
    __syncthreads();
    for (int w = kOptThreads / 2; w > 0; w >>= 1) {                          // a fixed tree
        if (tid < w) {
            sred[tid] += sred[tid + w];
            bred[tid] |= bred[tid + w];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    float* sf = reinterpret_cast<float*>(a.state);
    int32_t* si = reinterpret_cast<int32_t*>(a.state);
    const float scale = sf[kOsScale];
    const double inv_scale = a.scaled ? 1.0 / (double)scale : 1.0;
    bool found = false;
    double clip = 1.0;
    if (a.total_blocks > 0) {                                                // else: no pass over the gradients was made
        const double sum = sred[0], norm = sqrt(sum);
        found = bred[0] != 0 || !isfinite(sum);
        if (a.has_max_norm && !found) clip = fmin(1.0, a.max_norm / (norm + 1e-6));
        sf[kOsNorm] = (float)norm;
    }
    si[kOsFoundInf] = found ? 1 : 0;
    sf[kOsClip] = (float)clip;
    sf[kOsFactor] = found ? 0.0f : (float)(inv_scale * clip);
    if (!found) {
        const int t = si[kOsStep] + 1;
        si[kOsStep] = t;
        sf[kOsBc1] = (float)(1.0 - opt_ipow(a.beta1, t));
        sf[kOsBc2s] = (float)sqrt(1.0 - opt_ipow(a.beta2, t));
    } else {
        si[kOsSkipped] += 1;
    }
    if (a.scaled) {                                                          // GradScaler's policy
        if (found) {
            sf[kOsScale] = scale * 0.5f;
            si[kOsGrowth] = 0;
        } else {
            const int good = si[kOsGrowth] + 1;
            const bool grow = good >= kOptGrowthInterval;
            if (grow) sf[kOsScale] = scale * 2.0f;
            si[kOsGrowth] = grow ? 0 : good;
        }
    }
}

// G = float: p is the fp32 parameter.  G = f16_t / bf16_t: the fp32 value lives in the master w, p receives its rounded copy.
template <typename G>
__global__ void __launch_bounds__(kOptThreads) opt_adamw_kernel(const OptArgs a) {
    constexpr bool kMaster = sizeof(G) == 2;
    if (reinterpret_cast<const int32_t*>(a.state)[kOsFoundInf] != 0) return;      // a skipped step writes nothing
    const int blk = a.first_block + (int)blockIdx.x, tid = threadIdx.x;
    int64_t off = 0;
    int nb = 0;
    const int li = opt_locate(a, blk, off, nb);
    if (li < 0) return;
    const float* sf = reinterpret_cast<const float*>(a.state);
    const float factor = sf[kOsFactor], bc2s = sf[kOsBc2s];
    const float step_size = a.lr / sf[kOsBc1];
    const int ti = a.first_tensor + li;
    const G* __restrict__ g = static_cast<const G*>(a.g[li]) + off;
    G* __restrict__ p16 = static_cast<G*>(a.p[ti]) + off;                         // only stored to, and only with a master
    float* __restrict__ p = kMaster ? a.w[ti] + off : reinterpret_cast<float*>(p16);
    float* __restrict__ m = a.m[ti] + off;
    float* __restrict__ v = a.v[ti] + off;
    const bool vec = opt_aligned(g) && opt_aligned(p16) && opt_aligned(p) && opt_aligned(m) && opt_aligned(v);
#pragma unroll
    for (int it = 0; it < kOptIters; ++it) {
        const int i = (it * kOptThreads + tid) * kOptVec;
        if (i >= nb) break;
        float gx[kOptVec], px[kOptVec], mx[kOptVec], vx[kOptVec];
        opt_load4(g, i, nb, vec, gx);
        opt_load4(p, i, nb, vec, px);
        opt_load4(m, i, nb, vec, mx);
        opt_load4(v, i, nb, vec, vx);
#pragma unroll
        for (int k = 0; k < kOptVec; ++k) {
            const float gs = gx[k] * factor;
            const float mn = fmaf(a.omb1, gs - mx[k], mx[k]);                     // m + (1 - b1) (g' - m)
            const float vn = fmaf(a.b2, vx[k], (a.omb2 * gs) * gs);               // b2 v + (1 - b2) g'^2
            const float denom = sqrtf(vn) / bc2s + a.eps;
            px[k] = fmaf(-step_size, mn / denom, px[k] * a.decay);               // p (1 - lr wd) - (lr / bc1) m' / denom
            mx[k] = mn;
            vx[k] = vn;
        }
        opt_store4(p, i, nb, vec, px);
        if constexpr (kMaster) opt_store4(p16, i, nb, vec, px);
        opt_store4(m, i, nb, vec, mx);
        opt_store4(v, i, nb, vec, vx);
    }
}

static OptArgs opt_args(const vivim_opt_step_params& q, const void* masters = nullptr) {
    OptArgs a;
    a.first_tensor = q.first_tensor;
    a.count = q.count;
    a.first_block = q.first_block;
    a.scaled = q.scaled;
    a.p = static_cast<void* const*>(q.params);
    a.m = static_cast<float* const*>(q.exp_avg);
    a.v = static_cast<float* const*>(q.exp_avg_sq);
    a.w = static_cast<float* const*>(masters);
    a.block_map = static_cast<const int32_t*>(q.block_map);
    a.state = static_cast<uint32_t*>(q.state);
    a.workspace = static_cast<float*>(q.workspace);
    a.lr = (float)q.lr;                                     // each constant is formed in double and rounded once
    a.omb1 = (float)(1.0 - q.beta1);
    a.b2 = (float)q.beta2;
    a.omb2 = (float)(1.0 - q.beta2);
    a.eps = (float)q.eps;
    a.decay = (float)(1.0 - q.lr * q.weight_decay);
    for (int i = 0; i < VIVIM_OPT_MAX_TENSORS; ++i) {
        a.g[i] = i < q.count ? q.grads[i] : nullptr;
        a.n[i] = i < q.count ? q.numel[i] : 0;
    }
    return a;
}

static void opt_grad_stats_launch(const vivim_opt_step_params& q, hipStream_t stream) {
    hipLaunchKernelGGL(opt_grad_stats_kernel<float>, dim3((unsigned)q.n_blocks), dim3(kOptThreads), 0, stream, opt_args(q));
}

static void opt_adamw_launch(const vivim_opt_step_params& q, hipStream_t stream) {
    hipLaunchKernelGGL(opt_adamw_kernel<float>, dim3((unsigned)q.n_blocks), dim3(kOptThreads), 0, stream, opt_args(q));
}

// dtype: VIVIM_F16 or VIVIM_BF16 (checked by the caller)
static void opt_grad_stats_mw_launch(const vivim_opt_step_params& q, int dtype, hipStream_t stream) {
    const dim3 grid((unsigned)q.n_blocks), block(kOptThreads);
    if (dtype == VIVIM_F16) hipLaunchKernelGGL(opt_grad_stats_kernel<f16_t>, grid, block, 0, stream, opt_args(q));
    else hipLaunchKernelGGL(opt_grad_stats_kernel<bf16_t>, grid, block, 0, stream, opt_args(q));
}

static void opt_adamw_mw_launch(const vivim_opt_step_params& q, const void* masters, int dtype, hipStream_t stream) {
    const dim3 grid((unsigned)q.n_blocks), block(kOptThreads);
    if (dtype == VIVIM_F16) hipLaunchKernelGGL(opt_adamw_kernel<f16_t>, grid, block, 0, stream, opt_args(q, masters));
    else hipLaunchKernelGGL(opt_adamw_kernel<bf16_t>, grid, block, 0, stream, opt_args(q, masters));
}

static void opt_finalise_launch(const vivim_opt_step_params& q, hipStream_t stream) {
    OptFinArgs a;
    a.state = static_cast<uint32_t*>(q.state);
    a.workspace = static_cast<const float*>(q.workspace);
    a.total_blocks = q.total_blocks;
    a.scaled = q.scaled;
    a.has_max_norm = q.has_max_norm;
    a._pad = 0;
    a.max_norm = q.max_norm;
    a.beta1 = q.beta1;
    a.beta2 = q.beta2;
    hipLaunchKernelGGL(opt_finalise_kernel, dim3(1), dim3(kOptThreads), 0, stream, a);
}

}  // namespace vivim

// ---- the C entry points
static int check_opt_common(const vivim_opt_step_params* p, const char* fn) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_opt_step_params", p->struct_bytes, sizeof(*p))) return rc;
    VCHECK(p->state != nullptr && aligned(p->state, 4));
    if (p->total_blocks < 0) return fail(VIVIM_ERR_INVALID, "%s: total_blocks = %d", fn, p->total_blocks);
    return VIVIM_OK;
}

// the tensors and map rows of one multi-tensor call
static int check_opt_tensors(const vivim_opt_step_params* p, const char* fn, size_t grad_align = 4) {
    if (p->count <= 0 || p->count > VIVIM_OPT_MAX_TENSORS)
        return fail(VIVIM_ERR_INVALID, "%s: count = %d, a call takes 1 to %d tensors", fn, p->count, VIVIM_OPT_MAX_TENSORS);
    VCHECK(p->grads != nullptr && p->numel != nullptr && p->block_map != nullptr);
    VCHECK(aligned(p->block_map, 4) && p->first_tensor >= 0);
    for (int i = 0; i < p->count; ++i) {
        if (p->numel[i] <= 0) return fail(VIVIM_ERR_INVALID, "%s: numel[%d] = %lld", fn, i, (long long)p->numel[i]);
        VCHECK(aligned(p->grads[i], grad_align));
    }
    if (p->first_block < 0 || p->n_blocks <= 0 || (int64_t)p->first_block + p->n_blocks > p->total_blocks)
        return fail(VIVIM_ERR_INVALID, "%s: map rows %d .. %d + %d of %d", fn, p->first_block, p->first_block, p->n_blocks, p->total_blocks);
    return VIVIM_OK;
}

static int check_opt_workspace(const vivim_opt_step_params* p, const char* fn) {
    const size_t need = 8 * (size_t)p->total_blocks;
    if (need && (p->workspace == nullptr || !aligned(p->workspace, 8) || p->workspace_bytes < (int64_t)need))
        return bad_workspace(fn, "vivim_opt_step_workspace_bytes", (long long)p->workspace_bytes, p->workspace, 8, need);
    return VIVIM_OK;
}

// the hyper-parameters of a step: the betas, and for the `update` itself lr, eps and weight_decay
static int check_opt_hyper(const vivim_opt_step_params* p, const char* fn, bool update) {
    if (!(p->beta1 >= 0.0 && p->beta1 < 1.0 && p->beta2 >= 0.0 && p->beta2 < 1.0))
        return fail(VIVIM_ERR_INVALID, "%s: betas = (%g, %g), each must be in [0, 1)", fn, p->beta1, p->beta2);
    if (update && !(p->lr >= 0.0 && p->eps >= 0.0 && p->weight_decay >= 0.0))
        return fail(VIVIM_ERR_INVALID, "%s: lr = %g, eps = %g, weight_decay = %g: none may be negative", fn, p->lr, p->eps, p->weight_decay);
    return VIVIM_OK;
}

// the same step for 16-bit parameters with fp32 masters: vivim_opt_mw_params is vivim_opt_step_params + masters + dtype
static int check_opt_mw(const vivim_opt_mw_params* p, const char* fn, vivim_opt_step_params& q) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_opt_mw_params", p->struct_bytes, sizeof(*p))) return rc;
    static_assert(offsetof(vivim_opt_mw_params, masters) == sizeof(vivim_opt_step_params), "the common fields come first");
    memcpy(&q, p, sizeof(q));
    q.struct_bytes = (int32_t)sizeof(q);
    if (int rc = check_opt_common(&q, fn)) return rc;
    if (p->dtype != VIVIM_F16 && p->dtype != VIVIM_BF16)
        return fail(VIVIM_ERR_INVALID, "%s: dtype = %d, master weights are for 1 (fp16) and 2 (bf16)", fn, p->dtype);
    return VIVIM_OK;
}

extern "C" {

size_t vivim_opt_step_workspace_bytes(const vivim_opt_step_params* p) {
    return p && p->struct_bytes == (int32_t)sizeof(vivim_opt_step_params) && p->total_blocks > 0 ? 8 * (size_t)p->total_blocks : 0;
}

int vivim_opt_grad_stats(const vivim_opt_step_params* p, void* stream) {
    const char* fn = "opt_grad_stats";
    if (int rc = check_opt_common(p, fn)) return rc;
    if (int rc = check_opt_tensors(p, fn)) return rc;
    if (int rc = check_opt_workspace(p, fn)) return rc;
    vivim::opt_grad_stats_launch(*p, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_finalise(const vivim_opt_step_params* p, void* stream) {
    const char* fn = "opt_finalise";
    if (int rc = check_opt_common(p, fn)) return rc;
    if (int rc = check_opt_hyper(p, fn, false)) return rc;
    if (p->has_max_norm && !(p->max_norm >= 0.0)) return fail(VIVIM_ERR_INVALID, "%s: max_norm = %g", fn, p->max_norm);
    if (int rc = check_opt_workspace(p, fn)) return rc;
    vivim::opt_finalise_launch(*p, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_adamw(const vivim_opt_step_params* p, void* stream) {
    const char* fn = "opt_adamw";
    if (int rc = check_opt_common(p, fn)) return rc;
    VCHECK(p->params != nullptr && p->exp_avg != nullptr && p->exp_avg_sq != nullptr);
    VCHECK(aligned(p->params, 8) && aligned(p->exp_avg, 8) && aligned(p->exp_avg_sq, 8));
    if (int rc = check_opt_tensors(p, fn)) return rc;
    if (int rc = check_opt_hyper(p, fn, true)) return rc;
    vivim::opt_adamw_launch(*p, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_grad_stats_mw(const vivim_opt_mw_params* p, void* stream) {
    const char* fn = "opt_grad_stats_mw";
    vivim_opt_step_params q;
    if (int rc = check_opt_mw(p, fn, q)) return rc;
    if (int rc = check_opt_tensors(&q, fn, 2)) return rc;
    if (int rc = check_opt_workspace(&q, fn)) return rc;
    vivim::opt_grad_stats_mw_launch(q, p->dtype, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_adamw_mw(const vivim_opt_mw_params* p, void* stream) {
    const char* fn = "opt_adamw_mw";
    vivim_opt_step_params q;
    if (int rc = check_opt_mw(p, fn, q)) return rc;
    VCHECK(q.params != nullptr && q.exp_avg != nullptr && q.exp_avg_sq != nullptr && p->masters != nullptr);
    VCHECK(aligned(q.params, 8) && aligned(q.exp_avg, 8) && aligned(q.exp_avg_sq, 8) && aligned(p->masters, 8));
    if (int rc = check_opt_tensors(&q, fn, 2)) return rc;
    if (int rc = check_opt_hyper(&q, fn, true)) return rc;
    vivim::opt_adamw_mw_launch(q, p->masters, p->dtype, as_stream(stream));
    return after_launch(fn);
}

}  // extern "C"
