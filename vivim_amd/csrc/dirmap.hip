// dirmap.hip -- the v3 block's three scan directions as index maps (include/vivim_hip.h: vivim_dir_params).
//
// scatter: one read of the (batch, channels, seqlen) tensor, three writes into the stacked
//          (batch, halves, 3, csplit, seqlen) tensor the grouped fused op consumes;
// gather : three reads of the stacked tensor, one write -- the (out + out_b.flip + out_s^-1) / 3 combination of
//          mamba_simple.py:261-264 and, with scale 1, the gradient of scatter.
// A thread owns one 16-byte vector of consecutive tokens on the FLAT side (coalesced there); on the stacked side
// direction 0 is the same vector, direction 1 the mirrored vector with its elements reversed (still one 16-byte
// access), direction 2 (frame interleave, token t*hw+p <-> p*nf+t) is element-wise: consecutive flat tokens are
// nf elements apart there, the lines are shared between neighbouring threads and served by L2.
// Pure data movement: HBM-bound, algorithmic bytes 4 * batch * channels * seqlen * sizeof(T) either way.
#include "capi.cuh"

namespace vivim {

template <typename T, bool GATHER>
__global__ void __launch_bounds__(256) dir_kernel(const vivim_dir_params p) {
    constexpr int E = 16 / (int)sizeof(T);
    typedef typename Pack<T, 16>::type vec;
    const int L = p.seqlen, nf = p.nframes, hw = L / nf;
    const int l0 = (blockIdx.x * 256 + threadIdx.x) * E;
    if (l0 >= L) return;                               // L % E == 0 (host)
    const int c = blockIdx.y, b = blockIdx.z;
    const int64_t stk = (int64_t)b * p.stk_batch_stride + (int64_t)(c / p.csplit) * p.stk_half_stride +
                        (int64_t)(c % p.csplit) * p.stk_c_stride;
    const int64_t flat = (int64_t)b * p.flat_batch_stride + (int64_t)c * p.flat_c_stride + l0;
    const float scale = p.scale;
    union U { vec v; T e[E]; };
    if (GATHER) {
        const T* __restrict__ s = static_cast<const T*>(p.src) + stk;
        U a0, a1, r;
        a0.v = *reinterpret_cast<const vec*>(s + l0);
        a1.v = *reinterpret_cast<const vec*>(s + p.stk_dir_stride + (L - E - l0));
        const T* __restrict__ s2 = s + 2 * p.stk_dir_stride;
        int t = l0 / hw, q = l0 - t * hw;              // flat token l0 + j = t*hw + q
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const float v2 = to_f32<T>(s2[(int64_t)q * nf + t]);
            r.e[j] = from_f32<T>((to_f32<T>(a0.e[j]) + to_f32<T>(a1.e[E - 1 - j]) + v2) * scale);
            if (++q == hw) { q = 0; ++t; }
        }
        *reinterpret_cast<vec*>(static_cast<T*>(p.dst) + flat) = r.v;
    } else {
        U a, o0, o1;
        a.v = *reinterpret_cast<const vec*>(static_cast<const T*>(p.src) + flat);
        T* __restrict__ d = static_cast<T*>(p.dst) + stk;
        T* __restrict__ d2 = d + 2 * p.stk_dir_stride;
        int t = l0 / hw, q = l0 - t * hw;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const T v = from_f32<T>(to_f32<T>(a.e[j]) * scale);
            o0.e[j] = v;
            o1.e[E - 1 - j] = v;
            d2[(int64_t)q * nf + t] = v;
            if (++q == hw) { q = 0; ++t; }
        }
        *reinterpret_cast<vec*>(d + l0) = o0.v;
        *reinterpret_cast<vec*>(d + p.stk_dir_stride + (L - E - l0)) = o1.v;
    }
}

// The same maps with the frame interleave transposed through LDS: a workgroup owns Q pixel positions of ALL frames of one
// (batch, channel) -- nf contiguous Q-token pieces on the flat side, ONE contiguous nf*Q-token piece on the interleaved
// side -- so direction 2 is written (read) with whole 16-byte vectors too.  The element-wise kernel above issued E two-byte
// stores per thread into lines that four other workgroups complete (30.8 us per launch in the bench, 16 launches per
// step: half the time of all forward scans).  Needs hw % E == 0 (vectors of a frame's piece stay aligned) and nf <= 16.
constexpr int kDirMaxFrames = 16;
template <typename T, bool GATHER>
__global__ void __launch_bounds__(256) dir_tile_kernel(const vivim_dir_params p) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int Q = 64 * E;                          // pixel positions per workgroup: 64 vectors per frame
    typedef typename Pack<T, 16>::type vec;
    __shared__ __attribute__((aligned(16))) T lds[kDirMaxFrames * Q];
    const int L = p.seqlen, nf = p.nframes, hw = L / nf;
    const int q0 = blockIdx.x * Q, c = blockIdx.y, b = blockIdx.z;
    const int qn = min(Q, hw - q0);                    // % E == 0
    const int64_t stk = (int64_t)b * p.stk_batch_stride + (int64_t)(c / p.csplit) * p.stk_half_stride +
                        (int64_t)(c % p.csplit) * p.stk_c_stride;
    const int64_t flat = (int64_t)b * p.flat_batch_stride + (int64_t)c * p.flat_c_stride;
    const float scale = p.scale;
    const int vpf = qn / E;                            // vectors per frame piece
    union U { vec v; T e[E]; };
    if (GATHER) {
        const T* __restrict__ s = static_cast<const T*>(p.src) + stk;
        const T* __restrict__ s2 = s + 2 * p.stk_dir_stride + (int64_t)q0 * nf;
        for (int j = threadIdx.x; j < vpf * nf; j += 256) {               // the interleaved piece, vector by vector
            U a;
            a.v = *reinterpret_cast<const vec*>(s2 + j * E);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int idx = j * E + e, q = idx / nf, t = idx - q * nf;
                lds[t * Q + q] = a.e[e];
            }
        }
        __syncthreads();
        T* __restrict__ d = static_cast<T*>(p.dst) + flat;
        for (int i = threadIdx.x; i < vpf * nf; i += 256) {
            const int t = i / vpf, v = i - t * vpf;
            const int l0 = t * hw + q0 + v * E;
            U a0, a1, a2, r;
            a2.v = *reinterpret_cast<const vec*>(lds + t * Q + v * E);
            a0.v = *reinterpret_cast<const vec*>(s + l0);
            a1.v = *reinterpret_cast<const vec*>(s + p.stk_dir_stride + (L - E - l0));
#pragma unroll
            for (int e = 0; e < E; ++e)
                r.e[e] = from_f32<T>((to_f32<T>(a0.e[e]) + to_f32<T>(a1.e[E - 1 - e]) + to_f32<T>(a2.e[e])) * scale);
            *reinterpret_cast<vec*>(d + l0) = r.v;
        }
    } else {
        const T* __restrict__ sflat = static_cast<const T*>(p.src) + flat;
        T* __restrict__ d = static_cast<T*>(p.dst) + stk;
        for (int i = threadIdx.x; i < vpf * nf; i += 256) {
            const int t = i / vpf, v = i - t * vpf;
            const int l0 = t * hw + q0 + v * E;
            U a, o0, o1;
            a.v = *reinterpret_cast<const vec*>(sflat + l0);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const T x = from_f32<T>(to_f32<T>(a.e[e]) * scale);
                o0.e[e] = x;
                o1.e[E - 1 - e] = x;
            }
            *reinterpret_cast<vec*>(d + l0) = o0.v;
            *reinterpret_cast<vec*>(d + p.stk_dir_stride + (L - E - l0)) = o1.v;
            *reinterpret_cast<vec*>(lds + t * Q + v * E) = o0.v;
        }
        __syncthreads();
        T* __restrict__ d2 = d + 2 * p.stk_dir_stride + (int64_t)q0 * nf;
        for (int j = threadIdx.x; j < vpf * nf; j += 256) {
            U o;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int idx = j * E + e, q = idx / nf, t = idx - q * nf;
                o.e[e] = lds[t * Q + q];
            }
            *reinterpret_cast<vec*>(d2 + j * E) = o.v;
        }
    }
}

template <bool GATHER>
static bool dir_dispatch(const vivim_dir_params& p, hipStream_t stream) {
    const int E = vec_elems(p.itype);
    const int hw = p.seqlen / p.nframes;
    if (hw % E == 0 && p.nframes <= kDirMaxFrames && p.nframes > 1) {
        const dim3 grid((hw + 64 * E - 1) / (64 * E), p.channels, p.batch), block(256);
        return with_itype(p.itype, [&](auto t) {
            hipLaunchKernelGGL((dir_tile_kernel<decltype(t), GATHER>), grid, block, 0, stream, p);
        });
    }
    const dim3 grid((p.seqlen / E + 255) / 256, p.channels, p.batch), block(256);
    return with_itype(p.itype, [&](auto t) { hipLaunchKernelGGL((dir_kernel<decltype(t), GATHER>), grid, block, 0, stream, p); });
}

}  // namespace vivim

// ---- the C entry points
static int check_dir(const vivim_dir_params* p) {
    VCHECK(p != nullptr);
    VCHECK(p->itype == VIVIM_F32 || p->itype == VIVIM_F16 || p->itype == VIVIM_BF16);
    VCHECK(p->batch > 0 && p->channels > 0 && p->seqlen > 0 && p->nframes > 0 && p->csplit > 0);
    VCHECK(p->batch <= 65535 && p->channels <= 65535);
    VCHECK(p->seqlen % p->nframes == 0 && p->channels % p->csplit == 0);
    VCHECK(p->src && p->dst);
    const int64_t e = vec_elems(p->itype);                      // 16-byte vectors on both sides
    VCHECK(p->seqlen % e == 0);
    VCHECK(aligned16(p->src) && aligned16(p->dst));
    VCHECK(p->flat_batch_stride % e == 0 && p->flat_c_stride % e == 0 && p->stk_batch_stride % e == 0 &&
           p->stk_half_stride % e == 0 && p->stk_dir_stride % e == 0 && p->stk_c_stride % e == 0);
    return VIVIM_OK;
}

extern "C" {

int vivim_dir_scatter(const vivim_dir_params* p, void* stream) {
    if (int rc = check_dir(p)) return rc;
    return after_dispatch(vivim::dir_dispatch<false>(*p, as_stream(stream)), "dir_scatter", "dir_scatter: bad itype");
}

int vivim_dir_gather(const vivim_dir_params* p, void* stream) {
    if (int rc = check_dir(p)) return rc;
    return after_dispatch(vivim::dir_dispatch<true>(*p, as_stream(stream)), "dir_gather", "dir_gather: bad itype");
}

}  // extern "C"
