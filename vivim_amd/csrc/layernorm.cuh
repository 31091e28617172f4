// layernorm.cuh -- what the channel-major LayerNorm kernels (layernorm.hip) and their residual-add variants
// (add_layernorm.hip) share: the tile deal over the XCDs, the channel-major tile load, the per-token sum, the LDS sizes and
// the host-side tile choice.
#pragma once
#include "common.cuh"

namespace vivim {

constexpr int kLnMaxC = 512;         // backward: 2 tiles x 512 channels x 9 floats = 37 KB of LDS per wave at TT = 8

template <typename T> struct LnVec {
    static constexpr int E = 16 / (int)sizeof(T);
    typedef typename Pack<T, 16>::type vec;
    union U { vec v; T e[16 / sizeof(T)]; };
};

// Which tile this wave (= workgroup) works on.  Workgroups are dealt round-robin over the 8 XCDs: XCD k takes the k-th eighth
// of the tiles, in order.
__device__ __forceinline__ bool ln_tile(int ntiles, int tpb, int TT, int& b, int& t0) {
    const int per = (ntiles + 7) / 8;
    const int tile = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
    if ((int)(blockIdx.x / 8) >= per || tile >= ntiles) return false;
    b = tile / tpb;
    t0 = (tile - b * tpb) * TT;
    return true;
}

// tile[c][t] <- x[b][c][t0 + t] as f32 (zero beyond the row's end); seqlen % E == 0 (host check).  Eight vectors per lane are
// in flight before the first LDS write.
template <typename T, int TT>
__device__ __forceinline__ void ln_load_cm(float* tile, const T* __restrict__ xb, int64_t c_stride, int C, int t0, int L, int lane) {
    constexpr int E = LnVec<T>::E;
    constexpr int VPR = TT / E;                        // 16-byte vectors per channel piece
    constexpr int PAD = TT + 1;
    const int nvec = C * VPR;
    for (int base = 0; base < nvec; base += 64 * 8) {
        typename LnVec<T>::U u[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = base + i * 64 + lane;
            const int c = idx / VPR, v = idx - c * VPR;
            const int t = t0 + v * E;
            if (idx < nvec && t < L) u[i].v = *reinterpret_cast<const typename LnVec<T>::vec*>(xb + (int64_t)c * c_stride + t);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = base + i * 64 + lane;
            const int c = idx / VPR, v = idx - c * VPR;
            const bool ok = t0 + v * E < L;
            if (idx < nvec) {
#pragma unroll
                for (int e = 0; e < E; ++e) tile[c * PAD + v * E + e] = ok ? to_f32<T>(u[i].e[e]) : 0.0f;
            }
        }
    }
}

// sum over the 64 / TT channel parts of a token (lanes t, t + TT, t + 2 TT, ...)
template <int TT>
__device__ __forceinline__ float ln_parts_sum(float v) {
#pragma unroll
    for (int off = TT; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

static inline size_t ln_fwd_smem(int C, int TT) { return ((size_t)C * (TT + 1) + 2 * TT + 2 * C) * sizeof(float); }
static inline size_t ln_bwd_smem(int C, int TT) { return ((size_t)2 * C * (TT + 1) + 4 * TT + C) * sizeof(float); }

// layernorm.hip
int layernorm_tile_tokens(const vivim_layernorm_params& p);       // from batch, seqlen, channels, itype (and VIVIM_LN_TT)
void ln_reduce_launch(const float* ws, int ntiles, int C, float* dweight, float* dbias, hipStream_t stream);

}  // namespace vivim
