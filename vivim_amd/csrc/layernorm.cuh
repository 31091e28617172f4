// layernorm.cuh -- the pieces the channel-major LayerNorm family (layernorm.hip: plain, residual-add + norm, add alone) is
// built from: the tile deal over the XCDs, the channel-major tile load, the token-major read and write, the rounding to x's
// type, the per-token sum and the LDS sizes.
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

// v as x's type will hold it.  The fp32 sum is a value of its own (the empty asm): left alone, hipcc folds the f16 case into
// v_fma_mixlo_f16, which rounds the exact fma straight to f16 -- one ulp away from "fp32, then x's type" (what torch's adds and
// the bf16 path give) wherever the fp32 sum lands on an f16 midpoint, 3.4 % of the elements at s = 4 / 3.
template <typename T> __device__ __forceinline__ float ln_round(float v) {
    asm volatile("" : "+v"(v));
    return to_f32<T>(from_f32<T>(v));
}
template <> __device__ __forceinline__ float ln_round<float>(float v) { return v; }

// f(channel, token of the tile, value) for every element of the tile, read token-major: 64 consecutive channels of a token per
// instruction, eight in flight; tokens beyond the row's end (>= nt) come as 0
template <typename T, int TT, typename F>
__device__ __forceinline__ void ln_read_tm(const T* __restrict__ base, int64_t token_stride, int C, int nt, int lane, F&& f) {
    int tt = 0, c = lane;
    while (c >= C) { c -= C; ++tt; }
    while (tt < TT) {
        float v[8];
        int ct[8], tk[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ct[i] = c; tk[i] = tt;
            v[i] = tt < nt ? to_f32<T>(base[(int64_t)tt * token_stride + c]) : 0.0f;
            c += kWave;
            while (c >= C) { c -= C; ++tt; }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (tk[i] < TT) f(ct[i], tk[i], v[i]);
    }
}

// out[tt][c] = f(channel, token) for the tile's nt tokens, written token-major: 64 consecutive channels of a token per instruction
template <typename T, typename F>
__device__ __forceinline__ void ln_write_tm(T* __restrict__ base, int64_t token_stride, int C, int nt, int lane, F&& f) {
    int tt = 0, c = lane;
    while (c >= C) { c -= C; ++tt; }
    const int iters = (nt * C + kWave - 1) / kWave;
#pragma unroll 4
    for (int k = 0; k < iters; ++k) {
        if (tt < nt) base[(int64_t)tt * token_stride + c] = from_f32<T>(f(c, tt));
        c += kWave;
        while (c >= C) { c -= C; ++tt; }
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

}  // namespace vivim
