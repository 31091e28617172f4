// add_layernorm.hip -- the residual add of MambaLayer fused with the LayerNorm that follows it, forward and backward
// (include/vivim_hip.h: vivim_add_layernorm_params; the kernels of layernorm.hip with one more operand).
//
// The residual stream x is CHANNEL-major ((B, C, L) memory seen as (B, L, C)); a branch (out_proj of the Mamba block, fc2 of the
// Mlp) comes back TOKEN-major.  `x + drop_path(branch)` is then a DropPath multiply plus a mixed-layout strided add, and the norm
// reads the sum straight back from HBM.  Here the wave that owns a tile of TT tokens x all C channels (layernorm.hip: no workgroup
// barrier, 8-way XCD tile deal) reads x with 16-byte vectors along the tokens into its LDS tile, adds s[b] * branch read as 64
// consecutive channels of a token, rounds once to x's type IN the tile, writes x_new channel-major and y = LayerNorm(x_new as
// stored) token-major from it.  The backward needs no more LDS than layernorm.hip's two tiles: it computes dx in place of the dy
// tile while it sweeps channel-major (adding dres, the gradient that reaches x_new from later in the network, and writing dx),
// then writes the same tile out token-major as dbranch = s[b] * dx.  dweight / dbias: workspace rows + ln_reduce_kernel.
// Add-only mode (no weight): the forward stops after x_new, the backward is the scaled transposed copy of dres.
#include "layernorm.cuh"

namespace vivim {

// v as x's type will hold it.  The fp32 sum is a value of its own (the empty asm): left alone, hipcc folds the f16 case into
// v_fma_mixlo_f16, which rounds the exact fma straight to f16 -- one ulp away from "fp32, then x's type" (what torch's adds and
// the bf16 path give) wherever the fp32 sum lands on an f16 midpoint, 3.4 % of the elements at s = 4 / 3.
template <typename T> __device__ __forceinline__ float aln_round(float v) {
    asm volatile("" : "+v"(v));
    return to_f32<T>(from_f32<T>(v));
}
template <> __device__ __forceinline__ float aln_round<float>(float v) { return v; }

// f(channel, token of the tile, value) for every element of the tile, read token-major: 64 consecutive channels of a token per
// instruction, eight in flight; tokens beyond the row's end (>= nt) come as 0
template <typename T, int TT, typename F>
__device__ __forceinline__ void aln_read_tm(const T* __restrict__ base, int64_t token_stride, int C, int nt, int lane, F&& f) {
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
__device__ __forceinline__ void aln_write_tm(T* __restrict__ base, int64_t token_stride, int C, int nt, int lane, F&& f) {
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

// TI: x / x_new, TB: branch, TO: y.  NORM = false: the add alone.
template <typename TI, typename TB, typename TO, int TT, bool NORM>
__global__ void __launch_bounds__(kWave) add_ln_fwd_kernel(const vivim_add_layernorm_params p, const int ntiles, const int tpb) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    constexpr int PAD = TT + 1, P = kWave / TT;
    const int C = p.channels, L = p.seqlen, lane = threadIdx.x;
    int b, t0;
    if (!ln_tile(ntiles, tpb, TT, b, t0)) return;
    float* tile = ln_smem;                             // [C][TT + 1]
    float* stat = tile + C * PAD;                      // [2][TT]: mean, rstd
    float* gb = stat + 2 * TT;                         // [2][C]: weight, bias
    if (NORM) {
        for (int c = lane; c < C; c += kWave) {
            gb[c] = static_cast<const float*>(p.weight)[c];
            gb[C + c] = p.bias ? static_cast<const float*>(p.bias)[c] : 0.0f;
        }
    }
    const float s = p.scale ? static_cast<const float*>(p.scale)[b] : 1.0f;
    const int nt = min(TT, L - t0);
    ln_load_cm<TI, TT>(tile, static_cast<const TI*>(p.x) + (int64_t)b * p.x_batch_stride, p.x_c_stride, C, t0, L, lane);
    wave_lds_fence();
    // x_new = x + s * branch: one fma in f32, rounded once to x's type; the tile holds x_new as it will be stored
    aln_read_tm<TB, TT>(static_cast<const TB*>(p.branch) + (int64_t)b * p.branch_batch_stride + (int64_t)t0 * p.branch_token_stride,
                        p.branch_token_stride, C, nt, lane, [&](int c, int tt, float v) {
                            float* q = tile + c * PAD + tt;
                            *q = aln_round<TI>(fmaf(s, v, *q));
                        });
    wave_lds_fence();
    {   // x_new: channel-major, 16-byte vectors along the tokens
        constexpr int E = LnVec<TI>::E;
        constexpr int VPR = TT / E;
        TI* __restrict__ xnb = static_cast<TI*>(p.x_new) + (int64_t)b * p.x_new_batch_stride;
        const int nvec = C * VPR;
        for (int idx = lane; idx < nvec; idx += kWave) {
            const int c = idx / VPR, v = idx - c * VPR;
            const int tg = t0 + v * E;
            if (tg >= L) continue;
            typename LnVec<TI>::U u;
#pragma unroll
            for (int e = 0; e < E; ++e) u.e[e] = from_f32<TI>(tile[c * PAD + v * E + e]);
            *reinterpret_cast<typename LnVec<TI>::vec*>(xnb + (int64_t)c * p.x_new_c_stride + tg) = u.v;
        }
    }
    if (!NORM) return;
    const int t = lane % TT, part = lane / TT;
    const float pivot = tile[t];                       // channel 0 of the token
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll 8
    for (int c = part; c < C; c += P) {
        const float d = tile[c * PAD + t] - pivot;
        s1 += d;
        s2 = fmaf(d, d, s2);
    }
    s1 = ln_parts_sum<TT>(s1);
    s2 = ln_parts_sum<TT>(s2);
    const float inv_c = 1.0f / (float)C;
    const float m = s1 * inv_c;
    const float mean = pivot + m;
    const float rstd = rsqrtf(fmaxf(s2 * inv_c - m * m, 0.0f) + p.eps);
    if (part == 0) {
        stat[t] = mean;
        stat[TT + t] = rstd;
        if (t0 + t < L) {
            static_cast<float*>(p.mean)[(int64_t)b * L + t0 + t] = mean;
            static_cast<float*>(p.rstd)[(int64_t)b * L + t0 + t] = rstd;
        }
    }
    wave_lds_fence();
    aln_write_tm<TO>(static_cast<TO*>(p.y) + (int64_t)b * p.y_batch_stride + (int64_t)t0 * p.y_token_stride, p.y_token_stride, C, nt, lane,
                     [&](int c, int tt) { return (tile[c * PAD + tt] - stat[tt]) * stat[TT + tt] * gb[c] + gb[C + c]; });
}

template <typename TI, typename TB, typename TO, int TT>
__global__ void __launch_bounds__(kWave) add_ln_bwd_kernel(const vivim_add_layernorm_params p, const int ntiles, const int tpb) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    constexpr int PAD = TT + 1, P = kWave / TT;
    const int C = p.channels, L = p.seqlen, lane = threadIdx.x;
    int b, t0;
    if (!ln_tile(ntiles, tpb, TT, b, t0)) return;
    const int tile_id = b * tpb + t0 / TT;
    float* xt = ln_smem;                               // [C][TT + 1]: x_new
    float* gt = xt + C * PAD;                          // [C][TT + 1]: dy, then dx
    float* stat = gt + C * PAD;                        // [4][TT]: mean, rstd, S1 / C, S2 / C
    float* gam = stat + 4 * TT;                        // [C]: weight
    const int nt = min(TT, L - t0);
    for (int c = lane; c < C; c += kWave) gam[c] = static_cast<const float*>(p.weight)[c];
    if (p.dy) {
        aln_read_tm<TO, TT>(static_cast<const TO*>(p.dy) + (int64_t)b * p.y_batch_stride + (int64_t)t0 * p.y_token_stride, p.y_token_stride,
                            C, nt, lane, [&](int c, int tt, float v) { gt[c * PAD + tt] = v; });
    } else {
        for (int i = lane; i < C * PAD; i += kWave) gt[i] = 0.0f;
    }
    ln_load_cm<TI, TT>(xt, static_cast<const TI*>(p.x_new) + (int64_t)b * p.x_new_batch_stride, p.x_new_c_stride, C, t0, L, lane);
    const int t = lane % TT, part = lane / TT;
    const bool tok = t0 + t < L;
    const float mean = tok ? static_cast<const float*>(p.mean)[(int64_t)b * L + t0 + t] : 0.0f;
    const float rstd = tok ? static_cast<const float*>(p.rstd)[(int64_t)b * L + t0 + t] : 0.0f;
    const float s = p.scale ? static_cast<const float*>(p.scale)[b] : 1.0f;
    wave_lds_fence();
    // per-token S1 = sum_c dy gamma, S2 = sum_c dy gamma xhat
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll 8
    for (int c = part; c < C; c += P) {
        const float g = gt[c * PAD + t] * gam[c];
        s1 += g;
        s2 = fmaf(g, (xt[c * PAD + t] - mean) * rstd, s2);
    }
    s1 = ln_parts_sum<TT>(s1);
    s2 = ln_parts_sum<TT>(s2);
    const float inv_c = 1.0f / (float)C;
    if (part == 0) {
        stat[t] = mean;
        stat[TT + t] = rstd;                           // 0 for a token beyond the row: its xhat and dx vanish
        stat[2 * TT + t] = s1 * inv_c;
        stat[3 * TT + t] = s2 * inv_c;
    }
    wave_lds_fence();
    // dweight, dbias partials of this tile: lane = channel, sum over the tile's tokens; row tile_id of the workspace
    if (p.workspace) {
        float* __restrict__ row = static_cast<float*>(p.workspace) + (int64_t)tile_id * 2 * C;
        for (int c = lane; c < C; c += kWave) {
            float dw = 0.0f, db = 0.0f;
#pragma unroll
            for (int k = 0; k < TT; ++k) {
                const float g = gt[c * PAD + k];
                dw = fmaf(g, (xt[c * PAD + k] - stat[k]) * stat[TT + k], dw);
                db += g;
            }
            row[c] = dw;
            row[C + c] = db;
        }
        wave_lds_fence();                              // the sweep below overwrites the dy tile
    }
    // dx = rstd * (dy gamma - S1 / C - xhat S2 / C) + dres, channel-major with 16-byte vectors along the tokens (eight dres
    // vectors per lane in flight); the f32 value replaces dy in the tile for the token-major pass below
    constexpr int E = LnVec<TI>::E;
    constexpr int VPR = TT / E;
    TI* __restrict__ dxb = static_cast<TI*>(p.dx) + (int64_t)b * p.dx_batch_stride;
    const TI* __restrict__ drb = static_cast<const TI*>(p.dres) + (int64_t)b * p.dres_batch_stride;
    const bool has_res = p.dres != nullptr;
    const int nvec = C * VPR;
    for (int base = 0; base < nvec; base += kWave * 8) {
        typename LnVec<TI>::U r8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = base + i * kWave + lane;
            const int c = idx / VPR, v = idx - c * VPR;
            const int tg = t0 + v * E;
            r8[i].v = typename LnVec<TI>::vec{0u, 0u, 0u, 0u};
            if (has_res && idx < nvec && tg < L) r8[i].v = *reinterpret_cast<const typename LnVec<TI>::vec*>(drb + (int64_t)c * p.dres_c_stride + tg);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = base + i * kWave + lane;
            const int c = idx / VPR, v = idx - c * VPR;
            const int tg = t0 + v * E;
            if (idx >= nvec || tg >= L) continue;
            const float g = gam[c];
            typename LnVec<TI>::U u;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = v * E + e;
                const float r = stat[TT + k];
                const float xh = (xt[c * PAD + k] - stat[k]) * r;
                const float d = r * (gt[c * PAD + k] * g - stat[2 * TT + k] - xh * stat[3 * TT + k]) + to_f32<TI>(r8[i].e[e]);
                gt[c * PAD + k] = d;
                u.e[e] = from_f32<TI>(d);
            }
            *reinterpret_cast<typename LnVec<TI>::vec*>(dxb + (int64_t)c * p.dx_c_stride + tg) = u.v;
        }
    }
    if (!p.dbranch) return;
    wave_lds_fence();
    aln_write_tm<TB>(static_cast<TB*>(p.dbranch) + (int64_t)b * p.dbranch_batch_stride + (int64_t)t0 * p.dbranch_token_stride,
                     p.dbranch_token_stride, C, nt, lane, [&](int c, int tt) { return s * gt[c * PAD + tt]; });
}

// add-only backward: dbranch[b][t][c] = s[b] * dres[b][c][t]
template <typename TI, typename TB, int TT>
__global__ void __launch_bounds__(kWave) add_cm_bwd_kernel(const vivim_add_layernorm_params p, const int ntiles, const int tpb) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    constexpr int PAD = TT + 1;
    const int C = p.channels, L = p.seqlen, lane = threadIdx.x;
    int b, t0;
    if (!ln_tile(ntiles, tpb, TT, b, t0)) return;
    float* tile = ln_smem;                             // [C][TT + 1]
    const float s = p.scale ? static_cast<const float*>(p.scale)[b] : 1.0f;
    ln_load_cm<TI, TT>(tile, static_cast<const TI*>(p.dres) + (int64_t)b * p.dres_batch_stride, p.dres_c_stride, C, t0, L, lane);
    wave_lds_fence();
    aln_write_tm<TB>(static_cast<TB*>(p.dbranch) + (int64_t)b * p.dbranch_batch_stride + (int64_t)t0 * p.dbranch_token_stride,
                     p.dbranch_token_stride, C, min(TT, L - t0), lane, [&](int c, int tt) { return s * tile[c * PAD + tt]; });
}

static vivim_layernorm_params aln_shape(const vivim_add_layernorm_params& p) {
    vivim_layernorm_params q = {};
    q.batch = p.batch; q.seqlen = p.seqlen; q.channels = p.channels; q.itype = p.itype; q.otype = p.otype;
    return q;
}
// the tile choice and the workspace rows of layernorm.hip, so that VIVIM_LN_TT and the thresholds hold for both
size_t add_layernorm_bwd_workspace_bytes(const vivim_add_layernorm_params& p) {
    const int TT = layernorm_tile_tokens(aln_shape(p));
    return (size_t)p.batch * ((p.seqlen + TT - 1) / TT) * 2 * p.channels * sizeof(float);
}

template <typename TI, typename TB, typename TO, int TT>
static void aln_launch_tt(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    const int tpb = (p.seqlen + TT - 1) / TT, ntiles = p.batch * tpb;
    const dim3 grid((unsigned)((ntiles + 7) / 8 * 8)), block(kWave);
    if (!bwd) {
        hipLaunchKernelGGL((add_ln_fwd_kernel<TI, TB, TO, TT, true>), grid, block, ln_fwd_smem(p.channels, TT), stream, p, ntiles, tpb);
        return;
    }
    hipLaunchKernelGGL((add_ln_bwd_kernel<TI, TB, TO, TT>), grid, block, ln_bwd_smem(p.channels, TT), stream, p, ntiles, tpb);
    if (p.workspace && (p.dweight || p.dbias))
        ln_reduce_launch(static_cast<const float*>(p.workspace), ntiles, p.channels, static_cast<float*>(p.dweight),
                         static_cast<float*>(p.dbias), stream);
}
template <typename TI, typename TB, int TT>
static void aln_add_launch_tt(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    const int tpb = (p.seqlen + TT - 1) / TT, ntiles = p.batch * tpb;
    const dim3 grid((unsigned)((ntiles + 7) / 8 * 8)), block(kWave);
    const size_t smem = (size_t)p.channels * (TT + 1) * sizeof(float);
    if (!bwd) hipLaunchKernelGGL((add_ln_fwd_kernel<TI, TB, TI, TT, false>), grid, block, smem, stream, p, ntiles, tpb);
    else hipLaunchKernelGGL((add_cm_bwd_kernel<TI, TB, TT>), grid, block, smem, stream, p, ntiles, tpb);
}

template <typename TI, typename TB, typename TO>
static void aln_launch(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    switch (layernorm_tile_tokens(aln_shape(p))) {
        case 32: aln_launch_tt<TI, TB, TO, 32>(p, bwd, stream); break;
        case 16: aln_launch_tt<TI, TB, TO, 16>(p, bwd, stream); break;
        default: aln_launch_tt<TI, TB, TO, 8>(p, bwd, stream); break;
    }
}
template <typename TI, typename TB>
static bool aln_pair(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    if (!p.weight) {                                   // add-only: no y, its type does not matter
        switch (layernorm_tile_tokens(aln_shape(p))) {
            case 32: aln_add_launch_tt<TI, TB, 32>(p, bwd, stream); break;
            case 16: aln_add_launch_tt<TI, TB, 16>(p, bwd, stream); break;
            default: aln_add_launch_tt<TI, TB, 8>(p, bwd, stream); break;
        }
        return true;
    }
    // the output / incoming-gradient side is f32 (what autocast makes of layer_norm) or the input's own type
    if (p.otype == VIVIM_F32) { aln_launch<TI, TB, float>(p, bwd, stream); return true; }
    if (p.otype == p.itype) { aln_launch<TI, TB, TI>(p, bwd, stream); return true; }
    return false;
}

bool add_layernorm_dispatch(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    if (p.channels > kLnMaxC) return false;
    if (p.btype == p.itype) {
        switch (p.itype) {
            case VIVIM_F32: return aln_pair<float, float>(p, bwd, stream);
            case VIVIM_F16: return aln_pair<f16_t, f16_t>(p, bwd, stream);
            case VIVIM_BF16: return aln_pair<bf16_t, bf16_t>(p, bwd, stream);
        }
    } else if (p.itype == VIVIM_F32) {                 // an f32 residual stream with an autocast branch
        switch (p.btype) {
            case VIVIM_F16: return aln_pair<float, f16_t>(p, bwd, stream);
            case VIVIM_BF16: return aln_pair<float, bf16_t>(p, bwd, stream);
        }
    }
    return false;
}

}  // namespace vivim
