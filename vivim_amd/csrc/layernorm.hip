// layernorm.hip -- LayerNorm over the channel axis of a CHANNEL-major token tensor, forward and backward (SURVEY.md 8f row 4:
// the two nn.LayerNorms around the Mamba call, modeling/vivim.py:155-156), and the same kernels with the residual add of
// MambaLayer in front of the norm (include/vivim_hip.h: vivim_add_layernorm_params).  One kernel family: ADD and NORM are
// template parameters, the plain LayerNorm is the instantiation without the add.
//
// MambaLayer holds its activations as (B, C, nf*H*W) and hands the norm the transposed VIEW (B, L, C) with strides
// (C*L, 1, L) (modeling/vivim.py:151-155).  The ATen path first makes that view contiguous (one full copy kernel) and then
// runs its row kernels; here the transpose IS the kernel.
//
// One WAVE owns a tile of TT tokens x all C channels of one batch element and nothing is shared between waves: no workgroup
// barrier anywhere (the first version of this file had six in the forward and eight in the backward and spent its time in
// them: 15-21 us for the 4-10 MB of stages 2 / 3).  The wave reads every channel's TT-token piece with 16-byte vectors
// (coalesced along the tokens), keeps the tile in its LDS as f32 [channel][TT + 1], takes the per-token sums with lanes =
// (token, channel part) -- two sweeps of the LDS tile: the mean around the token's first channel, then sum and sum of squares
// around that mean, so that neither a common shift nor an outlier channel cancels -- and writes the normalised rows token-major (coalesced along the channels) in the dtype autocast would give them.  The
// backward does the same in the other direction: dy arrives token-major, dx leaves channel-major (the layout of the
// residual stream it is added to).  dweight / dbias: the wave leaves its tile's partial sums as one row of a workspace and a
// second small kernel adds the rows up (two launches, no same-address atomic traffic from thousands of waves; the only
// atomics are one per row group of the reduce kernel, 128 groups at most).
// TT is 32, 16 or 8: the largest that still gives a couple of thousand waves and fits the LDS.  Waves are numbered so that the
// tiles an XCD works on are neighbours in memory (pieces shorter than a 128-byte line meet in one L2).
// HBM-bound: forward reads x once and writes y once; backward reads dy and x once and writes dx once.
//
// ADD: a branch (out_proj of the Mamba block, fc2 of the Mlp) comes back TOKEN-major, so `x + drop_path(branch)` is a DropPath
// multiply plus a mixed-layout strided add, and the norm reads the sum straight back from HBM.  Here the wave adds s[b] * branch,
// read as 64 consecutive channels of a token, to its tile of x, rounds once to x's type IN the tile, writes x_new channel-major
// and y = LayerNorm(x_new as stored) from it.  The backward needs no more LDS than the plain one's two tiles: it computes dx in
// place of the dy tile while it sweeps channel-major (adding dres, the gradient that reaches x_new from later in the network,
// and writing dx), then writes the same tile out token-major as dbranch = s[b] * dx.
// Add-only mode (no weight, NORM = false): the forward stops after x_new, the backward is the scaled transposed copy of dres.
#include "layernorm.cuh"
#include "capi.cuh"

namespace vivim {

// TI: x / x_new, TB: branch, TO: y.  ADD = false: the plain LayerNorm of x (the host passes it as vivim_add_layernorm_params
// with x_new = x; TB is TI).  NORM = false: the add alone.
template <typename TI, typename TB, typename TO, int TT, bool ADD, bool NORM>
__global__ void __launch_bounds__(kWave) ln_cm_fwd_kernel(const vivim_add_layernorm_params p, const int ntiles, const int tpb) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    constexpr int PAD = TT + 1, P = kWave / TT;
    const int C = p.channels, L = p.seqlen, lane = threadIdx.x;
    int b, t0;
    if (!ln_tile(ntiles, tpb, TT, b, t0)) return;
    float* tile = ln_smem;                             // [C][TT + 1]
    float* stat = tile + C * PAD;                      // [2][TT]: mean, rstd
    float* gb = stat + 2 * TT;                         // [2][C]: weight, bias (a global load per output element would serialise the store loop)
    if constexpr (NORM) {
        for (int c = lane; c < C; c += kWave) {        // a null weight: gain 1 in the plain mode (with the add it selects NORM = false)
            gb[c] = ADD || p.weight ? static_cast<const float*>(p.weight)[c] : 1.0f;
            gb[C + c] = p.bias ? static_cast<const float*>(p.bias)[c] : 0.0f;
        }
    }
    const float s = ADD && p.scale ? static_cast<const float*>(p.scale)[b] : 1.0f;
    const int nt = min(TT, L - t0);
    ln_load_cm<TI, TT>(tile, static_cast<const TI*>(p.x) + (int64_t)b * p.x_batch_stride, p.x_c_stride, C, t0, L, lane);
    wave_lds_fence();
    if constexpr (ADD) {
        // x_new = x + s * branch: one fma in f32, rounded once to x's type; the tile holds x_new as it will be stored
        ln_read_tm<TB, TT>(static_cast<const TB*>(p.branch) + (int64_t)b * p.branch_batch_stride + (int64_t)t0 * p.branch_token_stride,
                           p.branch_token_stride, C, nt, lane, [&](int c, int tt, float v) {
                               float* q = tile + c * PAD + tt;
                               *q = ln_round<TI>(fmaf(s, v, *q));
                           });
        wave_lds_fence();
        // x_new: channel-major, 16-byte vectors along the tokens
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
    if constexpr (!NORM) return;
    const int t = lane % TT, part = lane / TT;
    // Two sweeps over the tile.  The first takes the mean around channel 0 of the token (a shift common to all channels cancels
    // there); the second takes sum d and sum d^2 around THAT mean, so that m * m below is a rounding-sized correction.  One
    // sweep around channel 0 alone loses the variance when channel 0 is the outlier: m * m is then as large as s2 / C and up to
    // C roundings land in rstd (channel 0 = 40 among randn, C = 512: 40 to 100 times the per-token bound of the tests).
    const float pivot = tile[t];
    const float inv_c = 1.0f / (float)C;
    float s0 = 0.0f;
#pragma unroll 8
    for (int c = part; c < C; c += P) s0 += tile[c * PAD + t] - pivot;
    const float mu = pivot + ln_parts_sum<TT>(s0) * inv_c;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll 8
    for (int c = part; c < C; c += P) {
        const float d = tile[c * PAD + t] - mu;
        s1 += d;
        s2 = fmaf(d, d, s2);
    }
    s1 = ln_parts_sum<TT>(s1);
    s2 = ln_parts_sum<TT>(s2);
    const float m = s1 * inv_c;
    const float mean = mu + m;
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
    ln_write_tm<TO>(static_cast<TO*>(p.y) + (int64_t)b * p.y_batch_stride + (int64_t)t0 * p.y_token_stride, p.y_token_stride, C, nt, lane,
                    [&](int c, int tt) { return (tile[c * PAD + tt] - stat[tt]) * stat[TT + tt] * gb[c] + gb[C + c]; });
}

template <typename TI, typename TB, typename TO, int TT, bool ADD>
__global__ void __launch_bounds__(kWave) ln_cm_bwd_kernel(const vivim_add_layernorm_params p, const int ntiles, const int tpb) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    constexpr int PAD = TT + 1, P = kWave / TT;
    const int C = p.channels, L = p.seqlen, lane = threadIdx.x;
    int b, t0;
    if (!ln_tile(ntiles, tpb, TT, b, t0)) return;
    const int tile_id = b * tpb + t0 / TT;
    float* xt = ln_smem;                               // [C][TT + 1]: x_new
    float* gt = xt + C * PAD;                          // [C][TT + 1]: dy, then (ADD) dx
    float* stat = gt + C * PAD;                        // [4][TT]: mean, rstd, S1 / C, S2 / C
    float* gam = stat + 4 * TT;                        // [C]: weight
    const int nt = min(TT, L - t0);
    for (int c = lane; c < C; c += kWave) gam[c] = ADD || p.weight ? static_cast<const float*>(p.weight)[c] : 1.0f;
    if (!ADD || p.dy) {                                // with the add, dy may be absent (only dres arrives)
        ln_read_tm<TO, TT>(static_cast<const TO*>(p.dy) + (int64_t)b * p.y_batch_stride + (int64_t)t0 * p.y_token_stride, p.y_token_stride,
                           C, nt, lane, [&](int c, int tt, float v) { gt[c * PAD + tt] = v; });
    } else {
        for (int i = lane; i < C * PAD; i += kWave) gt[i] = 0.0f;
    }
    ln_load_cm<TI, TT>(xt, static_cast<const TI*>(p.x_new) + (int64_t)b * p.x_new_batch_stride, p.x_new_c_stride, C, t0, L, lane);
    const int t = lane % TT, part = lane / TT;
    const bool tok = t0 + t < L;
    const float mean = tok ? static_cast<const float*>(p.mean)[(int64_t)b * L + t0 + t] : 0.0f;
    const float rstd = tok ? static_cast<const float*>(p.rstd)[(int64_t)b * L + t0 + t] : 0.0f;
    const float s = ADD && p.scale ? static_cast<const float*>(p.scale)[b] : 1.0f;
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
        if constexpr (ADD) wave_lds_fence();           // the sweep below overwrites the dy tile
    }
    // dx = rstd * (dy gamma - S1 / C - xhat S2 / C) (+ dres), channel-major with 16-byte vectors along the tokens.  The one place
    // where the two modes keep separate bodies: the add wants eight dres vectors per lane in flight, and the same batched sweep with
    // the dres loads compiled out costs the plain mode registers and occupancy (fp32 TT 32: 92 -> 98 VGPRs, 5 -> 4 waves; bf16 -> f32
    // TT 16: 72 -> 91, 7 -> 5), so that one goes vector by vector.
    constexpr int E = LnVec<TI>::E;
    constexpr int VPR = TT / E;
    TI* __restrict__ dxb = static_cast<TI*>(p.dx) + (int64_t)b * p.dx_batch_stride;
    const int nvec = C * VPR;
    if constexpr (!ADD) {
        for (int idx = lane; idx < nvec; idx += kWave) {
            const int c = idx / VPR, v = idx - c * VPR;
            const int tg = t0 + v * E;
            if (tg >= L) continue;
            const float g = gam[c];
            typename LnVec<TI>::U u;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = v * E + e;
                const float r = stat[TT + k];
                const float xh = (xt[c * PAD + k] - stat[k]) * r;
                u.e[e] = from_f32<TI>(r * (gt[c * PAD + k] * g - stat[2 * TT + k] - xh * stat[3 * TT + k]));
            }
            *reinterpret_cast<typename LnVec<TI>::vec*>(dxb + (int64_t)c * p.dx_c_stride + tg) = u.v;
        }
    } else {
        // the f32 value replaces dy in the tile for the token-major pass below
        const TI* __restrict__ drb = static_cast<const TI*>(p.dres) + (int64_t)b * p.dres_batch_stride;
        const bool has_res = p.dres != nullptr;
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
        ln_write_tm<TB>(static_cast<TB*>(p.dbranch) + (int64_t)b * p.dbranch_batch_stride + (int64_t)t0 * p.dbranch_token_stride,
                        p.dbranch_token_stride, C, nt, lane, [&](int c, int tt) { return s * gt[c * PAD + tt]; });
    }
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
    ln_write_tm<TB>(static_cast<TB*>(p.dbranch) + (int64_t)b * p.dbranch_batch_stride + (int64_t)t0 * p.dbranch_token_stride,
                    p.dbranch_token_stride, C, min(TT, L - t0), lane, [&](int c, int tt) { return s * tile[c * PAD + tt]; });
}

// dweight[c] += sum over the workspace rows of column c, dbias[c] += ... of column C + c.  grid (ceil(2C / 64), row groups),
// 256 threads: lane = column, the four waves of a workgroup and the row groups interleave the rows (about eight rows per wave).
__global__ void __launch_bounds__(256) ln_reduce_kernel(const float* __restrict__ ws, int ntiles, int C, float* dweight, float* dbias) {
    __shared__ float part[4][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * kWave + lane;
    float s = 0.0f;
    if (col < 2 * C) {
        const int step = 4 * (int)gridDim.y;
        for (int r = blockIdx.y * 4 + wave; r < ntiles; r += step) s += ws[(int64_t)r * 2 * C + col];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && col < 2 * C) {
        s = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        if (col < C) { if (dweight) atomicAdd(dweight + col, s); }
        else if (dbias) atomicAdd(dbias + col - C, s);
    }
}

// tokens per wave: the largest of 32 / 16 / 8 that leaves a couple of thousand waves and at most 64 KB of LDS per wave
// (VIVIM_LN_TT overrides, for the tests and for tuning); from batch, seqlen, channels and itype
static int layernorm_tile_tokens(const vivim_add_layernorm_params& p) {
    const char* e = getenv("VIVIM_LN_TT");
    const int forced = e ? atoi(e) : 0;
    const int vec = p.itype == VIVIM_F32 ? 4 : 8;
    for (int TT : {32, 16, 8}) {
        if (TT % vec != 0 || ln_bwd_smem(p.channels, TT) > 65536) continue;
        if (forced == TT) return TT;
        if (!forced && (int64_t)p.batch * ((p.seqlen + TT - 1) / TT) >= (TT == 32 ? 4096 : 2048)) return TT;
    }
    return 8;
}
static size_t add_layernorm_bwd_workspace_bytes(const vivim_add_layernorm_params& p) {
    const int TT = layernorm_tile_tokens(p);
    return (size_t)p.batch * ((p.seqlen + TT - 1) / TT) * 2 * p.channels * sizeof(float);
}

static void ln_reduce_launch(const float* ws, int ntiles, int C, float* dweight, float* dbias, hipStream_t stream) {
    hipLaunchKernelGGL(ln_reduce_kernel, dim3((2 * C + kWave - 1) / kWave, std::min(128, std::max(1, ntiles / 32))), dim3(256), 0, stream,
                       ws, ntiles, C, dweight, dbias);
}

template <typename TI, typename TB, typename TO, int TT, bool ADD, bool NORM>
static void ln_launch_tt(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    const int tpb = (p.seqlen + TT - 1) / TT, ntiles = p.batch * tpb;
    const dim3 grid((unsigned)((ntiles + 7) / 8 * 8)), block(kWave);
    if constexpr (!NORM) {                             // the add alone: one tile, no statistics
        const size_t smem = (size_t)p.channels * (TT + 1) * sizeof(float);
        if (!bwd) hipLaunchKernelGGL((ln_cm_fwd_kernel<TI, TB, TO, TT, ADD, false>), grid, block, smem, stream, p, ntiles, tpb);
        else hipLaunchKernelGGL((add_cm_bwd_kernel<TI, TB, TT>), grid, block, smem, stream, p, ntiles, tpb);
    } else if (!bwd) {
        hipLaunchKernelGGL((ln_cm_fwd_kernel<TI, TB, TO, TT, ADD, true>), grid, block, ln_fwd_smem(p.channels, TT), stream, p, ntiles, tpb);
    } else {
        hipLaunchKernelGGL((ln_cm_bwd_kernel<TI, TB, TO, TT, ADD>), grid, block, ln_bwd_smem(p.channels, TT), stream, p, ntiles, tpb);
        if (p.workspace && (p.dweight || p.dbias))
            ln_reduce_launch(static_cast<const float*>(p.workspace), ntiles, p.channels, static_cast<float*>(p.dweight),
                             static_cast<float*>(p.dbias), stream);
    }
}
template <typename TI, typename TB, typename TO, bool ADD, bool NORM>
static void ln_launch(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    switch (layernorm_tile_tokens(p)) {
        case 32: ln_launch_tt<TI, TB, TO, 32, ADD, NORM>(p, bwd, stream); break;
        case 16: ln_launch_tt<TI, TB, TO, 16, ADD, NORM>(p, bwd, stream); break;
        default: ln_launch_tt<TI, TB, TO, 8, ADD, NORM>(p, bwd, stream); break;
    }
}

template <typename TI, typename TB>
static bool aln_pair(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
    if (!p.weight) { ln_launch<TI, TB, TI, true, false>(p, bwd, stream); return true; }   // add-only: no y, its type does not matter
    // the output / incoming-gradient side is f32 (what autocast makes of layer_norm) or the input's own type
    if (p.otype == VIVIM_F32) { ln_launch<TI, TB, float, true, true>(p, bwd, stream); return true; }
    if (p.otype == p.itype) { ln_launch<TI, TB, TI, true, true>(p, bwd, stream); return true; }
    return false;
}

static bool add_layernorm_dispatch(const vivim_add_layernorm_params& p, bool bwd, hipStream_t stream) {
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

// The plain LayerNorm as the family sees it: x_new is x itself, no branch, no dres, no dbranch.
static vivim_add_layernorm_params ln_plain(const vivim_layernorm_params& p) {
    vivim_add_layernorm_params q = {};
    q.batch = p.batch; q.seqlen = p.seqlen; q.channels = p.channels;
    q.itype = q.btype = p.itype; q.otype = p.otype; q.eps = p.eps;
    q.x_batch_stride = q.x_new_batch_stride = p.x_batch_stride; q.x_c_stride = q.x_new_c_stride = p.x_c_stride;
    q.y_batch_stride = p.y_batch_stride; q.y_token_stride = p.y_token_stride;
    q.dx_batch_stride = p.dx_batch_stride; q.dx_c_stride = p.dx_c_stride;
    q.x = p.x; q.x_new = const_cast<void*>(p.x); q.weight = p.weight; q.bias = p.bias;
    q.y = p.y; q.mean = p.mean; q.rstd = p.rstd;
    q.dy = p.dy; q.dx = p.dx; q.dweight = p.dweight; q.dbias = p.dbias; q.workspace = p.workspace;
    return q;
}
static size_t layernorm_bwd_workspace_bytes(const vivim_layernorm_params& p) { return add_layernorm_bwd_workspace_bytes(ln_plain(p)); }

static bool layernorm_dispatch(const vivim_layernorm_params& p, bool bwd, hipStream_t stream) {
    if (p.channels > kLnMaxC) return false;
    const vivim_add_layernorm_params q = ln_plain(p);
    // the output / incoming-gradient side is f32 (what autocast makes of layer_norm) or the input's own type
    if (p.otype == VIVIM_F32) {
        switch (p.itype) {
            case VIVIM_F32: ln_launch<float, float, float, false, true>(q, bwd, stream); return true;
            case VIVIM_F16: ln_launch<f16_t, f16_t, float, false, true>(q, bwd, stream); return true;
            case VIVIM_BF16: ln_launch<bf16_t, bf16_t, float, false, true>(q, bwd, stream); return true;
        }
    } else if (p.otype == p.itype) {
        switch (p.itype) {
            case VIVIM_F16: ln_launch<f16_t, f16_t, f16_t, false, true>(q, bwd, stream); return true;
            case VIVIM_BF16: ln_launch<bf16_t, bf16_t, bf16_t, false, true>(q, bwd, stream); return true;
        }
    }
    return false;
}

}  // namespace vivim

// ---- the C entry points
using vivim::kLnMaxC;

static int check_layernorm(const vivim_layernorm_params* p) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && (p->otype == VIVIM_F32 || p->otype == p->itype));
    VCHECK(p->batch > 0 && p->seqlen > 0 && p->channels > 0 && p->batch <= 65535);
    if (p->channels > kLnMaxC)
        return fail(VIVIM_ERR_UNSUPPORTED, "layernorm_cm: more than %d channels do not fit the backward's two LDS tiles", kLnMaxC);
    const int64_t e = vec_elems(p->itype);                       // 16-byte vectors along the tokens of x / dx
    VCHECK(p->seqlen % e == 0 && p->x_batch_stride % e == 0 && p->x_c_stride % e == 0);
    VCHECK(p->x && aligned16(p->x) && p->mean && p->rstd);
    return VIVIM_OK;
}

// what the forward and the backward of the residual-add LayerNorm share; `e` <- elements per 16-byte vector of x / x_new / dres / dx
static int check_add_layernorm(const vivim_add_layernorm_params* p, int64_t* e) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && dtype_ok(p->btype) && (p->weight == nullptr || dtype_ok(p->otype)));
    VCHECK(p->batch > 0 && p->seqlen > 0 && p->channels > 0 && p->batch <= 65535);
    if (p->channels > kLnMaxC)
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm: more than %d channels do not fit the backward's two LDS tiles", kLnMaxC);
    if (p->btype != p->itype && p->itype != VIVIM_F32)
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm: branch type %d with x type %d is not built (the branch has x's type, or x is f32)",
                    p->btype, p->itype);
    if (p->weight && p->otype != VIVIM_F32 && p->otype != p->itype)
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm: output type %d with x type %d is not built (f32 or x's type)", p->otype, p->itype);
    *e = vec_elems(p->itype);
    VCHECK(p->seqlen % *e == 0);
    return VIVIM_OK;
}

extern "C" {

int vivim_layernorm_cm_fwd(const vivim_layernorm_params* p, void* stream) {
    if (int rc = check_layernorm(p)) return rc;
    VCHECK(p->y != nullptr);
    return after_dispatch(vivim::layernorm_dispatch(*p, false, as_stream(stream)), "layernorm_cm_fwd",
                          "layernorm_cm_fwd not implemented for input type %d / output type %d", p->itype, p->otype);
}

size_t vivim_layernorm_bwd_workspace_bytes(const vivim_layernorm_params* p) {
    return p && p->batch > 0 && p->seqlen > 0 && p->channels > 0 ? vivim::layernorm_bwd_workspace_bytes(*p) : 0;
}

int vivim_layernorm_cm_bwd(const vivim_layernorm_params* p, void* stream) {
    if (int rc = check_layernorm(p)) return rc;
    VCHECK(p->dy && p->dx && aligned16(p->dx));
    const int64_t e = vec_elems(p->itype);
    VCHECK(p->dx_batch_stride % e == 0 && p->dx_c_stride % e == 0);
    if ((p->dweight || p->dbias) && !p->workspace)
        return fail(VIVIM_ERR_INVALID, "layernorm_cm_bwd: dweight / dbias need the workspace (vivim_layernorm_bwd_workspace_bytes)");
    return after_dispatch(vivim::layernorm_dispatch(*p, true, as_stream(stream)), "layernorm_cm_bwd",
                          "layernorm_cm_bwd not implemented for input type %d / output type %d", p->itype, p->otype);
}

int vivim_add_layernorm_cm_fwd(const vivim_add_layernorm_params* p, void* stream) {
    int64_t e = 0;
    if (int rc = check_add_layernorm(p, &e)) return rc;
    VCHECK(p->x && p->branch && p->x_new && aligned16(p->x) && aligned16(p->x_new));
    VCHECK(p->x_batch_stride % e == 0 && p->x_c_stride % e == 0 && p->x_new_batch_stride % e == 0 && p->x_new_c_stride % e == 0);
    if (p->weight) VCHECK(p->y && p->mean && p->rstd);
    return after_dispatch(vivim::add_layernorm_dispatch(*p, false, as_stream(stream)), "add_layernorm_cm_fwd",
                          "add_layernorm_cm_fwd not implemented for x type %d / branch type %d / output type %d", p->itype, p->btype, p->otype);
}

size_t vivim_add_layernorm_bwd_workspace_bytes(const vivim_add_layernorm_params* p) {
    return p && p->batch > 0 && p->seqlen > 0 && p->channels > 0 ? vivim::add_layernorm_bwd_workspace_bytes(*p) : 0;
}

int vivim_add_layernorm_cm_bwd(const vivim_add_layernorm_params* p, void* stream) {
    int64_t e = 0;
    if (int rc = check_add_layernorm(p, &e)) return rc;
    if (p->dres) VCHECK(aligned16(p->dres) && p->dres_batch_stride % e == 0 && p->dres_c_stride % e == 0);
    if (p->weight) {
        VCHECK(p->x_new && aligned16(p->x_new) && p->mean && p->rstd && (p->dy || p->dres));
        VCHECK(p->x_new_batch_stride % e == 0 && p->x_new_c_stride % e == 0);
        VCHECK(p->dx && aligned16(p->dx) && p->dx_batch_stride % e == 0 && p->dx_c_stride % e == 0);
        if ((p->dweight || p->dbias) && !p->workspace)
            return fail(VIVIM_ERR_INVALID,
                        "add_layernorm_cm_bwd: dweight / dbias need the workspace (vivim_add_layernorm_bwd_workspace_bytes)");
    } else {
        VCHECK(p->dres && p->dbranch);                 // add-only: dbranch = scale * dres, dx is dres itself
    }
    return after_dispatch(vivim::add_layernorm_dispatch(*p, true, as_stream(stream)), "add_layernorm_cm_bwd",
                          "add_layernorm_cm_bwd not implemented for x type %d / branch type %d / output type %d", p->itype, p->btype, p->otype);
}

}  // extern "C"
