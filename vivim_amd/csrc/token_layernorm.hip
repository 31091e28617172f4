// token_layernorm.hip -- LayerNorm over the channels of TOKEN-major rows, forward and backward (include/vivim_hip.h:
// vivim_token_layernorm_params): the layernorm_before / layernorm_after of the SegFormer blocks, (B, N, C) contiguous with
// C = 64 / 128 / 320 / 512.  layernorm.hip is the family for channel-major views; this is the one for rows.
//
// G = 8 / 16 / 32 / 64 lanes own one row, a wave carries 64 / G rows, and every lane holds K chunks of E consecutive channels of
// its row in registers (chunk j of the row belongs to lane j % G, slot j / G: consecutive lanes read consecutive chunks).  E is
// one 16-byte vector of x (4 f32, 8 f16 / bf16) when the channel count, the row strides and the addresses allow it -- at C = 64
// bf16 one wave instruction then reads 8 rows = 1 KB contiguous -- and 1 otherwise (odd C, odd offsets): the same kernels with
// lanes striding over the channels.  G, K and E are template parameters, so the row is never indexed at run time (no scratch).
// Row sums are xor butterflies over the lane offsets < G: every lane of a row ends with the same bits.
// Forward: the mean first, then the sum of squared differences from it on the row in registers (a row with a mean far from 0
// loses nothing to cancellation), one rounding to the output type.
// Backward: dx per row as above; a wave walks its row groups with its dweight / dbias partial sums in registers, folds them over
// the lanes that own the same channels (offsets >= G), then over the workgroup's waves through LDS in wave order, and stores
// ONE slot of the workspace.  A second kernel adds the slots in slot order and WRITES dweight / dbias: no atomics, no pre-zeroed
// outputs, the same bits every run.
// Rows past `rows` and chunks past C are neither read nor written.
// HBM-bound: the forward reads x and writes y once; the backward reads x and dy and writes dx once.
//
// The residual add in front of the norm (vivim_token_add_norm_params) is the same kernels with ADD = true: the forward builds the
// row as h = res + scale * branch, rounds it once to the residual type, stores it (res_out) and norms what it stored; the
// backward adds the gradient arriving at res_out to the norm's and writes it twice, as dres_in and, times scale, as dbranch.
// RMSNorm is a run-time flag of those launches that skips the mean.  With ADD = false all of it is compiled out: the plain
// entry points run the arithmetic they always ran.  E is then one 16-byte vector of the NARROWER of the two types, so that the
// wider stream moves in two 16-byte accesses per chunk.
#include <algorithm>
#include "capi.cuh"

namespace vivim {

constexpr int kTlnWaves = 4;          // waves per workgroup
constexpr int kTlnMaxSlots = 1024;    // workgroups of the backward = slots of its workspace
constexpr int kTlnRedWaves = 16;      // waves of the slot-sum kernel: each adds a contiguous run of slots
constexpr int kTlnMaxC = 1024;        // channels of a row: 64 lanes x 16 registers (tln_launch), what the entry points refuse beyond

template <int G>
__device__ __forceinline__ float tln_row_sum(float v) {
#pragma unroll
    for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

template <typename T, int E>
__device__ __forceinline__ void tln_load(const T* __restrict__ q, bool pred, float (&v)[E]) {
    const RawK<T, E> r = load_vec<T, E>(q, pred);
    unpack<T, E>(r, v);
}

// What the kernels take: either public struct, restated.  x is the norm's input (ADD: the saved res_out of the backward).
struct TlnArgs {
    int32_t rows, channels, rows_per_sample, rms;
    float eps;
    int64_t x_row_stride, y_row_stride, dy_row_stride, dx_row_stride;
    int64_t branch_row_stride, res_row_stride, res_out_row_stride, dres_row_stride, dbranch_row_stride;
    const void *x, *weight, *bias;
    void *y, *mean, *rstd;
    const void* dy;
    void *dx, *dweight, *dbias, *workspace;
    const void *branch, *res, *scale, *dres;         // ADD only
    void *res_out, *dbranch;
};

template <bool ADD, typename TI, typename TO, int G, int K, int E>
__global__ void __launch_bounds__(kWave * kTlnWaves) tln_fwd_kernel(const TlnArgs p) {
    constexpr int RPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sub = lane % G, rl = lane / G;
    const int C = p.channels;
    const float* __restrict__ wp = static_cast<const float*>(p.weight);
    const float* __restrict__ bp = static_cast<const float*>(p.bias);
    const bool norm = !ADD || wp != nullptr;             // ADD without a weight: the add alone
    const bool rms = ADD && p.rms != 0;
    float w[K][E], b[K][E];
    bool cv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (sub + k * G) * E;
        cv[k] = c0 < C;                                  // E > 1: C is a whole number of chunks
        tln_load<float, E>(wp + c0, cv[k] && norm, w[k]);
        tln_load<float, E>(bp + c0, cv[k] && bp != nullptr, b[k]);
    }
    const float inv_c = 1.0f / (float)C;
    const int64_t rows = p.rows, ngroups = (rows + RPW - 1) / RPW;
    const TI* __restrict__ x = static_cast<const TI*>(p.x);
    TO* __restrict__ y = static_cast<TO*>(p.y);
    float* __restrict__ meanp = static_cast<float*>(p.mean);
    float* __restrict__ rstdp = static_cast<float*>(p.rstd);
    for (int64_t g = (int64_t)blockIdx.x * kTlnWaves + wave; g < ngroups; g += (int64_t)gridDim.x * kTlnWaves) {
        const int64_t r = g * RPW + rl;
        const bool ok = r < rows;
        float v[K][E];
        if constexpr (ADD) {
            const TO* __restrict__ br = static_cast<const TO*>(p.branch) + r * p.branch_row_stride;
            const TI* __restrict__ rr = static_cast<const TI*>(p.res) + r * p.res_row_stride;
            TI* __restrict__ hr = static_cast<TI*>(p.res_out) + r * p.res_out_row_stride;
            const float* __restrict__ scp = static_cast<const float*>(p.scale);
            const float sc = scp != nullptr && ok ? scp[(int)r / p.rows_per_sample] : 1.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float bv[E];
                tln_load<TO, E>(br + (sub + k * G) * E, ok && cv[k], bv);
                tln_load<TI, E>(rr + (sub + k * G) * E, ok && cv[k] && p.res != nullptr, v[k]);
#pragma unroll
                for (int e = 0; e < E; ++e) v[k][e] = fmaf(sc, bv[e], v[k][e]);
                if (p.res_out != nullptr) {              // the row as stored is the row that is normed
#pragma unroll
                    for (int e = 0; e < E; ++e) v[k][e] = to_f32<TI>(from_f32<TI>(v[k][e]));
                    store_vec<TI, E>(hr + (sub + k * G) * E, ok && cv[k], v[k]);
                }
            }
            if (!norm) continue;
        } else {
            const TI* __restrict__ xr = x + r * p.x_row_stride;
#pragma unroll
            for (int k = 0; k < K; ++k) tln_load<TI, E>(xr + (sub + k * G) * E, ok && cv[k], v[k]);
        }
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < E; ++e) s += v[k][e];    // what was not loaded is 0
        float mean = tln_row_sum<G>(s) * inv_c;
        if constexpr (ADD) mean = rms ? 0.0f : mean;
        float q = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float d = cv[k] ? v[k][e] - mean : 0.0f;
                v[k][e] = d;
                q = fmaf(d, d, q);
            }
        const float rstd = rsqrtf(tln_row_sum<G>(q) * inv_c + p.eps);
        TO* __restrict__ yr = y + r * p.y_row_stride;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = fmaf(v[k][e] * rstd, w[k][e], b[k][e]);
            store_vec<TO, E>(yr + (sub + k * G) * E, ok && cv[k], o);
        }
        if (sub == 0 && ok && meanp != nullptr) {
            meanp[r] = mean;
            rstdp[r] = rstd;
        }
    }
}

// grid: the slots.  Every workgroup stores its slot (zeros when it had no row), so the slot sum never reads what nobody wrote.
template <bool ADD, typename TI, typename TO, int G, int K, int E>
__global__ void __launch_bounds__(kWave * kTlnWaves) tln_bwd_kernel(const TlnArgs p) {
    constexpr int RPW = kWave / G, CH = G * K * E;
    __shared__ float red[kTlnWaves][2][CH];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sub = lane % G, rl = lane / G;
    const int C = p.channels;
    const float* __restrict__ wp = static_cast<const float*>(p.weight);
    const bool has_dy = !ADD || (wp != nullptr && p.dy != nullptr);   // ADD without dy: dh is dres
    const bool rms = ADD && p.rms != 0;
    float w[K][E], dw[K][E], db[K][E];
    bool cv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c0 = (sub + k * G) * E;
        cv[k] = c0 < C;
        tln_load<float, E>(wp + c0, cv[k] && has_dy, w[k]);
#pragma unroll
        for (int e = 0; e < E; ++e) dw[k][e] = db[k][e] = 0.0f;
    }
    const float inv_c = 1.0f / (float)C;
    const int64_t rows = p.rows, ngroups = (rows + RPW - 1) / RPW;
    const TI* __restrict__ x = static_cast<const TI*>(p.x);
    const TO* __restrict__ dy = static_cast<const TO*>(p.dy);
    TI* __restrict__ dx = static_cast<TI*>(p.dx);
    const float* __restrict__ meanp = static_cast<const float*>(p.mean);
    const float* __restrict__ rstdp = static_cast<const float*>(p.rstd);
    for (int64_t g = (int64_t)blockIdx.x * kTlnWaves + wave; g < ngroups; g += (int64_t)gridDim.x * kTlnWaves) {
        const int64_t r = g * RPW + rl;
        const bool ok = r < rows;
        const bool okn = ok && has_dy;                   // the norm's side of this row is live
        const TI* __restrict__ xr = x + r * p.x_row_stride;
        const TO* __restrict__ gr = dy + r * p.dy_row_stride;
        float v[K][E], gy[K][E];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            tln_load<TI, E>(xr + (sub + k * G) * E, okn && cv[k], v[k]);
            tln_load<TO, E>(gr + (sub + k * G) * E, okn && cv[k], gy[k]);
        }
        float mean = okn ? meanp[r] : 0.0f;
        const float rstd = okn ? rstdp[r] : 0.0f;
        if constexpr (ADD) mean = rms ? 0.0f : mean;
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float xh = cv[k] ? (v[k][e] - mean) * rstd : 0.0f;      // 0 for a row past the end too (rstd 0, x 0)
                const float gw = gy[k][e] * w[k][e];
                v[k][e] = xh;
                s1 += gw;
                s2 = fmaf(gw, xh, s2);
                dw[k][e] = fmaf(gy[k][e], xh, dw[k][e]);
                db[k][e] += gy[k][e];
                gy[k][e] = gw;
            }
        s1 = tln_row_sum<G>(s1) * inv_c;
        s2 = tln_row_sum<G>(s2) * inv_c;
        if constexpr (ADD) s1 = rms ? 0.0f : s1;
        TI* __restrict__ dxr = dx + r * p.dx_row_stride;
        if constexpr (ADD) {
            const TI* __restrict__ dr = static_cast<const TI*>(p.dres) + r * p.dres_row_stride;
            TO* __restrict__ dbr = static_cast<TO*>(p.dbranch) + r * p.dbranch_row_stride;
            const float* __restrict__ scp = static_cast<const float*>(p.scale);
            const float sc = scp != nullptr && ok ? scp[(int)r / p.rows_per_sample] : 1.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float o[E], t[E];
                tln_load<TI, E>(dr + (sub + k * G) * E, ok && cv[k] && p.dres != nullptr, o);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    o[e] += rstd * (gy[k][e] - s1 - v[k][e] * s2);
                    t[e] = sc * o[e];
                }
                store_vec<TI, E>(dxr + (sub + k * G) * E, ok && cv[k] && dx != nullptr, o);
                store_vec<TO, E>(dbr + (sub + k * G) * E, ok && cv[k] && p.dbranch != nullptr, t);
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float o[E];
#pragma unroll
                for (int e = 0; e < E; ++e) o[e] = rstd * (gy[k][e] - s1 - v[k][e] * s2);
                store_vec<TI, E>(dxr + (sub + k * G) * E, ok && cv[k], o);
            }
        }
    }
    if (p.workspace == nullptr) return;                  // neither dweight nor dbias is wanted (the same in every thread)
    // the rows of the wave that share a channel, then the workgroup's waves in wave order, then this workgroup's slot
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) {
#pragma unroll
            for (int off = G; off < kWave; off <<= 1) {
                dw[k][e] += __shfl_xor(dw[k][e], off, kWave);
                db[k][e] += __shfl_xor(db[k][e], off, kWave);
            }
            if (rl == 0) {
                red[wave][0][(sub + k * G) * E + e] = dw[k][e];
                red[wave][1][(sub + k * G) * E + e] = db[k][e];
            }
        }
    __syncthreads();
    float* __restrict__ slot = static_cast<float*>(p.workspace) + (int64_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x; i < 2 * CH; i += kWave * kTlnWaves) {
        const int which = i / CH, c = i - which * CH;
        if (c >= C) continue;
        float s = red[0][which][c];
#pragma unroll
        for (int wv = 1; wv < kTlnWaves; ++wv) s += red[wv][which][c];
        slot[which * C + c] = s;
    }
}

// dweight[c] = sum over the slots of column c, dbias[c] = ... of column C + c, in slot order: wave w of a workgroup adds the w-th
// run of ceil(nslots / 16) slots, wave 0 then adds the sixteen runs in run order.  grid: ceil(2C / 64), lane = column.
__global__ void __launch_bounds__(kWave * kTlnRedWaves) tln_slot_sum_kernel(const float* __restrict__ ws, int nslots, int C,
                                                                            float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float part[kTlnRedWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int col = blockIdx.x * kWave + lane;
    const int per = (nslots + kTlnRedWaves - 1) / kTlnRedWaves;
    const int s0 = wave * per, s1 = min(s0 + per, nslots);
    float s = 0.0f;
    if (col < 2 * C) {
#pragma unroll 8
        for (int i = s0; i < s1; ++i) s += ws[(int64_t)i * 2 * C + col];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || col >= 2 * C) return;
    s = part[0][lane];
#pragma unroll
    for (int wv = 1; wv < kTlnRedWaves; ++wv) s += part[wv][lane];
    if (col < C) { if (dweight) dweight[col] = s; }
    else if (dbias) dbias[col - C] = s;
}


static int tln_slots(int64_t rows) { return (int)std::min<int64_t>(kTlnMaxSlots, (rows + 3) / 4); }
static size_t token_layernorm_bwd_workspace_bytes(const vivim_token_layernorm_params& p) {
    return (size_t)tln_slots(p.rows) * 2 * p.channels * sizeof(float);
}
static size_t token_add_norm_bwd_workspace_bytes(const vivim_token_add_norm_params& p) {
    return (size_t)tln_slots(p.rows) * 2 * p.channels * sizeof(float);
}

// one stream of a call: its base, its row stride in elements and its element size.  A stream that is not given passes.
static bool tln_s16(const void* q, int64_t stride, int size) {
    return q == nullptr || (reinterpret_cast<uintptr_t>(q) % 16 == 0 && stride * size % 16 == 0);
}

template <bool ADD, typename TI, typename TO, int G, int K, int E>
static void tln_launch_gk(const TlnArgs& p, bool bwd, hipStream_t stream) {
    const int64_t ngroups = ((int64_t)p.rows + kWave / G - 1) / (kWave / G);
    const int64_t wgs = (ngroups + kTlnWaves - 1) / kTlnWaves;
    const dim3 block(kWave * kTlnWaves);
    if (!bwd) {
        hipLaunchKernelGGL((tln_fwd_kernel<ADD, TI, TO, G, K, E>), dim3((unsigned)std::min<int64_t>(wgs, 2048)), block, 0, stream, p);
        return;
    }
    const int nslots = (int)std::min<int64_t>(wgs, tln_slots(p.rows));     // wgs <= ceil(rows / 4)
    hipLaunchKernelGGL((tln_bwd_kernel<ADD, TI, TO, G, K, E>), dim3((unsigned)nslots), block, 0, stream, p);
    if (p.workspace != nullptr)
        hipLaunchKernelGGL(tln_slot_sum_kernel, dim3((unsigned)((2 * p.channels + kWave - 1) / kWave)), dim3(kWave * kTlnRedWaves), 0, stream,
                           static_cast<const float*>(p.workspace), nslots, p.channels, static_cast<float*>(p.dweight),
                           static_cast<float*>(p.dbias));
}

// the smallest lane group, then the fewest chunks per lane, that hold a row.  `vec`: 16-byte accesses (the caller has checked
// every stream of the call); a chunk is then one 16-byte vector of the narrower type of the call
template <bool ADD, typename TI, typename TO>
static void tln_launch(const TlnArgs& p, bool bwd, bool vec, hipStream_t stream) {
    constexpr int EV = 16 / (int)(ADD && sizeof(TO) < sizeof(TI) ? sizeof(TO) : sizeof(TI));
    if (vec) {
        const int n = p.channels / EV;
        if (n <= 8) tln_launch_gk<ADD, TI, TO, 8, 1, EV>(p, bwd, stream);
        else if (n <= 16) tln_launch_gk<ADD, TI, TO, 16, 1, EV>(p, bwd, stream);
        else if (n <= 32) tln_launch_gk<ADD, TI, TO, 32, 1, EV>(p, bwd, stream);
        else if (n <= 64) tln_launch_gk<ADD, TI, TO, 64, 1, EV>(p, bwd, stream);
        else if (n <= 128) tln_launch_gk<ADD, TI, TO, 64, 2, EV>(p, bwd, stream);
        else if constexpr (EV == 4) tln_launch_gk<ADD, TI, TO, 64, 4, EV>(p, bwd, stream);     // 1024 channels are 128 vectors of a 16-bit row
    } else {
        const int n = p.channels;
        if (n <= 8) tln_launch_gk<ADD, TI, TO, 8, 1, 1>(p, bwd, stream);
        else if (n <= 64) tln_launch_gk<ADD, TI, TO, 64, 1, 1>(p, bwd, stream);
        else if (n <= 128) tln_launch_gk<ADD, TI, TO, 64, 2, 1>(p, bwd, stream);
        else if (n <= 256) tln_launch_gk<ADD, TI, TO, 64, 4, 1>(p, bwd, stream);
        else if (n <= 512) tln_launch_gk<ADD, TI, TO, 64, 8, 1>(p, bwd, stream);
        else tln_launch_gk<ADD, TI, TO, 64, 16, 1>(p, bwd, stream);
    }
}

static bool token_layernorm_pair_ok(int itype, int otype) {
    return otype == itype || otype == VIVIM_F32 || itype == VIVIM_F32;
}

static bool token_layernorm_dispatch(const vivim_token_layernorm_params& p, bool bwd, hipStream_t stream) {
    if (p.channels < 1 || p.channels > kTlnMaxC || !token_layernorm_pair_ok(p.itype, p.otype)) return false;
    TlnArgs a = {};
    a.rows = p.rows, a.channels = p.channels, a.eps = p.eps;
    a.x_row_stride = p.x_row_stride, a.y_row_stride = p.y_row_stride, a.dy_row_stride = p.dy_row_stride, a.dx_row_stride = p.dx_row_stride;
    a.x = p.x, a.weight = p.weight, a.bias = p.bias, a.y = p.y, a.mean = p.mean, a.rstd = p.rstd;
    a.dy = p.dy, a.dx = p.dx, a.dweight = p.dweight, a.dbias = p.dbias, a.workspace = p.workspace;
    if (bwd && !p.dweight && !p.dbias) a.workspace = nullptr;       // nothing to sum: the kernel stores no slot
    // 16-byte accesses: whole vectors of x per row, and every address and row stride of this call on a 16-byte boundary
    const int isz = elem_bytes(p.itype), osz = elem_bytes(p.otype);
    bool vec = p.channels % (16 / isz) == 0 && tln_s16(p.x, p.x_row_stride, isz) && tln_s16(p.weight, 0, 4);
    if (!bwd) vec = vec && tln_s16(p.y, p.y_row_stride, osz) && tln_s16(p.bias, 0, 4);
    else vec = vec && tln_s16(p.dy, p.dy_row_stride, osz) && tln_s16(p.dx, p.dx_row_stride, isz);
    switch (p.itype * 3 + p.otype) {
        case VIVIM_F32 * 3 + VIVIM_F32: tln_launch<false, float, float>(a, bwd, vec, stream); return true;
        case VIVIM_F32 * 3 + VIVIM_F16: tln_launch<false, float, f16_t>(a, bwd, vec, stream); return true;
        case VIVIM_F32 * 3 + VIVIM_BF16: tln_launch<false, float, bf16_t>(a, bwd, vec, stream); return true;
        case VIVIM_F16 * 3 + VIVIM_F32: tln_launch<false, f16_t, float>(a, bwd, vec, stream); return true;
        case VIVIM_F16 * 3 + VIVIM_F16: tln_launch<false, f16_t, f16_t>(a, bwd, vec, stream); return true;
        case VIVIM_BF16 * 3 + VIVIM_F32: tln_launch<false, bf16_t, float>(a, bwd, vec, stream); return true;
        case VIVIM_BF16 * 3 + VIVIM_BF16: tln_launch<false, bf16_t, bf16_t>(a, bwd, vec, stream); return true;
    }
    return false;
}

// (branch = y type, residual type): the same, or a 16-bit branch on an f32 residual stream (the autocast case)
static bool token_add_norm_pair_ok(int btype, int rtype) {
    return rtype == btype || (rtype == VIVIM_F32 && (btype == VIVIM_F16 || btype == VIVIM_BF16));
}

static bool token_add_norm_dispatch(const vivim_token_add_norm_params& p, bool bwd, hipStream_t stream) {
    if (p.channels < 1 || p.channels > kTlnMaxC || !token_add_norm_pair_ok(p.btype, p.rtype) || p.otype != p.btype) return false;
    TlnArgs a = {};
    a.rows = p.rows, a.channels = p.channels, a.rows_per_sample = p.rows_per_sample, a.rms = p.rms, a.eps = p.eps;
    a.weight = p.weight, a.bias = p.bias, a.mean = p.mean, a.rstd = p.rstd, a.scale = p.scale;
    const int bsz = elem_bytes(p.btype), rsz = elem_bytes(p.rtype);
    bool vec = p.channels % (16 / std::min(bsz, rsz)) == 0 && tln_s16(p.weight, 0, 4);
    if (!bwd) {
        a.branch = p.branch, a.branch_row_stride = p.branch_row_stride;
        a.res = p.res, a.res_row_stride = p.res_row_stride;
        a.res_out = p.res_out, a.res_out_row_stride = p.res_out_row_stride;
        if (p.weight != nullptr) a.y = p.y, a.y_row_stride = p.y_row_stride;
        vec = vec && tln_s16(a.branch, a.branch_row_stride, bsz) && tln_s16(a.res, a.res_row_stride, rsz) &&
              tln_s16(a.res_out, a.res_out_row_stride, rsz) && tln_s16(a.y, a.y_row_stride, bsz) && tln_s16(p.bias, 0, 4);
    } else {
        if (p.weight != nullptr) {
            a.x = p.res_out, a.x_row_stride = p.res_out_row_stride;
            a.dy = p.dy, a.dy_row_stride = p.dy_row_stride;
            a.dweight = p.dweight, a.dbias = p.dbias;
            a.workspace = p.dweight || p.dbias ? p.workspace : nullptr;      // nothing to sum: the kernel stores no slot
        }
        a.dres = p.dres, a.dres_row_stride = p.dres_row_stride;
        a.dx = p.dres_in, a.dx_row_stride = p.dres_in_row_stride;
        a.dbranch = p.dbranch, a.dbranch_row_stride = p.dbranch_row_stride;
        if (a.dy == nullptr) a.x = nullptr;              // dh is dres: the saved row is not read
        vec = vec && tln_s16(a.x, a.x_row_stride, rsz) && tln_s16(a.dy, a.dy_row_stride, bsz) && tln_s16(a.dres, a.dres_row_stride, rsz) &&
              tln_s16(a.dx, a.dx_row_stride, rsz) && tln_s16(a.dbranch, a.dbranch_row_stride, bsz);
    }
    switch (p.btype * 3 + p.rtype) {
        case VIVIM_F32 * 3 + VIVIM_F32: tln_launch<true, float, float>(a, bwd, vec, stream); return true;
        case VIVIM_F16 * 3 + VIVIM_F16: tln_launch<true, f16_t, f16_t>(a, bwd, vec, stream); return true;
        case VIVIM_BF16 * 3 + VIVIM_BF16: tln_launch<true, bf16_t, bf16_t>(a, bwd, vec, stream); return true;
        case VIVIM_F16 * 3 + VIVIM_F32: tln_launch<true, float, f16_t>(a, bwd, vec, stream); return true;
        case VIVIM_BF16 * 3 + VIVIM_F32: tln_launch<true, float, bf16_t>(a, bwd, vec, stream); return true;
    }
    return false;
}

}  // namespace vivim

// ---- the C entry points
using vivim::kTlnMaxC;

// every refusal the forward and the backward of the token-major LayerNorm share, before any launch
static int check_token_layernorm(const vivim_token_layernorm_params* p, const char* fn) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_token_layernorm_params", p->struct_bytes, sizeof(*p))) return rc;
    VCHECK(dtype_ok(p->itype) && dtype_ok(p->otype));
    VCHECK(p->rows > 0);
    if (p->channels < 1)
        return fail(VIVIM_ERR_INVALID, "%s: channels = %d: a row has at least one channel", fn, p->channels);
    if (p->channels > kTlnMaxC)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: channels = %d: a row of more than %d channels does not fit the lanes' registers", fn,
                    p->channels, kTlnMaxC);
    if (!vivim::token_layernorm_pair_ok(p->itype, p->otype))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: input type %d with output type %d is not built (the same type, an f32 output, or an f32 input)",
                    fn, p->itype, p->otype);
    VCHECK(p->x != nullptr && aligned(p->x, p->itype == VIVIM_F32 ? 4 : 2));
    VCHECK(p->weight != nullptr && aligned(p->weight, 4));
    if (p->x_row_stride < p->channels)
        return fail(VIVIM_ERR_INVALID, "%s: x_row_stride = %lld is less than the %d channels of a row", fn, (long long)p->x_row_stride,
                    p->channels);
    return VIVIM_OK;
}

// every refusal the forward and the backward of the token-major residual add + norm share, before any launch
static int check_token_add_norm(const vivim_token_add_norm_params* p, const char* fn) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_token_add_norm_params", p->struct_bytes, sizeof(*p))) return rc;
    if (!dtype_ok(p->btype) || !dtype_ok(p->rtype) || !dtype_ok(p->otype))
        return fail(VIVIM_ERR_INVALID, "%s: btype = %d, rtype = %d, otype = %d: a type tag is 0 (f32), 1 (f16) or 2 (bf16)", fn, p->btype,
                    p->rtype, p->otype);
    if (p->rows <= 0) return fail(VIVIM_ERR_INVALID, "%s: rows = %d: at least one row", fn, p->rows);
    if (p->channels < 1)
        return fail(VIVIM_ERR_INVALID, "%s: channels = %d: a row has at least one channel", fn, p->channels);
    if (p->channels > kTlnMaxC)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: channels = %d: a row of more than %d channels does not fit the lanes' registers", fn,
                    p->channels, kTlnMaxC);
    if (!vivim::token_add_norm_pair_ok(p->btype, p->rtype) || p->otype != p->btype)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: branch type %d with residual type %d and output type %d is not built (one type, or an "
                    "f16 / bf16 branch and output on an f32 residual)", fn, p->btype, p->rtype, p->otype);
    if (p->rms != 0 && p->rms != 1) return fail(VIVIM_ERR_INVALID, "%s: rms = %d: 0 (LayerNorm) or 1 (RMSNorm)", fn, p->rms);
    if (p->scale != nullptr && (p->rows_per_sample <= 0 || p->rows % p->rows_per_sample != 0))
        return fail(VIVIM_ERR_INVALID, "%s: rows_per_sample = %d with scale: it must be positive and divide rows = %d", fn,
                    p->rows_per_sample, p->rows);
    return VIVIM_OK;
}

// one tensor of a call: required or not, element-aligned, a row stride that holds a row
static int check_tan_tensor(const char* fn, const char* name, const void* q, bool required, int type, int64_t stride, int channels) {
    if (q == nullptr)
        return required ? fail(VIVIM_ERR_INVALID, "%s: %s is NULL", fn, name) : VIVIM_OK;
    if (!aligned(q, elem_bytes(type)))
        return fail(VIVIM_ERR_INVALID, "%s: %s = %p is not aligned to its element type", fn, name, q);
    if (stride < channels)
        return fail(VIVIM_ERR_INVALID, "%s: %s_row_stride = %lld is less than the %d channels of a row", fn, name, (long long)stride, channels);
    return VIVIM_OK;
}
static int check_tan_f32(const char* fn, const char* name, const void* q, bool required) {
    if (q == nullptr)
        return required ? fail(VIVIM_ERR_INVALID, "%s: %s is NULL", fn, name) : VIVIM_OK;
    return aligned(q, 4) ? VIVIM_OK : fail(VIVIM_ERR_INVALID, "%s: %s = %p is not aligned to its element type", fn, name, q);
}

extern "C" {

int vivim_token_layernorm_fwd(const vivim_token_layernorm_params* p, void* stream) {
    if (int rc = check_token_layernorm(p, "token_layernorm_fwd")) return rc;
    VCHECK(p->y != nullptr && aligned(p->y, p->otype == VIVIM_F32 ? 4 : 2));
    VCHECK(aligned(p->bias, 4));                                     // NULL: zeros
    VCHECK((p->mean == nullptr) == (p->rstd == nullptr) && aligned(p->mean, 4) && aligned(p->rstd, 4));
    if (p->y_row_stride < p->channels)
        return fail(VIVIM_ERR_INVALID, "token_layernorm_fwd: y_row_stride = %lld is less than the %d channels of a row",
                    (long long)p->y_row_stride, p->channels);
    return after_dispatch(vivim::token_layernorm_dispatch(*p, false, as_stream(stream)), "token_layernorm_fwd",
                          "token_layernorm_fwd not implemented for input type %d / output type %d", p->itype, p->otype);
}

size_t vivim_token_layernorm_bwd_workspace_bytes(const vivim_token_layernorm_params* p) {
    return p && p->rows > 0 && p->channels > 0 && p->channels <= kTlnMaxC ? vivim::token_layernorm_bwd_workspace_bytes(*p) : 0;
}

int vivim_token_layernorm_bwd(const vivim_token_layernorm_params* p, void* stream) {
    if (int rc = check_token_layernorm(p, "token_layernorm_bwd")) return rc;
    VCHECK(p->dy != nullptr && aligned(p->dy, p->otype == VIVIM_F32 ? 4 : 2));
    VCHECK(p->dx != nullptr && aligned(p->dx, p->itype == VIVIM_F32 ? 4 : 2));
    VCHECK(p->mean != nullptr && p->rstd != nullptr && aligned(p->mean, 4) && aligned(p->rstd, 4));
    VCHECK(aligned(p->dweight, 4) && aligned(p->dbias, 4) && aligned(p->workspace, 4));
    if (p->dy_row_stride < p->channels || p->dx_row_stride < p->channels)
        return fail(VIVIM_ERR_INVALID, "token_layernorm_bwd: dy_row_stride = %lld / dx_row_stride = %lld is less than the %d channels of a row",
                    (long long)p->dy_row_stride, (long long)p->dx_row_stride, p->channels);
    if ((p->dweight || p->dbias) && !p->workspace)
        return fail(VIVIM_ERR_INVALID, "token_layernorm_bwd: dweight / dbias need the workspace (vivim_token_layernorm_bwd_workspace_bytes)");
    return after_dispatch(vivim::token_layernorm_dispatch(*p, true, as_stream(stream)), "token_layernorm_bwd",
                          "token_layernorm_bwd not implemented for input type %d / output type %d", p->itype, p->otype);
}

int vivim_token_add_norm_fwd(const vivim_token_add_norm_params* p, void* stream) {
    const char* fn = "token_add_norm_fwd";
    if (int rc = check_token_add_norm(p, fn)) return rc;
    const bool norm = p->weight != nullptr;
    const int C = p->channels;
    if (int rc = check_tan_tensor(fn, "branch", p->branch, true, p->btype, p->branch_row_stride, C)) return rc;
    if (int rc = check_tan_tensor(fn, "res", p->res, false, p->rtype, p->res_row_stride, C)) return rc;
    // the add alone writes nothing else; a residual that is read is a sum that is stored (the backward reads it)
    if (int rc = check_tan_tensor(fn, "res_out", p->res_out, !norm || p->res != nullptr, p->rtype, p->res_out_row_stride, C)) return rc;
    if (int rc = check_tan_f32(fn, "scale", p->scale, false)) return rc;
    if (norm) {
        if (int rc = check_tan_tensor(fn, "y", p->y, true, p->otype, p->y_row_stride, C)) return rc;
        if (int rc = check_tan_f32(fn, "weight", p->weight, true)) return rc;
        if (int rc = check_tan_f32(fn, "bias", p->bias, false)) return rc;
        if ((p->mean == nullptr) != (p->rstd == nullptr))
            return fail(VIVIM_ERR_INVALID, "%s: mean = %p with rstd = %p: both or neither", fn, p->mean, p->rstd);
        if (int rc = check_tan_f32(fn, "mean", p->mean, false)) return rc;
        if (int rc = check_tan_f32(fn, "rstd", p->rstd, false)) return rc;
    }
    return after_dispatch(vivim::token_add_norm_dispatch(*p, false, as_stream(stream)), fn,
                          "%s not implemented for branch type %d / residual type %d", fn, p->btype, p->rtype);
}

size_t vivim_token_add_norm_bwd_workspace_bytes(const vivim_token_add_norm_params* p) {
    return p && p->rows > 0 && p->channels > 0 && p->channels <= kTlnMaxC ? vivim::token_add_norm_bwd_workspace_bytes(*p) : 0;
}

int vivim_token_add_norm_bwd(const vivim_token_add_norm_params* p, void* stream) {
    const char* fn = "token_add_norm_bwd";
    if (int rc = check_token_add_norm(p, fn)) return rc;
    const bool norm = p->weight != nullptr;
    const int C = p->channels;
    if (p->dy == nullptr && p->dres == nullptr) return fail(VIVIM_ERR_INVALID, "%s: dy and dres are both NULL: nothing to propagate", fn);
    if (!norm && p->dy != nullptr) return fail(VIVIM_ERR_INVALID, "%s: dy = %p without weight: the add alone has no y", fn, p->dy);
    if (norm) {
        if (int rc = check_tan_tensor(fn, "res_out", p->res_out, true, p->rtype, p->res_out_row_stride, C)) return rc;
        if (int rc = check_tan_f32(fn, "mean", p->mean, true)) return rc;
        if (int rc = check_tan_f32(fn, "rstd", p->rstd, true)) return rc;
        if (int rc = check_tan_f32(fn, "weight", p->weight, true)) return rc;
        if (int rc = check_tan_tensor(fn, "dy", p->dy, false, p->otype, p->dy_row_stride, C)) return rc;
        if (int rc = check_tan_f32(fn, "dweight", p->dweight, false)) return rc;
        if (int rc = check_tan_f32(fn, "dbias", p->dbias, false)) return rc;
        if (int rc = check_tan_f32(fn, "workspace", p->workspace, false)) return rc;
        if ((p->dweight || p->dbias) && !p->workspace)
            return fail(VIVIM_ERR_INVALID, "%s: dweight / dbias need the workspace (vivim_token_add_norm_bwd_workspace_bytes)", fn);
    }
    if (int rc = check_tan_tensor(fn, "dres", p->dres, false, p->rtype, p->dres_row_stride, C)) return rc;
    if (int rc = check_tan_tensor(fn, "dres_in", p->dres_in, false, p->rtype, p->dres_in_row_stride, C)) return rc;
    if (int rc = check_tan_tensor(fn, "dbranch", p->dbranch, false, p->btype, p->dbranch_row_stride, C)) return rc;
    if (int rc = check_tan_f32(fn, "scale", p->scale, false)) return rc;
    return after_dispatch(vivim::token_add_norm_dispatch(*p, true, as_stream(stream)), fn,
                          "%s not implemented for branch type %d / residual type %d", fn, p->btype, p->rtype);
}

}  // extern "C"
