// decode_head.hip -- the eval-mode decode head behind its folded projections (include/vivim_hip.h: vivim_decode_head_params; the
// fold and the wrapper are vivim_amd/decode_head.py):
//     h[k] = max(0, bias[k] + sum over maps of the bilinear taps of m_s[k]),   logits[c] = b_out[c] + sum_k w_out[c][k] * h[k]
// per output pixel, fp32 throughout, rounded once.  The hidden vector h never leaves the chip: the only store is the logit.
//
// Tiling.  A workgroup of 4 waves owns an 8 x 8 tile of output pixels of one image, wave w the tile's rows w and w + 4: the
// pixels of a tile share their low-resolution taps (at most 5 x 5 + 3 x 3 + 2 x 2 pixels of maps at 1/2, 1/4, 1/8 of the
// output), so after the first pixel those reads hit L1 / L2, not HBM; there is no LDS stage for them.  A wave walks its 16 pixels;
// a pixel is wave-uniform, and so are its tap indices and weights (up_tap, the upsampling kernels' own function, formed again
// for every chunk: holding them for four maps costs more registers than the few instructions).  Lanes go along the hidden axis:
// lane l owns E consecutive channels of every chunk of 64 * E channels (E = 16 bytes of the map type when hidden and the
// addresses allow, one element otherwise), reads its E channels of every tap, forms h in registers, multiplies by its slice of
// w_out and adds into one partial sum per class.  After the last chunk the partial sums are reduced over the wave (wave_sum,
// a fixed butterfly) and lane c stores class c: one wave owns a logit and its order of additions is fixed.
// bias and w_out are copied to LDS once per workgroup (at most 9 rows of 1024 floats, 36 KiB: the limit on `hidden`), zero-padded
// to whole chunks and laid out so that a lane's E floats are E / 4 conflict-free 16-byte reads.  At 124 VGPRs (16-bit, E = 8)
// four workgroups share a CU: 16 waves, each with up to 13 16-byte loads per lane in flight.
// A map of the output's own size has r = 1, src = o, l1 = 0 on both axes: it is read with its one tap of weight 1.
// Measured at (15; 64^2 .. 8^2) bf16: 139 us.  Requesting the taps of all four maps before the first use (one memory round trip
// per chunk instead of one per map) costs 187 VGPRs, two waves per SIMD, and ran slower, 180 us: the kernel is not bound by
// the latency of a round trip.  12 of a pixel's 13 taps come from L2 (64 x 12 rows per tile where the tile's footprint is 38);
// staging that footprint in LDS is the open experiment.
#include "capi.cuh"
#include "seg_load.cuh"
#include "up_tap.cuh"

namespace vivim {

constexpr int kDhWaves = 4;
constexpr int kDhThreads = kDhWaves * kWave;
constexpr int kDhTile = 8;               // output pixels per tile edge; wave w owns rows w and w + 4
constexpr int kDhMaxHidden = 1024;       // check_decode_head refuses more
constexpr int kDhMaxClasses = 8;

struct DhRatios {
    float h[4], w[4];                    // ATen's area_pixel_compute_scale per map and axis, formed on the host in fp32
};

__device__ __forceinline__ int dh_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// where channel k of a row lies in LDS: chunk-major, then quarter (4 floats) of the lane's E, then lane
template <int E>
__device__ __forceinline__ int dh_lds_pos(int k) {
    if constexpr (E < 4) return k;
    constexpr int CH = kWave * E;
    const int chunk = k / CH, in = k - chunk * CH, lane = in / E, j = in - lane * E;
    return chunk * CH + (j / 4) * (kWave * 4) + lane * 4 + (j & 3);
}

// the lane's E floats of chunk `ch` of LDS row `row`
template <int E>
__device__ __forceinline__ void dh_lds_read(const float* row, int ch, int lane, float (&v)[E]) {
    if constexpr (E < 4) {
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = row[ch * kWave * E + lane * E + j];
    } else {
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
            const float4 f = *reinterpret_cast<const float4*>(row + ch * kWave * E + q * (kWave * 4) + lane * 4);
            v[4 * q] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
        }
    }
}

// blockIdx.x = (n * tiles_h + tile_h) * tiles_w + tile_w
template <typename T, int E>
__global__ void __launch_bounds__(kDhThreads) decode_head_kernel(const vivim_decode_head_params p, const DhRatios r, const int tiles_h,
                                                                  const int tiles_w) {
    __shared__ __attribute__((aligned(16))) float lds[(kDhMaxClasses + 1) * kDhMaxHidden];   // row 0: bias, row 1 + c: w_out[c]
    constexpr int CH = kWave * E;
    const int K = p.hidden, C = p.classes, OH = p.out_h, OW = p.out_w, tid = threadIdx.x;
    const int chunks = (K + CH - 1) / CH, Kp = chunks * CH;                               // Kp <= 1024
    {
        const float* __restrict__ bias = static_cast<const float*>(p.bias);
        const float* __restrict__ w_out = static_cast<const float*>(p.w_out);
        for (int i = tid; i < (C + 1) * Kp; i += kDhThreads) {
            const int row = i / Kp, k = i - row * Kp;
            const float v = k < K ? (row == 0 ? bias[k] : w_out[(row - 1) * K + k]) : 0.0f;
            lds[row * Kp + dh_lds_pos<E>(k)] = v;
        }
    }
    __syncthreads();

    const int tile_w = blockIdx.x % tiles_w, rest = blockIdx.x / tiles_w, tile_h = rest % tiles_h, n = rest / tiles_h;
    const int lane = tid & (kWave - 1), wave = dh_uniform(tid / kWave);
    const float* __restrict__ b_out = static_cast<const float*>(p.b_out);
    T* __restrict__ lb = static_cast<T*>(p.logits) + (int64_t)n * p.logits_batch_stride;

    for (int px = 0; px < kDhTile * kDhTile / kDhWaves; ++px) {
        // wave-uniform: the wave's rows are w, w + 4
        const int oh = tile_h * kDhTile + wave + (px / kDhTile) * kDhWaves, ow = tile_w * kDhTile + px % kDhTile;
        if (oh >= OH || ow >= OW) continue;
        float acc[kDhMaxClasses];
#pragma unroll
        for (int c = 0; c < kDhMaxClasses; ++c) acc[c] = 0.0f;
        for (int ch = 0; ch < chunks; ++ch) {
            const int k = ch * CH + lane * E;
            const bool in = k < K;                     // hidden % E == 0: a lane's E channels are all inside or all outside
            float h[E];
            dh_lds_read<E>(lds, ch, lane, h);           // the bias (0 in the padding)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (s >= p.n_maps) break;
                const T* __restrict__ mb = static_cast<const T*>(p.maps[s]) + (int64_t)n * p.map_batch_stride[s] + k;
                const int H = p.map_h[s], W = p.map_w[s];
                float a[E];
                if (H == OH && W == OW) {            // r = 1, src = o, l1 = 0 on both axes: the one tap of weight 1
                    unpack<T, E>(load_vec<T, E>(mb + (oh * OW + ow) * K, in), a);
#pragma unroll
                    for (int j = 0; j < E; ++j) h[j] += a[j];
                } else {
                    const UpTap th = up_tap(oh, r.h[s], H), tw = up_tap(ow, r.w[s], W);       // wave-uniform
                    float b[E], d[E], e[E];
                    unpack<T, E>(load_vec<T, E>(mb + (th.i0 * W + tw.i0) * K, in), a);
                    unpack<T, E>(load_vec<T, E>(mb + (th.i0 * W + tw.i1) * K, in), b);
                    unpack<T, E>(load_vec<T, E>(mb + (th.i1 * W + tw.i0) * K, in), d);
                    unpack<T, E>(load_vec<T, E>(mb + (th.i1 * W + tw.i1) * K, in), e);
#pragma unroll
                    for (int j = 0; j < E; ++j) h[j] += th.l0 * (tw.l0 * a[j] + tw.l1 * b[j]) + th.l1 * (tw.l0 * d[j] + tw.l1 * e[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < E; ++j) h[j] = fmaxf(h[j], 0.0f);
#pragma unroll
            for (int c = 0; c < kDhMaxClasses; ++c) {
                if (c >= C) break;
                float w[E];
                dh_lds_read<E>(lds + (c + 1) * Kp, ch, lane, w);
#pragma unroll
                for (int j = 0; j < E; ++j) acc[c] = fmaf(w[j], h[j], acc[c]);
            }
        }
        float mine = 0.0f;
#pragma unroll
        for (int c = 0; c < kDhMaxClasses; ++c) {
            if (c >= C) break;
            const float total = wave_sum(acc[c]);
            mine = lane == c ? total : mine;
        }
        if (lane < C) lb[(lane * OH + oh) * OW + ow] = from_f32<T>((b_out ? b_out[lane] : 0.0f) + mine);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// workgroups of the launch (check_decode_head keeps it within a 31-bit grid)
static int64_t decode_head_blocks(const vivim_decode_head_params& p) {
    return (int64_t)p.batch * ((p.out_h + kDhTile - 1) / kDhTile) * ((p.out_w + kDhTile - 1) / kDhTile);
}

// whether the maps may be read in 16-byte vectors: hidden a whole number of them, every base and batch stride aligned
static bool dh_vec(const vivim_decode_head_params& p, int64_t elem) {
    if (p.hidden % (16 / elem) != 0) return false;
    for (int s = 0; s < p.n_maps; ++s)
        if (!sl_aligned16(p.maps[s], elem, {p.map_batch_stride[s]})) return false;
    return true;
}

template <typename T, int E>
static void dh_launch_e(const vivim_decode_head_params& p, const DhRatios& r, hipStream_t stream) {
    const int tiles_h = (p.out_h + kDhTile - 1) / kDhTile, tiles_w = (p.out_w + kDhTile - 1) / kDhTile;
    hipLaunchKernelGGL((decode_head_kernel<T, E>), dim3((unsigned)decode_head_blocks(p)), dim3(kDhThreads), 0, stream, p, r, tiles_h,
                       tiles_w);
}

template <typename T>
static void dh_launch(const vivim_decode_head_params& p, hipStream_t stream) {
    DhRatios r = {};
    for (int s = 0; s < p.n_maps; ++s) {
        r.h[s] = (float)p.map_h[s] / (float)p.out_h;
        r.w[s] = (float)p.map_w[s] / (float)p.out_w;
    }
    if (dh_vec(p, sizeof(T))) dh_launch_e<T, 16 / (int)sizeof(T)>(p, r, stream);
    else dh_launch_e<T, 1>(p, r, stream);
}

static bool decode_head_dispatch(const vivim_decode_head_params& p, hipStream_t stream) {
    return with_itype(p.itype, [&](auto t) { dh_launch<decltype(t)>(p, stream); });
}

}  // namespace vivim

// ---- the C entry point
// every refusal of the fused decode head, before any launch
static int check_decode_head(const vivim_decode_head_params* p) {
    using vivim::kDhMaxHidden;
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes("decode_head_fwd", "vivim_decode_head_params", p->struct_bytes, sizeof(*p))) return rc;
    VCHECK(dtype_ok(p->itype));
    VCHECK(p->batch > 0 && p->hidden > 0 && p->classes > 0 && p->out_h > 0 && p->out_w > 0);
    VCHECK(p->n_maps >= 1 && p->n_maps <= 4);
    static_assert(vivim::kDhMaxClasses == 8, "the next check words the kernel's limit");
    VCHECK(p->classes <= 8);
    if (p->hidden > kDhMaxHidden)
        return fail(VIVIM_ERR_INVALID, "decode_head_fwd: hidden = %d: bias and w_out are kept in LDS, which holds up to %d channels",
                    p->hidden, kDhMaxHidden);
    const uintptr_t ib = elem_bytes(p->itype);
    // the kernel indexes inside an image, and builds its grid, with 32-bit integers
    VCHECK((int64_t)p->classes * p->out_h * p->out_w <= INT32_MAX);
    for (int s = 0; s < p->n_maps; ++s) {
        VCHECK(p->map_h[s] > 0 && p->map_w[s] > 0);
        if (p->map_h[s] > p->out_h || p->map_w[s] > p->out_w)
            return fail(VIVIM_ERR_UNSUPPORTED, "decode_head_fwd: map %d is (%d, %d), the output (%d, %d): upsampling only", s, p->map_h[s],
                        p->map_w[s], p->out_h, p->out_w);
        VCHECK((int64_t)p->hidden * p->map_h[s] * p->map_w[s] <= INT32_MAX);
    }
    for (int s = 0; s < p->n_maps; ++s) VCHECK(p->maps[s] != nullptr && aligned(p->maps[s], ib));
    VCHECK(p->bias != nullptr && aligned(p->bias, 4));
    VCHECK(p->w_out != nullptr && aligned(p->w_out, 4));
    VCHECK(aligned(p->b_out, 4));                                   // NULL: zeros
    VCHECK(p->logits != nullptr && aligned(p->logits, ib));
    for (int s = 0; s < p->n_maps; ++s) VCHECK(p->map_batch_stride[s] >= (int64_t)p->hidden * p->map_h[s] * p->map_w[s]);
    VCHECK(p->logits_batch_stride >= (int64_t)p->classes * p->out_h * p->out_w);
    VCHECK(vivim::decode_head_blocks(*p) <= INT32_MAX);
    return VIVIM_OK;
}

extern "C" int vivim_decode_head_fwd(const vivim_decode_head_params* p, void* stream) {
    if (int rc = check_decode_head(p)) return rc;
    return after_dispatch(vivim::decode_head_dispatch(*p, as_stream(stream)), "decode_head_fwd",
                          "decode_head_fwd not implemented for type %d", p->itype);
}
