// upsample.hip -- bilinear 2-D upsampling (align_corners = False, no explicit scale factors) and its gradient: the decode head's
// F.interpolate calls (include/vivim_hip.h: vivim_upsample_params; the autograd wrapper is vivim_amd/upsample.py).
//
// One tap function, up_tap (up_tap.cuh), turns an output index into (i0, i1, l0, l1) with ATen's fp32 arithmetic.  The forward reads four
// inputs through it; the backward is the same map transposed in GATHER form: a dx element looks at every output index that can
// tap it (up_window: a contiguous run, sized from the exact rational bounds plus two indices of slack for the fp32 rounding of
// the tap), recomputes that output's taps with up_tap itself and adds l0 where i0 is its own index and l1 where i1 is (at the
// bottom / right edge both are).  The terms are added in ascending output order by one thread: no atomics, no workspace, and
// the result is a pure function of the gradient and the shape.
//
// Four kernels.  Channels-last (dense NHWC memory): a thread owns E consecutive channels of one pixel, lanes run along the
// contiguous (w, c) axis, E = 16 bytes when C and the addresses allow and one element otherwise.  Planes (contiguous NCHW):
// lanes run along output columns, one workgroup per tile of an (n, c) plane; the backward is separable -- a vertical pass with
// lanes over output columns (coalesced reads of dy) into an fp32 LDS tile of kUpTileH input rows, then a horizontal pass out of
// LDS -- and walks a column window wider than the tile in chunks, in ascending order.
// Every grid is one-dimensional (blockIdx.x decoded on the scalar unit), so N * C planes are not bound by the y / z limits.
#include "capi.cuh"
#include "seg_load.cuh"
#include "up_tap.cuh"

namespace vivim {

constexpr int kUpThreads = 256;      // 4 waves per workgroup
constexpr int kUpFwdTileH = 16;      // planes forward: 64 output columns x 16 output rows per workgroup
constexpr int kUpTileW = 64;
constexpr int kUpTileH = 4;          // planes backward: 64 input columns x 4 input rows per workgroup
constexpr int kUpLdsW = 512;         // planes backward: output columns per LDS chunk

// ---- channels-last ------------------------------------------------------------------------------------------------------------
// blockIdx.x = (n * rows + row) * bpr + piece; a thread owns E channels of one pixel of that row
template <typename T, int E>
__global__ void __launch_bounds__(kUpThreads) upsample_cl_fwd_kernel(const vivim_upsample_params p, const float rh, const float rw,
                                                                      const int bpr) {
    const int C = p.channels, CV = C / E, H = p.in_h, W = p.in_w, OH = p.out_h, OW = p.out_w;
    const int piece = blockIdx.x % bpr, row = blockIdx.x / bpr, n = row / OH, oh = row - n * OH;
    const int j = piece * kUpThreads + threadIdx.x;
    if (j >= OW * CV) return;
    const int ow = j / CV, c = (j - ow * CV) * E;
    const UpTap th = up_tap(oh, rh, H), tw = up_tap(ow, rw, W);
    const T* __restrict__ xb = static_cast<const T*>(p.x) + (int64_t)n * p.x_batch_stride + c;
    float a[E], b[E], d[E], e[E], y[E];
    unpack<T, E>(load_vec<T, E>(xb + (th.i0 * W + tw.i0) * C, true), a);
    unpack<T, E>(load_vec<T, E>(xb + (th.i0 * W + tw.i1) * C, true), b);
    unpack<T, E>(load_vec<T, E>(xb + (th.i1 * W + tw.i0) * C, true), d);
    unpack<T, E>(load_vec<T, E>(xb + (th.i1 * W + tw.i1) * C, true), e);
#pragma unroll
    for (int k = 0; k < E; ++k) y[k] = th.l0 * (tw.l0 * a[k] + tw.l1 * b[k]) + th.l1 * (tw.l0 * d[k] + tw.l1 * e[k]);
    store_vec<T, E>(static_cast<T*>(p.y) + (int64_t)n * p.y_batch_stride + (oh * OW + ow) * C + c, true, y);
}

template <typename T, int E>
__global__ void __launch_bounds__(kUpThreads) upsample_cl_bwd_kernel(const vivim_upsample_params p, const float rh, const float rw,
                                                                      const int bpr) {
    const int C = p.channels, CV = C / E, H = p.in_h, W = p.in_w, OH = p.out_h, OW = p.out_w;
    const int piece = blockIdx.x % bpr, row = blockIdx.x / bpr, n = row / H, ih = row - n * H;
    const int j = piece * kUpThreads + threadIdx.x;
    if (j >= W * CV) return;
    const int iw = j / CV, c = (j - iw * CV) * E;
    int hlo, hhi, wlo, whi;
    up_window(ih, H, OH, hlo, hhi);
    up_window(iw, W, OW, wlo, whi);
    const T* __restrict__ gb = static_cast<const T*>(p.dy) + (int64_t)n * p.y_batch_stride + c;
    float acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = 0.0f;
    for (int oh = hlo; oh <= hhi; ++oh) {
        const UpTap th = up_tap(oh, rh, H);
        if (!up_hits(th, ih)) continue;
        float racc[E];
#pragma unroll
        for (int k = 0; k < E; ++k) racc[k] = 0.0f;
        for (int ow = wlo; ow <= whi; ++ow) {
            const UpTap tw = up_tap(ow, rw, W);
            if (!up_hits(tw, iw)) continue;
            const float ww = up_weight(tw, iw);
            float g[E];
            unpack<T, E>(load_vec<T, E>(gb + (oh * OW + ow) * C, true), g);
#pragma unroll
            for (int k = 0; k < E; ++k) racc[k] += ww * g[k];
        }
        const float wh = up_weight(th, ih);
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] += wh * racc[k];
    }
    store_vec<T, E>(static_cast<T*>(p.dx) + (int64_t)n * p.x_batch_stride + (ih * W + iw) * C + c, true, acc);
}

// ---- planes -------------------------------------------------------------------------------------------------------------------
// blockIdx.x = (plane * tiles_h + tile_h) * tiles_w + tile_w
template <typename T>
__global__ void __launch_bounds__(kUpThreads) upsample_pl_fwd_kernel(const vivim_upsample_params p, const float rh, const float rw,
                                                                      const int tiles_h, const int tiles_w) {
    const int C = p.channels, H = p.in_h, W = p.in_w, OH = p.out_h, OW = p.out_w;
    const int tw_i = blockIdx.x % tiles_w, rest = blockIdx.x / tiles_w, th_i = rest % tiles_h, plane = rest / tiles_h;
    const int n = plane / C, c = plane - n * C;
    const int ow = tw_i * kUpTileW + (threadIdx.x & (kUpTileW - 1)), ty = threadIdx.x / kUpTileW;
    if (ow >= OW) return;
    const T* __restrict__ xb = static_cast<const T*>(p.x) + (int64_t)n * p.x_batch_stride + c * (H * W);
    T* __restrict__ yb = static_cast<T*>(p.y) + (int64_t)n * p.y_batch_stride + c * (OH * OW);
    const UpTap tw = up_tap(ow, rw, W);
#pragma unroll
    for (int k = 0; k < kUpFwdTileH / (kUpThreads / kUpTileW); ++k) {
        const int oh = th_i * kUpFwdTileH + k * (kUpThreads / kUpTileW) + ty;
        if (oh >= OH) break;
        const UpTap th = up_tap(oh, rh, H);
        const float a = to_f32<T>(xb[th.i0 * W + tw.i0]), b = to_f32<T>(xb[th.i0 * W + tw.i1]);
        const float d = to_f32<T>(xb[th.i1 * W + tw.i0]), e = to_f32<T>(xb[th.i1 * W + tw.i1]);
        yb[oh * OW + ow] = from_f32<T>(th.l0 * (tw.l0 * a + tw.l1 * b) + th.l1 * (tw.l0 * d + tw.l1 * e));
    }
}

template <typename T>
__global__ void __launch_bounds__(kUpThreads) upsample_pl_bwd_kernel(const vivim_upsample_params p, const float rh, const float rw,
                                                                      const int tiles_h, const int tiles_w) {
    __shared__ float V[kUpTileH][kUpLdsW];       // V[r][ow - c0] = sum over oh of weight(oh, ih0 + r) * dy[oh][ow]
    const int C = p.channels, H = p.in_h, W = p.in_w, OH = p.out_h, OW = p.out_w, tid = threadIdx.x;
    const int tw_i = blockIdx.x % tiles_w, rest = blockIdx.x / tiles_w, th_i = rest % tiles_h, plane = rest / tiles_h;
    const int n = plane / C, c = plane - n * C;
    const T* __restrict__ gb = static_cast<const T*>(p.dy) + (int64_t)n * p.y_batch_stride + c * (OH * OW);
    const int ih0 = th_i * kUpTileH, iw0 = tw_i * kUpTileW;
    const int r = tid / kUpTileW, ih = ih0 + r, iw = iw0 + (tid & (kUpTileW - 1));
    const bool own = ih < H && iw < W;
    const int iw_last = iw0 + kUpTileW - 1 < W - 1 ? iw0 + kUpTileW - 1 : W - 1;
    int blk_lo, blk_hi, unused, wlo = 0, whi = -1;
    up_window(iw0, W, OW, blk_lo, unused);
    up_window(iw_last, W, OW, unused, blk_hi);
    if (own) up_window(iw, W, OW, wlo, whi);
    float acc = 0.0f;
    for (int c0 = blk_lo; c0 <= blk_hi; c0 += kUpLdsW) {
        const int cw = blk_hi - c0 + 1 < kUpLdsW ? blk_hi - c0 + 1 : kUpLdsW;
        for (int rr = 0; rr < kUpTileH && ih0 + rr < H; ++rr) {
            int hlo, hhi;
            up_window(ih0 + rr, H, OH, hlo, hhi);
            for (int col = tid; col < cw; col += kUpThreads) {
                float s = 0.0f;
                for (int oh = hlo; oh <= hhi; ++oh) {
                    const UpTap th = up_tap(oh, rh, H);
                    if (up_hits(th, ih0 + rr)) s += up_weight(th, ih0 + rr) * to_f32<T>(gb[oh * OW + c0 + col]);
                }
                V[rr][col] = s;
            }
        }
        __syncthreads();
        if (own) {
            const int a = wlo > c0 ? wlo : c0, b = whi < c0 + cw - 1 ? whi : c0 + cw - 1;
            for (int ow = a; ow <= b; ++ow) {
                const UpTap tw = up_tap(ow, rw, W);
                if (up_hits(tw, iw)) acc += up_weight(tw, iw) * V[r][ow - c0];
            }
        }
        __syncthreads();
    }
    if (own) static_cast<T*>(p.dx)[(int64_t)n * p.x_batch_stride + c * (H * W) + ih * W + iw] = from_f32<T>(acc);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int64_t up_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// whether the channels-last kernels may move 16-byte vectors: C a whole number of them, every base and batch stride aligned
static bool up_cl_vec(const vivim_upsample_params& p, bool bwd, int64_t elem) {
    if (p.channels % (16 / elem) != 0) return false;
    return sl_aligned16(bwd ? p.dx : p.x, elem, {p.x_batch_stride}) && sl_aligned16(bwd ? p.dy : p.y, elem, {p.y_batch_stride});
}

// workgroups of the launch (check_upsample keeps it within a 31-bit grid)
static int64_t upsample_blocks(const vivim_upsample_params& p, bool bwd) {
    if (p.layout == 1) {
        const int64_t elem = elem_bytes(p.itype), E = up_cl_vec(p, bwd, elem) ? 16 / elem : 1;
        const int64_t rows = bwd ? p.in_h : p.out_h, cols = bwd ? p.in_w : p.out_w;
        return (int64_t)p.batch * rows * up_ceil_div(cols * (p.channels / E), kUpThreads);
    }
    const int64_t planes = (int64_t)p.batch * p.channels;
    if (bwd) return planes * up_ceil_div(p.in_h, kUpTileH) * up_ceil_div(p.in_w, kUpTileW);
    return planes * up_ceil_div(p.out_h, kUpFwdTileH) * up_ceil_div(p.out_w, kUpTileW);
}

template <typename T, int E>
static void up_cl_launch(const vivim_upsample_params& p, bool bwd, float rh, float rw, hipStream_t stream) {
    const int cols = bwd ? p.in_w : p.out_w, bpr = (int)up_ceil_div((int64_t)cols * (p.channels / E), kUpThreads);
    const dim3 grid((unsigned)upsample_blocks(p, bwd)), block(kUpThreads);
    if (bwd) hipLaunchKernelGGL((upsample_cl_bwd_kernel<T, E>), grid, block, 0, stream, p, rh, rw, bpr);
    else hipLaunchKernelGGL((upsample_cl_fwd_kernel<T, E>), grid, block, 0, stream, p, rh, rw, bpr);
}

template <typename T>
static void up_launch(const vivim_upsample_params& p, bool bwd, hipStream_t stream) {
    // ATen's area_pixel_compute_scale: the ratio in fp32, on the host
    const float rh = (float)p.in_h / (float)p.out_h, rw = (float)p.in_w / (float)p.out_w;
    if (p.layout == 1) {
        if (up_cl_vec(p, bwd, sizeof(T))) up_cl_launch<T, 16 / (int)sizeof(T)>(p, bwd, rh, rw, stream);
        else up_cl_launch<T, 1>(p, bwd, rh, rw, stream);
        return;
    }
    const dim3 grid((unsigned)upsample_blocks(p, bwd)), block(kUpThreads);
    if (bwd)
        hipLaunchKernelGGL(upsample_pl_bwd_kernel<T>, grid, block, 0, stream, p, rh, rw, (int)up_ceil_div(p.in_h, kUpTileH),
                           (int)up_ceil_div(p.in_w, kUpTileW));
    else
        hipLaunchKernelGGL(upsample_pl_fwd_kernel<T>, grid, block, 0, stream, p, rh, rw, (int)up_ceil_div(p.out_h, kUpFwdTileH),
                           (int)up_ceil_div(p.out_w, kUpTileW));
}

static bool upsample_dispatch(const vivim_upsample_params& p, bool bwd, hipStream_t stream) {
    return with_itype(p.itype, [&](auto t) { up_launch<decltype(t)>(p, bwd, stream); });
}

}  // namespace vivim

// ---- the C entry points
// every refusal of the upsampling calls, before any launch
static int check_upsample(const vivim_upsample_params* p, bool bwd) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && (p->layout == 0 || p->layout == 1));
    VCHECK(p->batch > 0 && p->channels > 0 && p->in_h > 0 && p->in_w > 0 && p->out_h > 0 && p->out_w > 0);
    if (p->out_h < p->in_h || p->out_w < p->in_w)
        return fail(VIVIM_ERR_UNSUPPORTED, "upsample_bilinear2d: (%d, %d) -> (%d, %d): upsampling only", p->in_h, p->in_w, p->out_h,
                    p->out_w);
    const uintptr_t ib = elem_bytes(p->itype);
    const void* src = bwd ? p->dy : p->x;
    const void* dst = bwd ? p->dx : p->y;
    VCHECK(src != nullptr && aligned(src, ib));
    VCHECK(dst != nullptr && aligned(dst, ib));
    // the kernels above index inside an image, and build their windows (up_window) and their grid, with 32-bit integers
    VCHECK((int64_t)p->channels * p->in_h * p->in_w <= INT32_MAX && (int64_t)p->channels * p->out_h * p->out_w <= INT32_MAX);
    VCHECK((2 * (int64_t)p->in_h + 3) * p->out_h <= INT32_MAX && (2 * (int64_t)p->in_w + 3) * p->out_w <= INT32_MAX);
    VCHECK((int64_t)p->batch * p->channels <= INT32_MAX && (int64_t)p->batch * p->out_h <= INT32_MAX);
    VCHECK(vivim::upsample_blocks(*p, bwd) <= INT32_MAX);
    return VIVIM_OK;
}

extern "C" {

int vivim_upsample_bilinear2d_fwd(const vivim_upsample_params* p, void* stream) {
    if (int rc = check_upsample(p, false)) return rc;
    return after_dispatch(vivim::upsample_dispatch(*p, false, as_stream(stream)), "upsample_bilinear2d_fwd",
                          "upsample_bilinear2d_fwd not implemented for type %d", p->itype);
}

int vivim_upsample_bilinear2d_bwd(const vivim_upsample_params* p, void* stream) {
    if (int rc = check_upsample(p, true)) return rc;
    return after_dispatch(vivim::upsample_dispatch(*p, true, as_stream(stream)), "upsample_bilinear2d_bwd",
                          "upsample_bilinear2d_bwd not implemented for type %d", p->itype);
}

}  // extern "C"
