// head_concat.hip -- the training decode head's upsample + dropout + concat and its transpose, one launch per direction
// (include/vivim_hip_ext_head.h: vivim_head_concat_params; the autograd wrapper is vivim_amd/head_concat.py).
//
// Up to four channels-last maps are upsampled to the output size with up_tap (up_tap.cuh), multiplied by keep * scale and written
// into their channel blocks of ONE channels-last tensor: what linear_fuse reads.  The arithmetic is upsample.hip's
// (upsample_cl_fwd_kernel / upsample_cl_bwd_kernel), in the same expression order with the fused multiply-adds spelled out, and
// one more product before the one rounding: 16-byte and element accesses give the same bits.
// A dropped element is a select, not a product: it is exactly 0 forward, and backward its dout is never multiplied (a NaN there
// stays out of dx).
//
// Forward: blockIdx.x = (n * OH + oh) * bpr + piece; lanes run along the contiguous (ow, channel-of-concat) axis.  A pixel is cut
// into units: map s gives C_s / E_s of them, E_s = 16 bytes of channels where that map's C_s, chan_off, the pixel stride, the bases
// and the batch strides allow (hc_vec: up_cl_vec's rule extended to the strided output and the mask) and one element otherwise.
// A thread owns one unit; the mask is read as E_s bytes.
// Backward: blockIdx.x decodes to (map, n, ih, piece) through per-map first-block counts.  The maps are laid out along the grid by
// descending window length (smallest map first): their threads walk the longest runs of dout, latency-bound, and start first, so
// the large maps' streaming work overlaps them.
// Per-map fields are picked with compile-time indices (hc_select): a runtime index into a kernel argument's arrays would go through
// scratch memory.
#include "capi.cuh"
#include "seg_load.cuh"
#include "up_tap.cuh"

namespace vivim {

constexpr int kHcThreads = 256;      // 4 waves per workgroup

// What a launch needs per map, in launch order: concat order forward, descending window length backward.  `first` is the map's first
// unit inside a pixel (forward) or its first workgroup (backward); `x` the map (forward) or its gradient (backward).
struct HcPlan {
    const void* x[4];
    const void* keep[4];
    int64_t x_bs[4], keep_bs[4];
    int32_t c[4], h[4], w[4], off[4], vec[4], first[4], bpr[4];
    float scale[4], rh[4], rw[4];
    int32_t n_maps, out_h, out_w, units;             // units of one output pixel (forward)
    int64_t out_bs, out_ps;
    const void* out;                                 // out (forward, written) or dout (backward)
};

struct HcMap {
    const void* x;
    const void* keep;
    int64_t x_bs, keep_bs;
    int32_t c, h, w, off, vec, first, bpr;
    float scale, rh, rw;
};

// the last map k < n_maps with first[k] <= key
__device__ __forceinline__ HcMap hc_select(const HcPlan& p, int key) {
    HcMap m{p.x[0], p.keep[0], p.x_bs[0], p.keep_bs[0], p.c[0], p.h[0], p.w[0], p.off[0], p.vec[0], p.first[0], p.bpr[0],
            p.scale[0], p.rh[0], p.rw[0]};
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k < p.n_maps && key >= p.first[k])
            m = HcMap{p.x[k], p.keep[k], p.x_bs[k], p.keep_bs[k], p.c[k], p.h[k], p.w[k], p.off[k], p.vec[k], p.first[k], p.bpr[k],
                      p.scale[k], p.rh[k], p.rw[k]};
    return m;
}

// E mask bytes at q (NULL: no mask) -> whether each element is kept
template <int E>
__device__ __forceinline__ void hc_keep(const uint8_t* __restrict__ q, bool (&kept)[E]) {
    if (q == nullptr) {
#pragma unroll
        for (int k = 0; k < E; ++k) kept[k] = true;
        return;
    }
    if constexpr (E == 1) {
        kept[0] = q[0] != 0;
    } else {
        static_assert(E % 4 == 0, "the mask is read in 32-bit words");
#pragma unroll
        for (int i = 0; i < E / 4; ++i) {
            const uint32_t v = reinterpret_cast<const uint32_t*>(q)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) kept[4 * i + j] = ((v >> (8 * j)) & 255u) != 0;
        }
    }
}

// one unit of the forward: E channels from channel c of map m at output pixel (n, oh, ow)
template <typename T, int E>
__device__ __forceinline__ void hc_fwd_unit(const HcPlan& p, const HcMap& m, int n, int oh, int ow, int c) {
    const int C = m.c, H = m.h, W = m.w, OW = p.out_w;
    const T* __restrict__ xb = static_cast<const T*>(m.x) + n * m.x_bs + c;
    bool kept[E];
    hc_keep<E>(m.keep ? static_cast<const uint8_t*>(m.keep) + n * m.keep_bs + ((oh * OW + ow) * C + c) : nullptr, kept);
    float y[E];
    if (H == p.out_h && W == OW) {                   // a map of the output's own size: no tap arithmetic
        unpack<T, E>(load_vec<T, E>(xb + (oh * W + ow) * C, true), y);
    } else {
        const UpTap th = up_tap(oh, m.rh, H), tw = up_tap(ow, m.rw, W);
        float a[E], b[E], d[E], e[E];
        unpack<T, E>(load_vec<T, E>(xb + (th.i0 * W + tw.i0) * C, true), a);
        unpack<T, E>(load_vec<T, E>(xb + (th.i0 * W + tw.i1) * C, true), b);
        unpack<T, E>(load_vec<T, E>(xb + (th.i1 * W + tw.i0) * C, true), d);
        unpack<T, E>(load_vec<T, E>(xb + (th.i1 * W + tw.i1) * C, true), e);
        // th.l0 * (tw.l0 * a + tw.l1 * b) + th.l1 * (tw.l0 * d + tw.l1 * e), upsample.hip's expression, with the fused multiply-adds
        // spelled out: a sum of two products can be contracted either way round, and the vector and the element instantiation must
        // form the same bits
#pragma unroll
        for (int k = 0; k < E; ++k)
            y[k] = fmaf(th.l0, fmaf(tw.l0, a[k], tw.l1 * b[k]), th.l1 * fmaf(tw.l0, d[k], tw.l1 * e[k]));
    }
#pragma unroll
    for (int k = 0; k < E; ++k) y[k] = kept[k] ? y[k] * m.scale : 0.0f;
    T* out = static_cast<T*>(const_cast<void*>(p.out));
    store_vec<T, E>(out + n * p.out_bs + (int64_t)(oh * OW + ow) * p.out_ps + m.off + c, true, y);
}

template <typename T>
__global__ void __launch_bounds__(kHcThreads) head_concat_fwd_kernel(const HcPlan p, const int bpr) {
    constexpr int EV = 16 / (int)sizeof(T);
    const int piece = blockIdx.x % bpr, row = blockIdx.x / bpr, n = row / p.out_h, oh = row - n * p.out_h;
    const int j = piece * kHcThreads + threadIdx.x;
    if (j >= p.out_w * p.units) return;
    const int ow = j / p.units, u = j - ow * p.units;
    const HcMap m = hc_select(p, u);
    if (m.vec) hc_fwd_unit<T, EV>(p, m, n, oh, ow, (u - m.first) * EV);
    else hc_fwd_unit<T, 1>(p, m, n, oh, ow, u - m.first);
}

// E channels of dout at output pixel `pix` of image n, each times keep * scale (a dropped one is 0 whatever dout holds)
template <typename T, int E>
__device__ __forceinline__ void hc_grad(const HcPlan& p, const HcMap& m, const T* __restrict__ gb, const uint8_t* __restrict__ kb, int pix,
                                        float (&g)[E]) {
    bool kept[E];
    hc_keep<E>(kb ? kb + pix * m.c : nullptr, kept);
    unpack<T, E>(load_vec<T, E>(gb + (int64_t)pix * p.out_ps, true), g);
#pragma unroll
    for (int k = 0; k < E; ++k) g[k] = kept[k] ? g[k] * m.scale : 0.0f;
}

// one unit of the backward: E channels from channel c of dx of map m at input pixel (n, ih, iw)
template <typename T, int E>
__device__ __forceinline__ void hc_bwd_unit(const HcPlan& p, const HcMap& m, int n, int ih, int iw, int c) {
    const int C = m.c, H = m.h, W = m.w, OH = p.out_h, OW = p.out_w;
    const T* __restrict__ gb = static_cast<const T*>(p.out) + n * p.out_bs + m.off + c;
    const uint8_t* __restrict__ kb = m.keep ? static_cast<const uint8_t*>(m.keep) + n * m.keep_bs + c : nullptr;
    float acc[E];
    if (H == OH && W == OW) {
        hc_grad<T, E>(p, m, gb, kb, ih * OW + iw, acc);
    } else {
        int hlo, hhi, wlo, whi;
        up_window(ih, H, OH, hlo, hhi);
        up_window(iw, W, OW, wlo, whi);
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = 0.0f;
        for (int oh = hlo; oh <= hhi; ++oh) {
            const UpTap th = up_tap(oh, m.rh, H);
            if (!up_hits(th, ih)) continue;
            float racc[E];
#pragma unroll
            for (int k = 0; k < E; ++k) racc[k] = 0.0f;
            for (int ow = wlo; ow <= whi; ++ow) {
                const UpTap tw = up_tap(ow, m.rw, W);
                if (!up_hits(tw, iw)) continue;
                const float ww = up_weight(tw, iw);
                float g[E];
                hc_grad<T, E>(p, m, gb, kb, oh * OW + ow, g);
#pragma unroll
                for (int k = 0; k < E; ++k) racc[k] = fmaf(ww, g[k], racc[k]);
            }
            const float wh = up_weight(th, ih);
#pragma unroll
            for (int k = 0; k < E; ++k) acc[k] = fmaf(wh, racc[k], acc[k]);
        }
    }
    T* dx = static_cast<T*>(const_cast<void*>(m.x));
    store_vec<T, E>(dx + n * m.x_bs + (ih * W + iw) * C + c, true, acc);
}

template <typename T>
__global__ void __launch_bounds__(kHcThreads) head_concat_bwd_kernel(const HcPlan p) {
    constexpr int EV = 16 / (int)sizeof(T);
    const HcMap m = hc_select(p, (int)blockIdx.x);
    const int local = (int)blockIdx.x - m.first;
    const int piece = local % m.bpr, row = local / m.bpr, n = row / m.h, ih = row - n * m.h;
    const int j = piece * kHcThreads + threadIdx.x;
    const int CV = m.vec ? m.c / EV : m.c;
    if (j >= m.w * CV) return;
    const int iw = j / CV, cu = j - iw * CV;
    if (m.vec) hc_bwd_unit<T, EV>(p, m, n, ih, iw, cu * EV);
    else hc_bwd_unit<T, 1>(p, m, n, ih, iw, cu);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int64_t hc_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// whether map s may move 16-byte vectors: its channels, its block's offset and the pixel stride whole numbers of them, every base
// and batch stride aligned, the mask readable in words of E bytes
static bool hc_vec(const vivim_head_concat_params& p, int s, bool bwd, int64_t elem) {
    const int64_t E = 16 / elem;
    if (p.map_c[s] % E || p.chan_off[s] % E || p.out_pixel_stride % E) return false;
    if (!sl_aligned16(bwd ? p.dout : p.out, elem, {p.out_batch_stride})) return false;
    if (!(bwd ? sl_aligned16(p.dmaps[s], elem, {p.dmap_batch_stride[s]}) : sl_aligned16(p.maps[s], elem, {p.map_batch_stride[s]})))
        return false;
    return p.keep[s] == nullptr || (reinterpret_cast<uintptr_t>(p.keep[s]) % E == 0 && p.keep_batch_stride[s] % E == 0);
}

// units of one output pixel (forward): every map's channels in vectors or elements
static int64_t hc_units(const vivim_head_concat_params& p, int64_t elem) {
    int64_t units = 0;
    for (int s = 0; s < p.n_maps; ++s) units += hc_vec(p, s, false, elem) ? p.map_c[s] / (16 / elem) : p.map_c[s];
    return units;
}

// workgroups of the launch (check_head_concat keeps it within a 31-bit grid)
static int64_t head_concat_blocks(const vivim_head_concat_params& p, bool bwd) {
    const int64_t elem = elem_bytes(p.itype);
    if (!bwd) return (int64_t)p.batch * p.out_h * hc_ceil_div(p.out_w * hc_units(p, elem), kHcThreads);
    int64_t blocks = 0;
    for (int s = 0; s < p.n_maps; ++s) {
        const int64_t cv = hc_vec(p, s, true, elem) ? p.map_c[s] / (16 / elem) : p.map_c[s];
        blocks += (int64_t)p.batch * p.map_h[s] * hc_ceil_div(p.map_w[s] * cv, kHcThreads);
    }
    return blocks;
}

template <typename T>
static void hc_launch(const vivim_head_concat_params& p, bool bwd, hipStream_t stream) {
    constexpr int64_t EV = 16 / (int64_t)sizeof(T);
    int order[4] = {0, 1, 2, 3};
    if (bwd)                                         // descending window length = ascending map area; ties keep concat order
        for (int i = 1; i < p.n_maps; ++i)
            for (int k = i; k > 0 && (int64_t)p.map_h[order[k]] * p.map_w[order[k]] < (int64_t)p.map_h[order[k - 1]] * p.map_w[order[k - 1]]; --k) {
                const int t = order[k];
                order[k] = order[k - 1];
                order[k - 1] = t;
            }
    HcPlan q{};
    q.n_maps = p.n_maps, q.out_h = p.out_h, q.out_w = p.out_w;
    q.out_bs = p.out_batch_stride, q.out_ps = p.out_pixel_stride;
    q.out = bwd ? p.dout : p.out;
    int64_t first = 0;
    for (int k = 0; k < p.n_maps; ++k) {
        const int s = order[k];
        const bool vec = hc_vec(p, s, bwd, sizeof(T));
        const int64_t cv = vec ? p.map_c[s] / EV : p.map_c[s];
        q.x[k] = bwd ? p.dmaps[s] : p.maps[s];
        q.keep[k] = p.keep[s];
        q.x_bs[k] = bwd ? p.dmap_batch_stride[s] : p.map_batch_stride[s];
        q.keep_bs[k] = p.keep_batch_stride[s];
        q.c[k] = p.map_c[s], q.h[k] = p.map_h[s], q.w[k] = p.map_w[s], q.off[k] = p.chan_off[s], q.vec[k] = vec ? 1 : 0;
        q.scale[k] = p.scale[s];
        // ATen's area_pixel_compute_scale: the ratio in fp32, on the host
        q.rh[k] = (float)p.map_h[s] / (float)p.out_h, q.rw[k] = (float)p.map_w[s] / (float)p.out_w;
        q.first[k] = (int32_t)first;
        q.bpr[k] = (int32_t)hc_ceil_div(p.map_w[s] * cv, kHcThreads);
        first += bwd ? (int64_t)p.batch * p.map_h[s] * q.bpr[k] : cv;
    }
    const dim3 block(kHcThreads);
    if (bwd) {
        hipLaunchKernelGGL(head_concat_bwd_kernel<T>, dim3((unsigned)first), block, 0, stream, q);
    } else {
        q.units = (int32_t)first;
        const int bpr = (int)hc_ceil_div(p.out_w * first, kHcThreads);
        hipLaunchKernelGGL(head_concat_fwd_kernel<T>, dim3((unsigned)((int64_t)p.batch * p.out_h * bpr)), block, 0, stream, q, bpr);
    }
}

static bool head_concat_dispatch(const vivim_head_concat_params& p, bool bwd, hipStream_t stream) {
    return with_itype(p.itype, [&](auto t) { hc_launch<decltype(t)>(p, bwd, stream); });
}

}  // namespace vivim

// ---- the C entry points
// every refusal the forward and the backward of the head concat share, before any launch
static int check_head_concat(const vivim_head_concat_params* p, const char* fn, bool bwd) {
    if (p == nullptr) return fail(VIVIM_ERR_INVALID, "%s: params is NULL", fn);
    if (int rc = check_struct_bytes(fn, "vivim_head_concat_params", p->struct_bytes, sizeof(*p))) return rc;
    if (p->n_maps < 1 || p->n_maps > 4) return fail(VIVIM_ERR_INVALID, "%s: n_maps = %d: one to four maps", fn, p->n_maps);
    if (!dtype_ok(p->itype)) return fail(VIVIM_ERR_INVALID, "%s: itype = %d: the maps are fp32 / fp16 / bf16 (0 / 1 / 2)", fn, p->itype);
    if (p->batch <= 0 || p->out_h <= 0 || p->out_w <= 0)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, out_h = %d, out_w = %d: every size must be positive", fn, p->batch, p->out_h, p->out_w);
    for (int s = 0; s < p->n_maps; ++s)
        if (p->map_c[s] <= 0 || p->map_h[s] <= 0 || p->map_w[s] <= 0)
            return fail(VIVIM_ERR_INVALID, "%s: map %d: map_c = %d, map_h = %d, map_w = %d: every size must be positive", fn, s, p->map_c[s],
                        p->map_h[s], p->map_w[s]);
    for (int s = 0; s < p->n_maps; ++s)
        if (p->map_h[s] > p->out_h || p->map_w[s] > p->out_w)
            return fail(VIVIM_ERR_UNSUPPORTED, "%s: map %d is (%d, %d), the output (%d, %d): upsampling only", fn, s, p->map_h[s], p->map_w[s],
                        p->out_h, p->out_w);
    for (int s = 0; s < p->n_maps; ++s) {
        if (p->chan_off[s] < 0 || (int64_t)p->chan_off[s] + p->map_c[s] > p->out_pixel_stride)
            return fail(VIVIM_ERR_INVALID, "%s: map %d: channels [%d, %lld) lie outside a pixel of out_pixel_stride = %lld", fn, s, p->chan_off[s],
                        (long long)p->chan_off[s] + p->map_c[s], (long long)p->out_pixel_stride);
        for (int t = 0; t < s; ++t)
            if (p->chan_off[s] < p->chan_off[t] + p->map_c[t] && p->chan_off[t] < p->chan_off[s] + p->map_c[s])
                return fail(VIVIM_ERR_INVALID, "%s: the channel blocks of maps %d and %d overlap: [%d, %d) and [%d, %d)", fn, t, s, p->chan_off[t],
                            p->chan_off[t] + p->map_c[t], p->chan_off[s], p->chan_off[s] + p->map_c[s]);
    }
    const uintptr_t ib = elem_bytes(p->itype);
    const void* big = bwd ? p->dout : p->out;
    if (big == nullptr || !aligned(big, ib))
        return fail(VIVIM_ERR_INVALID, "%s: %s at %p: need a %d-byte aligned pointer", fn, bwd ? "dout" : "out", big, (int)ib);
    for (int s = 0; s < p->n_maps; ++s) {
        const void* q = bwd ? p->dmaps[s] : p->maps[s];
        if (q == nullptr || !aligned(q, ib))
            return fail(VIVIM_ERR_INVALID, "%s: %s[%d] at %p: need a %d-byte aligned pointer", fn, bwd ? "dmaps" : "maps", s, q, (int)ib);
    }
    for (int s = 0; s < p->n_maps; ++s)
        if (!(p->scale[s] >= 1.0f) || p->scale[s] > FLT_MAX)                                      // NaN fails the first test
            return fail(VIVIM_ERR_INVALID, "%s: scale[%d] = %g: 1 / (1 - p) is finite and at least 1", fn, s, (double)p->scale[s]);
    // a batch holds its images one after the other without overlap
    const int64_t out_image = (int64_t)p->out_h * p->out_w * p->out_pixel_stride;
    if (p->out_batch_stride < out_image)
        return fail(VIVIM_ERR_INVALID, "%s: out_batch_stride = %lld: an image of out has %lld elements", fn, (long long)p->out_batch_stride,
                    (long long)out_image);
    for (int s = 0; s < p->n_maps; ++s) {
        const int64_t image = (int64_t)p->map_c[s] * p->map_h[s] * p->map_w[s], mask = (int64_t)p->map_c[s] * p->out_h * p->out_w;
        const int64_t have = bwd ? p->dmap_batch_stride[s] : p->map_batch_stride[s];
        if (have < image)
            return fail(VIVIM_ERR_INVALID, "%s: %s[%d] = %lld: an image of map %d has %lld elements", fn,
                        bwd ? "dmap_batch_stride" : "map_batch_stride", s, (long long)have, s, (long long)image);
        if (p->keep[s] != nullptr && p->keep_batch_stride[s] < mask)
            return fail(VIVIM_ERR_INVALID, "%s: keep_batch_stride[%d] = %lld: a mask of map %d has %lld bytes", fn, s,
                        (long long)p->keep_batch_stride[s], s, (long long)mask);
    }
    // the kernels index inside an image, and build their windows and their grid, with 32-bit integers
    // (a row's last workgroup counts up to kHcThreads - 1 positions past its end)
    bool fits = out_image <= INT32_MAX - vivim::kHcThreads && (int64_t)p->batch * p->out_h <= INT32_MAX;
    for (int s = 0; s < p->n_maps; ++s)
        fits = fits && (2 * (int64_t)p->map_h[s] + 3) * p->out_h <= INT32_MAX && (2 * (int64_t)p->map_w[s] + 3) * p->out_w <= INT32_MAX;
    if (!fits || vivim::head_concat_blocks(*p, bwd) > INT32_MAX)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, out (%d, %d), out_pixel_stride = %lld: the index range overflows int32", fn, p->batch,
                    p->out_h, p->out_w, (long long)p->out_pixel_stride);
    return VIVIM_OK;
}

extern "C" {

int vivim_head_concat_fwd(const vivim_head_concat_params* p, void* stream) {
    const char* fn = "head_concat_fwd";
    if (int rc = check_head_concat(p, fn, false)) return rc;
    return after_dispatch(vivim::head_concat_dispatch(*p, false, as_stream(stream)), fn, "%s not implemented for type %d", fn, p->itype);
}

int vivim_head_concat_bwd(const vivim_head_concat_params* p, void* stream) {
    const char* fn = "head_concat_bwd";
    if (int rc = check_head_concat(p, fn, true)) return rc;
    return after_dispatch(vivim::head_concat_dispatch(*p, true, as_stream(stream)), fn, "%s not implemented for type %d", fn, p->itype);
}

}  // extern "C"
