// binary_metrics.hip -- validation metrics of the binary recipe on the device (include/vivim_hip_ext_binary_metrics.h; the
// definition is the docstring of vivim_amd/binary_metrics.py, whose eager composition computes the same): per image the
// 256-threshold sweep of six confusion metrics, S-measure, mean E-measure and MAE of a probability map against a mask.
//
// Everything is a reduction over one map and one mask, in five launches on one stream:
//   1 bm_stats_kernel     per (image, block): min / max of p, |g|, the integer row and column sums of g -> its slot; the block
//                         also zeroes its share of the image's four global histograms
//   2 bm_moments_kernel   adds its image's stats slots in slot order (-> mn, mx, centroid), then per pixel: pn, the sweep bin and
//                         the E bin into four LDS histograms (integer atomics), and the fp64 first moments sum|pn - g|, sum pn over
//                         g, sum (1 - pn) over ~g, per quadrant sum pn and sum g -> its slot; the LDS histograms are added to
//                         the image's global ones with integer atomics (order-free, so bit-repeatable)
//   3 bm_centred_kernel   forms the means from the slots of 2, then the CENTRED second moments around them -> its slot.  Means
//                         first: a region where pn is constant has sums that are exact in fp64, so its mean is that constant
//                         and its variance and covariance are exactly 0 -- E[x^2] - mean^2 would leave rounding noise there and
//                         flip the ssim branch
//   4 bm_image_kernel     one workgroup per image: adds the slots in slot order, takes the flipped cumulative sums of the
//                         histograms, evaluates the formulas in fp64, writes values[n][0..9) (and the histograms if asked)
//   5 bm_state_kernel     state[k] += values[n][k] for n ascending
// No float atomics; fp64 partial sums meet in a fixed order (xor butterfly inside a wave, waves in order, slots in order).  A
// thread owns E consecutive pixels (16 bytes of pred) per step and loads them as vectors where the address allows.
#include "capi.cuh"

namespace vivim {

constexpr int kBmThreads = 256;
constexpr int kBmWaves = kBmThreads / kWave;
constexpr int kBmMaxBlocks = 32;     // workgroups per image (grid-stride loop beyond)
constexpr int kBmBins = 256;
constexpr int kBmM1 = 11;            // doubles per slot of launch 2: mae, fg, bg, quadrant sum pn [4], quadrant sum g [4]
constexpr int kBmM2 = 10;            // of launch 3: fg, bg, quadrant sum dx^2 [4], quadrant sum dx dy [4]
constexpr double kBmEps = 2.220446049250313e-16;       // numpy.spacing(1)

struct BmStatSlot {
    float mn, mx;
    int32_t G, pad;
    int64_t srow, scol;
};

static int bm_blocks_per_image(const vivim_binary_metrics_params& p) {
    const int64_t per_block = (int64_t)kBmThreads * vec_elems(p.ptype);
    const int64_t b = ((int64_t)p.height * p.width + per_block - 1) / per_block;
    return (int)(b < kBmMaxBlocks ? b : kBmMaxBlocks);
}

// the workspace: stats slots | histograms | slots of launch 2 | slots of launch 3, each 8-byte aligned
struct BmLayout {
    size_t stats, hist, m1, m2, total;
};
static BmLayout bm_layout(const vivim_binary_metrics_params& p) {
    const size_t slots = (size_t)p.batch * bm_blocks_per_image(p);
    BmLayout L;
    L.stats = 0;
    L.hist = L.stats + slots * sizeof(BmStatSlot);
    L.m1 = L.hist + (size_t)p.batch * 4 * kBmBins * sizeof(int32_t);
    L.m2 = L.m1 + slots * kBmM1 * sizeof(double);
    L.total = L.m2 + slots * kBmM2 * sizeof(double);
    return L;
}

static size_t binary_metrics_workspace_bytes(const vivim_binary_metrics_params& p) { return bm_layout(p).total; }

// what the kernels get besides the params: the parts of the workspace
struct BmWs {
    BmStatSlot* stats;
    int32_t* hist;
    double* m1;
    double* m2;
    int bpi;
};

template <typename V> __device__ __forceinline__ V bm_wave_sum(V v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// the sums of K per-thread values over the workgroup, in a fixed order; valid in thread 0 afterwards
template <typename V, int K> __device__ __forceinline__ void bm_block_sums(V (&v)[K], V (*red)[kBmWaves]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    __syncthreads();                             // red may still be read from an earlier use
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const V s = bm_wave_sum(v[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        V s = red[k][0];
#pragma unroll
        for (int w = 1; w < kBmWaves; ++w) s += red[k][w];
        v[k] = s;
    }
}

// E pixels of pred and of the mask; pixels >= nv read as p = 0, g = false
template <typename T, int E>
__device__ __forceinline__ void bm_load(const vivim_binary_metrics_params& p, int n, int64_t pix0, int nv, float (&x)[E], bool (&g)[E]) {
    load_k<T, E>(static_cast<const T*>(p.pred) + (int64_t)n * p.pred_batch_stride + pix0, nv, x);
    float m[E];
    const int64_t off = (int64_t)n * p.gt_batch_stride + pix0;
    switch (p.gtype) {
        case VIVIM_F32: load_k<float, E>(static_cast<const float*>(p.gt) + off, nv, m); break;
        case VIVIM_F16: load_k<f16_t, E>(static_cast<const f16_t*>(p.gt) + off, nv, m); break;
        case VIVIM_BF16: load_k<bf16_t, E>(static_cast<const bf16_t*>(p.gt) + off, nv, m); break;
        default: load_k<uint8_t, E>(static_cast<const uint8_t*>(p.gt) + off, nv, m); break;
    }
#pragma unroll
    for (int k = 0; k < E; ++k) g[k] = m[k] > 0.5f;             // a nonzero byte widens to >= 1
}

// what launches 2 to 4 know of an image after adding its stats slots in slot order
struct BmImage {
    float mn, d;         // pn = (p - mn) / d when norm
    bool norm;           // mx != mn
    int G, X, Y;         // |g| and the centroid + 1: the quadrants split at column X and row Y
};

__device__ __forceinline__ BmImage bm_image(const vivim_binary_metrics_params& p, const BmWs& w, int n) {
    const BmStatSlot* __restrict__ s = w.stats + (int64_t)n * w.bpi;
    float mn = s[0].mn, mx = s[0].mx;
    int64_t G = s[0].G, srow = s[0].srow, scol = s[0].scol;
    for (int b = 1; b < w.bpi; ++b) {
        mn = fminf(mn, s[b].mn);
        mx = fmaxf(mx, s[b].mx);
        G += s[b].G;
        srow += s[b].srow;
        scol += s[b].scol;
    }
    BmImage im;
    im.mn = mn;
    im.norm = mx != mn;
    im.d = __fsub_rn(mx, mn);
    im.G = (int)G;
    // numpy.round is round-half-even, as rint; an empty mask takes the middle (never used: its S-measure is 1 - mean)
    const double cx = G > 0 ? (double)scol / (double)G : 0.5 * p.width, cy = G > 0 ? (double)srow / (double)G : 0.5 * p.height;
    const int X = (int)rint(cx) + 1, Y = (int)rint(cy) + 1;
    im.X = X < 1 ? 1 : (X > p.width ? p.width : X);             // already in range for every G > 0; the clamp is for G == 0
    im.Y = Y < 1 ? 1 : (Y > p.height ? p.height : Y);
    return im;
}

__device__ __forceinline__ float bm_norm(const BmImage& im, float p) { return im.norm ? __fdiv_rn(__fsub_rn(p, im.mn), im.d) : p; }

template <typename T>
__global__ void __launch_bounds__(kBmThreads) bm_stats_kernel(const vivim_binary_metrics_params p, const BmWs w) {
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ float fred[2][kBmWaves];
    __shared__ int64_t ired[3][kBmWaves];
    const int n = blockIdx.x / w.bpi, blk = blockIdx.x - n * w.bpi, W = p.width;
    const int64_t HW = (int64_t)p.height * W;
    for (int i = blk * kBmThreads + threadIdx.x; i < 4 * kBmBins; i += w.bpi * kBmThreads) w.hist[(int64_t)n * 4 * kBmBins + i] = 0;
    float mn = INFINITY, mx = -INFINITY;
    int64_t cnt[3] = {0, 0, 0};                  // |g|, sum of rows, sum of columns
    for (int64_t pix0 = ((int64_t)blk * kBmThreads + threadIdx.x) * E; pix0 < HW; pix0 += (int64_t)w.bpi * kBmThreads * E) {
        const int nv = (int)(HW - pix0 < E ? HW - pix0 : E);
        float x[E];
        bool g[E];
        bm_load<T, E>(p, n, pix0, nv, x, g);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if (k < nv) {
                mn = fminf(mn, x[k]);
                mx = fmaxf(mx, x[k]);
                const int pix = (int)pix0 + k, row = pix / W, col = pix - row * W;
                cnt[0] += g[k] ? 1 : 0;
                cnt[1] += g[k] ? row : 0;
                cnt[2] += g[k] ? col : 0;
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, kWave));
        mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
    }
    if (lane == 0) {
        fred[0][wave] = mn;
        fred[1][wave] = mx;
    }
    bm_block_sums<int64_t, 3>(cnt, ired);        // its barriers order the writes of fred as well
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 1; v < kBmWaves; ++v) {
            mn = fminf(mn, fred[0][v]);
            mx = fmaxf(mx, fred[1][v]);
        }
        BmStatSlot s;
        s.mn = mn;
        s.mx = mx;
        s.G = (int32_t)cnt[0];
        s.pad = 0;
        s.srow = cnt[1];
        s.scol = cnt[2];
        w.stats[blockIdx.x] = s;
    }
}

// the number of thresholds that p exceeds: a candidate from arithmetic, corrected against the table (asc[k] = the k-th
// threshold in ASCENDING order).  b is the one value with p > asc[b - 1] and not p > asc[b]; a NaN exceeds none.
__device__ __forceinline__ int bm_sweep_bin(float p, const float* asc) {
    int b = (int)fminf(fmaxf(p * 255.0f, 0.0f), 256.0f);
    while (b < kBmBins && p > asc[b]) ++b;
    while (b > 0 && !(p > asc[b - 1])) --b;
    return b;
}

template <typename T>
__global__ void __launch_bounds__(kBmThreads) bm_moments_kernel(const vivim_binary_metrics_params p, const BmWs w) {
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ int hist[4 * kBmBins];
    __shared__ float asc[kBmBins];
    __shared__ double red[kBmM1][kBmWaves];
    const int n = blockIdx.x / w.bpi, blk = blockIdx.x - n * w.bpi, W = p.width;
    const int64_t HW = (int64_t)p.height * W;
    for (int i = threadIdx.x; i < 4 * kBmBins; i += kBmThreads) hist[i] = 0;
    for (int i = threadIdx.x; i < kBmBins; i += kBmThreads) asc[i] = static_cast<const float*>(p.thresholds)[kBmBins - 1 - i];
    const BmImage im = bm_image(p, w, n);
    __syncthreads();
    double acc[kBmM1];
#pragma unroll
    for (int i = 0; i < kBmM1; ++i) acc[i] = 0.0;
    for (int64_t pix0 = ((int64_t)blk * kBmThreads + threadIdx.x) * E; pix0 < HW; pix0 += (int64_t)w.bpi * kBmThreads * E) {
        const int nv = (int)(HW - pix0 < E ? HW - pix0 : E);
        float x[E];
        bool g[E];
        bm_load<T, E>(p, n, pix0, nv, x, g);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if (k < nv) {
                const float pn = bm_norm(im, x[k]);
                const int b = bm_sweep_bin(x[k], asc);
                if (b > 0) atomicAdd(&hist[(g[k] ? 0 : kBmBins) + b - 1], 1);
                // uint8(pn * 255): truncated; the clamp only acts on a constant map outside [0, 1], where numpy's cast is undefined
                const int e = (int)fminf(fmaxf(__fmul_rn(pn, 255.0f), 0.0f), 255.0f);
                atomicAdd(&hist[(g[k] ? 2 : 3) * kBmBins + e], 1);
                const double v = (double)pn, gd = g[k] ? 1.0 : 0.0;
                acc[0] += fabs(v - gd);
                acc[1] += g[k] ? v : 0.0;
                acc[2] += g[k] ? 0.0 : 1.0 - v;
                const int pix = (int)pix0 + k, row = pix / W, col = pix - row * W;
                const int q = (row >= im.Y ? 2 : 0) + (col >= im.X ? 1 : 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[3 + j] += q == j ? v : 0.0;
                    acc[7 + j] += q == j ? gd : 0.0;
                }
            }
        }
    }
    bm_block_sums<double, kBmM1>(acc, red);      // its first barrier also ends the LDS atomics
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kBmM1; ++i) w.m1[(int64_t)blockIdx.x * kBmM1 + i] = acc[i];
    }
    for (int i = threadIdx.x; i < 4 * kBmBins; i += kBmThreads)
        if (hist[i] != 0) atomicAdd(&w.hist[(int64_t)n * 4 * kBmBins + i], hist[i]);
}

// the slots of launch 2 (or 3) of image n added in slot order: component i by thread i, into LDS
template <int K> __device__ __forceinline__ void bm_add_slots(const double* __restrict__ slots, int n, int bpi, double* out) {
    if (threadIdx.x < K) {
        const double* __restrict__ s = slots + (int64_t)n * bpi * K + threadIdx.x;
        double a = s[0];
        for (int b = 1; b < bpi; ++b) a += s[(int64_t)b * K];
        out[threadIdx.x] = a;
    }
}

// the pixel counts of the four quadrants (left-top, right-top, left-bottom, right-bottom)
__device__ __forceinline__ void bm_quadrant_sizes(const vivim_binary_metrics_params& p, const BmImage& im, double (&nq)[4]) {
    nq[0] = (double)im.X * im.Y;
    nq[1] = (double)(p.width - im.X) * im.Y;
    nq[2] = (double)im.X * (p.height - im.Y);
    nq[3] = (double)(p.width - im.X) * (p.height - im.Y);
}

template <typename T>
__global__ void __launch_bounds__(kBmThreads) bm_centred_kernel(const vivim_binary_metrics_params p, const BmWs w) {
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ double m1[kBmM1];
    __shared__ double mean[10];                  // fg, bg, quadrant mean of pn [4], of g [4]
    __shared__ double red[kBmM2][kBmWaves];
    const int n = blockIdx.x / w.bpi, blk = blockIdx.x - n * w.bpi, W = p.width;
    const int64_t HW = (int64_t)p.height * W;
    const BmImage im = bm_image(p, w, n);
    bm_add_slots<kBmM1>(w.m1, n, w.bpi, m1);
    __syncthreads();
    if (threadIdx.x == 0) {
        double nq[4];
        bm_quadrant_sizes(p, im, nq);
        mean[0] = m1[1] / (double)im.G;          // 0 / 0 for an empty or a full mask: never used then
        mean[1] = m1[2] / (double)(HW - im.G);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mean[2 + j] = m1[3 + j] / nq[j];
            mean[6 + j] = m1[7 + j] / nq[j];
        }
    }
    __syncthreads();
    double acc[kBmM2];
#pragma unroll
    for (int i = 0; i < kBmM2; ++i) acc[i] = 0.0;
    for (int64_t pix0 = ((int64_t)blk * kBmThreads + threadIdx.x) * E; pix0 < HW; pix0 += (int64_t)w.bpi * kBmThreads * E) {
        const int nv = (int)(HW - pix0 < E ? HW - pix0 : E);
        float x[E];
        bool g[E];
        bm_load<T, E>(p, n, pix0, nv, x, g);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if (k < nv) {
                const double v = (double)bm_norm(im, x[k]), gd = g[k] ? 1.0 : 0.0;
                const double dfg = v - mean[0], dbg = (1.0 - v) - mean[1];
                acc[0] += g[k] ? dfg * dfg : 0.0;
                acc[1] += g[k] ? 0.0 : dbg * dbg;
                const int pix = (int)pix0 + k, row = pix / W, col = pix - row * W;
                const int q = (row >= im.Y ? 2 : 0) + (col >= im.X ? 1 : 0);
                const double dx = v - mean[2 + q], dy = gd - mean[6 + q];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[2 + j] += q == j ? dx * dx : 0.0;
                    acc[6 + j] += q == j ? dx * dy : 0.0;
                }
            }
        }
    }
    bm_block_sums<double, kBmM2>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kBmM2; ++i) w.m2[(int64_t)blockIdx.x * kBmM2 + i] = acc[i];
    }
}

// S-measure of one image from its moments (alpha = 0.5).  NaN where the reference's arithmetic yields NaN (a quadrant of fewer
// than 2 pixels, |g| == 1, |~g| == 1): the caller turns that into 0, which is what the reference's max(0, nan) returns.
__device__ double bm_smeasure(const vivim_binary_metrics_params& p, const BmImage& im, const double* m1, const double* m2) {
    const double S = (double)p.height * p.width, G = (double)im.G;
    double nq[4];
    bm_quadrant_sizes(p, im, nq);
    const double total = ((m1[3] + m1[4]) + m1[5]) + m1[6];
    if (im.G == 0) return 1.0 - total / S;
    if (G == S) return total / S;
    const double y = G / S;
    const double xf = m1[1] / G, sf = sqrt(m2[0] / (G - 1.0));
    const double xb = m1[2] / (S - G), sb = sqrt(m2[1] / (S - G - 1.0));
    const double object = y * (2.0 * xf / (xf * xf + 1.0 + sf + kBmEps)) + (1.0 - y) * (2.0 * xb / (xb * xb + 1.0 + sb + kBmEps));
    double score[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double N = nq[j], x = m1[3 + j] / N, gq = m1[7 + j], yq = gq / N;
        const double sx = m2[2 + j] / (N - 1.0), sxy = m2[6 + j] / (N - 1.0);
        const double sy = (gq * ((1.0 - yq) * (1.0 - yq)) + (N - gq) * (yq * yq)) / (N - 1.0);     // sum (g - yq)^2 of a 0 / 1 map
        const double alpha = 4.0 * x * yq * sxy, beta = (x * x + yq * yq) * (sx + sy);
        score[j] = alpha != 0.0 ? alpha / (beta + kBmEps) : (beta == 0.0 ? 1.0 : 0.0);            // a NaN alpha != 0: NaN
    }
    const double w1 = nq[0] / S, w2 = nq[1] / S, w3 = nq[2] / S, w4 = 1.0 - w1 - w2 - w3;
    const double region = w1 * score[0] + w2 * score[1] + w3 * score[2] + w4 * score[3];
    const double sm = 0.5 * object + 0.5 * region;
    return sm > 0.0 ? sm : 0.0;                  // max(0, sm); a NaN compares false: 0
}

__global__ void __launch_bounds__(kBmThreads) bm_image_kernel(const vivim_binary_metrics_params p, const BmWs w) {
    __shared__ int h[4 * kBmBins];
    __shared__ double m1[kBmM1];
    __shared__ double m2[kBmM2];
    __shared__ double vals[7][kBmBins];
    const int n = blockIdx.x, j = threadIdx.x;
    const BmImage im = bm_image(p, w, n);
    for (int i = j; i < 4 * kBmBins; i += kBmThreads) {
        h[i] = w.hist[(int64_t)n * 4 * kBmBins + i];
        if (p.hist) static_cast<int32_t*>(p.hist)[(int64_t)n * 4 * kBmBins + i] = h[i];
    }
    bm_add_slots<kBmM1>(w.m1, n, w.bpi, m1);
    bm_add_slots<kBmM2>(w.m2, n, w.bpi, m2);
    __syncthreads();
    // threshold j: the flipped cumulative sums, then the six sweep metrics and the enhanced-alignment value
    int64_t c[4] = {0, 0, 0, 0};
    for (int i = kBmBins - 1 - j; i < kBmBins; ++i) {
#pragma unroll
        for (int a = 0; a < 4; ++a) c[a] += h[a * kBmBins + i];
    }
    const int64_t Si = (int64_t)p.height * p.width, Gi = im.G;
    const double S = (double)Si, G = (double)Gi;
    {
        const double tp = (double)c[0], fp = (double)c[1], fn = (double)(Gi - c[0]), tn = (double)(Si - Gi - c[1]);
        const bool test_empty = c[0] + c[1] == 0, ref_empty = Gi == 0, ref_full = Gi == Si;
        const bool both = test_empty && ref_empty;
        const double prec = test_empty ? 0.0 : tp / (tp + fp), rec = ref_empty ? 0.0 : tp / (tp + fn);
        vals[0][j] = both ? 0.0 : 2.0 * tp / (2.0 * tp + fp + fn);
        vals[1][j] = both ? 0.0 : tp / (tp + fp + fn);
        vals[2][j] = prec;
        vals[3][j] = rec;
        vals[4][j] = 2.0 * prec * rec / (prec + rec + 1e-5);
        vals[5][j] = ref_full ? 0.0 : tn / (tn + fp);
    }
    {
        const double fg_fg = (double)c[2], fg_bg = (double)c[3], pred_fg = (double)(c[2] + c[3]), pred_bg = (double)(Si - c[2] - c[3]);
        double sum;
        if (Gi == 0) {
            sum = pred_bg;
        } else if (Gi == Si) {
            sum = pred_fg;
        } else {
            const double bg_fg = G - fg_fg, bg_bg = pred_bg - bg_fg;
            const double mp = pred_fg / S, mg = G / S;
            const double a[2] = {1.0 - mp, 0.0 - mp}, b[2] = {1.0 - mg, 0.0 - mg};
            const double numel[4] = {fg_fg, fg_bg, bg_fg, bg_bg};
            sum = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double x = a[k >> 1], y = b[k & 1];
                const double align = 2.0 * (x * y) / (x * x + y * y + kBmEps);
                sum += (align + 1.0) * (align + 1.0) / 4.0 * numel[k];
            }
        }
        vals[6][j] = sum / (S - 1.0 + kBmEps);
    }
    __syncthreads();
    double* __restrict__ out = static_cast<double*>(p.values) + (int64_t)n * 9;
    if (j < 7) {                                 // the sequential sum over the thresholds, divided by 256
        double s = 0.0;
        for (int i = 0; i < kBmBins; ++i) s += vals[j][i];
        out[j < 6 ? j : 7] = s / 256.0;
    } else if (j == 7) {
        const double sm = bm_smeasure(p, im, m1, m2);
        out[6] = sm == sm ? sm : 0.0;
    } else if (j == 8) {
        out[8] = m1[0] / S;
    }
}

__global__ void __launch_bounds__(kWave) bm_state_kernel(const vivim_binary_metrics_params p) {
    double* __restrict__ st = static_cast<double*>(p.state);
    const double* __restrict__ v = static_cast<const double*>(p.values);
    const int k = threadIdx.x;
    if (k < 9) {
        double s = st[k];
        for (int64_t n = 0; n < p.batch; ++n) s += v[n * 9 + k];
        st[k] = s;
    } else if (k == 9) {
        st[9] += (double)p.batch;
    }
}

template <typename T> static void bm_launch(const vivim_binary_metrics_params& p, const BmWs& w, hipStream_t stream) {
    const dim3 grid((unsigned)((int64_t)p.batch * w.bpi)), block(kBmThreads);
    hipLaunchKernelGGL(bm_stats_kernel<T>, grid, block, 0, stream, p, w);
    hipLaunchKernelGGL(bm_moments_kernel<T>, grid, block, 0, stream, p, w);
    hipLaunchKernelGGL(bm_centred_kernel<T>, grid, block, 0, stream, p, w);
    hipLaunchKernelGGL(bm_image_kernel, dim3((unsigned)p.batch), block, 0, stream, p, w);
    if (p.state) hipLaunchKernelGGL(bm_state_kernel, dim3(1), dim3(kWave), 0, stream, p);
}

static bool binary_metrics_dispatch(const vivim_binary_metrics_params& p, hipStream_t stream) {
    const BmLayout L = bm_layout(p);
    char* base = static_cast<char*>(p.workspace);
    BmWs w;
    w.stats = reinterpret_cast<BmStatSlot*>(base + L.stats);
    w.hist = reinterpret_cast<int32_t*>(base + L.hist);
    w.m1 = reinterpret_cast<double*>(base + L.m1);
    w.m2 = reinterpret_cast<double*>(base + L.m2);
    w.bpi = bm_blocks_per_image(p);
    return with_itype(p.ptype, [&](auto t) { bm_launch<decltype(t)>(p, w, stream); });
}

}  // namespace vivim

// ---- the C entry points
// every refusal that needs no workspace, before any launch; `fn` names the caller in the message
static int check_binary_metrics(const vivim_binary_metrics_params* p, const char* fn) {
    if (p == nullptr) return fail(VIVIM_ERR_INVALID, "%s: params is NULL", fn);
    if (int rc = check_struct_bytes(fn, "vivim_binary_metrics_params", p->struct_bytes, sizeof(*p))) return rc;
    if (!dtype_ok(p->ptype)) return fail(VIVIM_ERR_INVALID, "%s: ptype = %d: pred is fp32 / fp16 / bf16 (0 / 1 / 2)", fn, p->ptype);
    if (!dtype_ok(p->gtype) && p->gtype != 3)
        return fail(VIVIM_ERR_INVALID, "%s: gtype = %d: gt is fp32 / fp16 / bf16 (0 / 1 / 2) or uint8 / bool (3)", fn, p->gtype);
    if (p->batch <= 0 || p->height <= 0 || p->width <= 0)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, height = %d, width = %d: every size must be positive", fn, p->batch, p->height, p->width);
    const int64_t pixels = (int64_t)p->height * p->width;
    if (pixels < 2) return fail(VIVIM_ERR_INVALID, "%s: height * width = %lld: the metrics need at least 2 pixels", fn, (long long)pixels);
    // the kernels index inside an image and build their grid with 32-bit integers (a thread counts up to 8 pixels past the end)
    if (pixels > INT32_MAX - 4096 || (int64_t)p->batch * vivim::kBmMaxBlocks > INT32_MAX)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, height * width = %lld: the index range overflows int32", fn, p->batch, (long long)pixels);
    if (p->pred_batch_stride < pixels || p->gt_batch_stride < pixels)
        return fail(VIVIM_ERR_INVALID, "%s: pred_batch_stride = %lld, gt_batch_stride = %lld: an image has %lld elements", fn,
                    (long long)p->pred_batch_stride, (long long)p->gt_batch_stride, (long long)pixels);
    return VIVIM_OK;
}

extern "C" {

size_t vivim_binary_metrics_workspace_bytes(const vivim_binary_metrics_params* p) {
    if (check_binary_metrics(p, "binary_metrics_workspace_bytes") != VIVIM_OK) return 0;
    return vivim::binary_metrics_workspace_bytes(*p);
}

int vivim_binary_metrics(const vivim_binary_metrics_params* p, void* stream) {
    const char* fn = "binary_metrics";
    if (int rc = check_binary_metrics(p, fn)) return rc;
    if (p->pred == nullptr || !aligned(p->pred, elem_bytes(p->ptype)))
        return fail(VIVIM_ERR_INVALID, "%s: pred at %p: need a %d-byte aligned pointer", fn, p->pred, elem_bytes(p->ptype));
    const int gbytes = p->gtype == 3 ? 1 : elem_bytes(p->gtype);
    if (p->gt == nullptr || !aligned(p->gt, gbytes))
        return fail(VIVIM_ERR_INVALID, "%s: gt at %p: need a %d-byte aligned pointer", fn, p->gt, gbytes);
    if (p->thresholds == nullptr || !aligned(p->thresholds, 4))
        return fail(VIVIM_ERR_INVALID, "%s: thresholds at %p: need 256 fp32 thresholds at a 4-byte aligned pointer", fn, p->thresholds);
    if (p->values == nullptr || !aligned(p->values, 8))
        return fail(VIVIM_ERR_INVALID, "%s: values at %p: need an 8-byte aligned pointer to (batch, 9) fp64", fn, p->values);
    if (p->hist != nullptr && !aligned(p->hist, 4))
        return fail(VIVIM_ERR_INVALID, "%s: hist at %p: need NULL or a 4-byte aligned pointer", fn, p->hist);
    if (p->state != nullptr && !aligned(p->state, 8))
        return fail(VIVIM_ERR_INVALID, "%s: state at %p: need NULL or an 8-byte aligned pointer to 10 fp64", fn, p->state);
    const size_t need = vivim::binary_metrics_workspace_bytes(*p);
    if (int rc = check_workspace(fn, "vivim_binary_metrics_workspace_bytes", p->workspace, p->workspace_bytes, 8, need)) return rc;
    return after_dispatch(vivim::binary_metrics_dispatch(*p, as_stream(stream)), fn, "%s not implemented for type %d", fn, p->ptype);
}

}  // extern "C"
