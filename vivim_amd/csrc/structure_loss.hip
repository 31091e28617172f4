// structure_loss.hip -- the structure loss, boundary-weighted BCE + weighted IoU with the weight map 1 + 5 * |avgpool31(mask) - mask|,
// forward and backward (include/vivim_hip_ext.h: vivim_structure_loss_params; the eager composition is
// vivim_amd/structure_loss.py: multiclass_structure_loss / structure_loss).
//
// Three launches instead of ~25 ATen ops per class each way, no (N, C, H, W) tensor kept for autograd, and no cancellation:
//   * the window count k is an integer (at most 961): the one-hot planes live in LDS as BIT rows, a 31-tap row sum is the
//     popcount of 31 bits, the 31-tap column sum adds those bytes four (or eight) columns at a time; a = k / 961 is one division
//     (of 961 - k where the pixel is of the class, so |a - m| is not formed by subtraction either);
//   * 1 - sigmoid(x) is sigmoid(-x), and S_d = sum w * (m ? 1 : s) is accumulated as such instead of union - inter.
// A workgroup owns one kTileW x (4 * E) tile of one image (E pixels = 16 bytes of logits per thread).  It reads the labels of
// the tile and its 15-pixel halo once, turns them into the bit rows of every channel with wave ballots (a pixel outside the image
// or of no class sets no bit: avg_pool2d's zero padding with count_include_pad), and then loops over the channels: row sums of
// the tile's rows and halo rows into LDS, one barrier, column sums + the per-pixel terms.  sl_partial: four partial sums per
// channel and thread, wave_sum, one LDS step across the waves, and the workgroup STORES its 4 * C floats into slot (image, tile)
// of the workspace -- no atomics, the order of every sum depends on the shape alone.  sl_finalize adds the slots in slot order
// in fp64.  The backward kernel recomputes k, w and the sigmoid with the same tiling and writes dlogits in the logits' type.
#include "capi.cuh"
#include "seg_load.cuh"      // sl_load, sl_labels, sl_aligned16

namespace vivim {

constexpr int kStThreads = 256;                  // 4 waves per workgroup
constexpr int kStTileW = 64;                     // tile columns: one ballot
constexpr int kStHalo = 15;                      // the 31 x 31 window
constexpr int kStMaxRows = 32 + 2 * kStHalo;     // tile rows (4 * E <= 32) + halo
constexpr int kStMaxC = 8;
constexpr int kStWin = 31 * 31;

static int st_tile_rows(int itype) { return itype == VIVIM_F32 ? 16 : 32; }      // 4 * E
static int64_t st_tiles_x(const vivim_structure_loss_params& p) { return ((int64_t)p.width + kStTileW - 1) / kStTileW; }
static int64_t st_tiles_y(const vivim_structure_loss_params& p) {
    const int th = st_tile_rows(p.itype);
    return ((int64_t)p.height + th - 1) / th;
}
static int64_t structure_loss_tiles(const vivim_structure_loss_params& p) { return st_tiles_x(p) * st_tiles_y(p); }

static size_t structure_loss_workspace_bytes(const vivim_structure_loss_params& p) {
    return sizeof(float) * 4 * (size_t)p.batch * (size_t)structure_loss_tiles(p) * (size_t)p.classes;
}

enum { kStVecLogits = 1, kStVecDlogits = 2 };

struct StShared {
    uint32_t bits[kStMaxC][kStMaxRows][4];       // bit x of row r: the pixel at tile column x - 15 of tile row r - 15 is of class c
    uint32_t rsum[2][kStMaxRows][kStTileW / 4];  // 31-tap row sums, one byte per tile column; two buffers: one barrier per channel
    float red[kStThreads / kWave][4];
};

// labels of the tile and its halo -> bit rows.  A wave takes whole rows: lane l the halo column l, then (l < 30) column 64 + l.
__device__ __forceinline__ void st_load_bits(const vivim_structure_loss_params& p, StShared& sh, int n, int ty0, int tx0, int rows) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t tb = (int64_t)n * p.target_batch_stride;
    for (int r = wave; r < rows; r += kStThreads / kWave) {
        const int y = ty0 - kStHalo + r;
        int v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int x = tx0 - kStHalo + h * kWave + lane;
            int lab[1] = {-1};
            if (y >= 0 && y < p.height && x >= 0 && x < p.width && (h == 0 || lane < 2 * kStHalo))
                sl_labels<1>(p.target, p.ttype, tb + (int64_t)y * p.width + x, 1, false, lab);
            v[h] = lab[0] >= 0 ? lab[0] - p.first_class : -1;         // the channel of the pixel, or no channel
        }
        for (int c = 0; c < p.classes; ++c) {
            const uint64_t b0 = __builtin_amdgcn_ballot_w64(v[0] == c), b1 = __builtin_amdgcn_ballot_w64(v[1] == c);
            if (lane < 4)
                sh.bits[c][r][lane] = lane == 0 ? (uint32_t)b0 : lane == 1 ? (uint32_t)(b0 >> 32) : lane == 2 ? (uint32_t)b1 : 0u;
        }
    }
}

// row sums of channel c for every row of the tile and its halo: a thread takes 4 tile columns of one row, 4 popcounts, one word
__device__ __forceinline__ void st_row_sums(StShared& sh, int c, int buf, int rows) {
    for (int i = threadIdx.x; i < rows * (kStTileW / 4); i += kStThreads) {
        const int r = i / (kStTileW / 4), x = (i - r * (kStTileW / 4)) * 4;
        const int w = x >> 5, s = x & 31;                                  // s <= 28: bits s .. s + 33 of the 64 read
        const uint64_t v = (uint64_t)sh.bits[c][r][w] | ((uint64_t)sh.bits[c][r][w + 1] << 32);
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) out |= (uint32_t)__builtin_popcount((uint32_t)(v >> (s + j)) & 0x7fffffffu) << (8 * j);
        sh.rsum[buf][r][x >> 2] = out;
    }
}

// k and m of the thread's E pixels: tile row ry, tile columns x0 .. x0 + E - 1
template <int E>
__device__ __forceinline__ void st_window(const StShared& sh, int c, int buf, int ry, int x0, int (&k)[E], bool (&m)[E]) {
    // columns in pairs of 16-bit lanes: 31 bytes of at most 31 each add up to at most 961
    uint32_t even[E / 4], odd[E / 4];
#pragma unroll
    for (int q = 0; q < E / 4; ++q) even[q] = odd[q] = 0u;
#pragma unroll
    for (int dy = 0; dy <= 2 * kStHalo; ++dy) {
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
            const uint32_t w = sh.rsum[buf][ry + dy][(x0 >> 2) + q];
            even[q] += w & 0x00ff00ffu;
            odd[q] += (w >> 8) & 0x00ff00ffu;
        }
    }
    const int pos = x0 + kStHalo, w = pos >> 5, s = pos & 31;               // the pixel's own bit: s + E - 1 <= 38
    const uint64_t v = (uint64_t)sh.bits[c][ry + kStHalo][w] | ((uint64_t)sh.bits[c][ry + kStHalo][w + 1] << 32);
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
        k[4 * q] = (int)(even[q] & 0xffffu);
        k[4 * q + 1] = (int)(odd[q] & 0xffffu);
        k[4 * q + 2] = (int)(even[q] >> 16);
        k[4 * q + 3] = (int)(odd[q] >> 16);
    }
#pragma unroll
    for (int j = 0; j < E; ++j) m[j] = ((v >> (s + j)) & 1u) != 0;
}

// the per-pixel pieces: w, s = sigmoid(x), t = sigmoid(-x), softplus(-|x|) = log1p(exp(-|x|))
__device__ __forceinline__ void st_pixel(float x, int k, bool m, float& w, float& s, float& t, float& lp) {
    w = fmaf(5.0f, (float)(m ? kStWin - k : k) / (float)kStWin, 1.0f);
    const float e = fast_exp2(-fabsf(x) * kLog2e);                         // in (0, 1]; 0 once |x| > ~104
    const float u = 1.0f + e, d = u - 1.0f;
    lp = d == 0.0f ? e : fast_log(u) * (e / d);                            // Kahan's log1p: full relative precision for small e
    const float r = 1.0f / u, er = e / u;
    s = x >= 0.0f ? r : er;
    t = x >= 0.0f ? er : r;
}

template <typename T, bool BWD>
__global__ void __launch_bounds__(kStThreads) structure_loss_kernel(const vivim_structure_loss_params p, const int tiles_x, const int tiles,
                                                                    const int flags, const float inv_nc) {
    constexpr int E = 16 / (int)sizeof(T), TH = 4 * E, TPR = kStTileW / E;      // threads per tile row
    __shared__ StShared sh;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int tyi = tile / tiles_x, ty0 = tyi * TH, tx0 = (tile - tyi * tiles_x) * kStTileW;
    constexpr int rows = TH + 2 * kStHalo;
    st_load_bits(p, sh, n, ty0, tx0, rows);
    const int ry = threadIdx.x / TPR, x0 = (threadIdx.x - ry * TPR) * E;       // the thread's pixels inside the tile
    const int y = ty0 + ry, x = tx0 + x0;
    const bool row_ok = y < p.height && x < p.width;
    const int nv = row_ok ? (p.width - x < E ? p.width - x : E) : 0;
    const int pix = row_ok ? y * p.width + x : 0;                               // < 2^31: checked on the host
    const T* __restrict__ xb = static_cast<const T*>(p.logits) + (int64_t)n * p.logits_batch_stride + pix;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    float go = 0.0f;
    if (BWD) go = *static_cast<const float*>(p.grad_out) * inv_nc;
    __syncthreads();                                                            // the bit rows are written
    for (int c = 0; c < p.classes; ++c) {
        const int buf = c & 1;
        float xv[1][E];
        sl_load<T, 1, E>(xb + (int64_t)c * p.logits_c_stride, 0, nv, (flags & kStVecLogits) != 0, xv);
        st_row_sums(sh, c, buf, rows);
        __syncthreads();     // rsum[buf] is written; its previous readers (channel c - 2) are past the barrier of channel c - 1
        int k[E];
        bool m[E];
        st_window<E>(sh, c, buf, ry, x0, k, m);
        if (!BWD) {
            float sw = 0.0f, sb = 0.0f, si = 0.0f, sd = 0.0f;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                float w, s, t, lp;
                st_pixel(xv[0][j], k[j], m[j], w, s, t, lp);
                const float bce = fmaxf(xv[0][j], 0.0f) - (m[j] ? xv[0][j] : 0.0f) + lp;
                const bool ok = j < nv;
                sw += ok ? w : 0.0f;
                sb += ok ? w * bce : 0.0f;
                si += ok && m[j] ? w * s : 0.0f;
                sd += ok ? (m[j] ? w : w * s) : 0.0f;
            }
            sw = wave_sum(sw);
            sb = wave_sum(sb);
            si = wave_sum(si);
            sd = wave_sum(sd);
            if (lane == 0) {
                sh.red[wave][0] = sw;
                sh.red[wave][1] = sb;
                sh.red[wave][2] = si;
                sh.red[wave][3] = sd;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                float s = sh.red[0][threadIdx.x];
#pragma unroll
                for (int v = 1; v < kStThreads / kWave; ++v) s += sh.red[v][threadIdx.x];
                static_cast<float*>(p.workspace)[((int64_t)blockIdx.x * p.classes + c) * 4 + threadIdx.x] = s;   // slot (image, tile)
            }
            // red is rewritten only after the next channel's barrier above, which these four readers reach first
        } else {
            const float* __restrict__ cf = static_cast<const float*>(p.coef) + ((int64_t)n * p.classes + c) * 3;
            const float c0 = cf[0], c1 = cf[1], c2 = cf[2];
            float g[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                float w, s, t, lp;
                st_pixel(xv[0][j], k[j], m[j], w, s, t, lp);
                // d bce = s - m (-t where the pixel is of the class), d IoU term = -s * t * (m ? 1 / D : -(S_i + eps) / D^2)
                const float a = (m[j] ? -t : s) * c0, b = s * t * (m[j] ? c1 : -c2);
                g[j] = go * (w * (a - b));                                      // f32 all the way: rounded once, below
            }
            T* __restrict__ db = static_cast<T*>(p.dlogits) + (int64_t)n * p.dlogits_batch_stride + (int64_t)c * p.dlogits_c_stride + pix;
            if ((flags & kStVecDlogits) != 0 && nv >= E) {
                store_vec<T, E>(db, true, g);
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j)
                    if (j < nv) db[j] = from_f32<T>(g[j]);
            }
        }
    }
}

// one workgroup: thread t owns the (image, channel) pairs t, t + 256, ... and adds their slots in slot order; then a fixed LDS tree
__global__ void __launch_bounds__(kStThreads) structure_loss_finalize_kernel(const vivim_structure_loss_params p, const int tiles) {
    __shared__ double red[kStThreads];
    const int C = p.classes, tid = threadIdx.x;
    const float* __restrict__ ws = static_cast<const float*>(p.workspace);
    float* __restrict__ coef = static_cast<float*>(p.coef);
    const double eps = (double)p.eps;
    double total = 0.0;
    for (int64_t i = tid; i < (int64_t)p.batch * C; i += kStThreads) {
        const int64_t n = i / C;
        const int c = (int)(i - n * C);
        double sw = 0.0, sb = 0.0, si = 0.0, sd = 0.0;
        for (int t = 0; t < tiles; ++t) {
            const float* __restrict__ s = ws + ((n * tiles + t) * C + c) * 4;
            sw += (double)s[0];
            sb += (double)s[1];
            si += (double)s[2];
            sd += (double)s[3];
        }
        const double I = si + eps, D = sd + eps;
        total += sb / sw + 1.0 - I / D;
        if (coef) {
            coef[3 * i] = (float)(1.0 / sw);
            coef[3 * i + 1] = (float)(1.0 / D);
            coef[3 * i + 2] = (float)(I / (D * D));
        }
    }
    red[tid] = total;
    __syncthreads();
    for (int off = kStThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) *static_cast<float*>(p.loss) = (float)(red[0] / ((double)p.batch * C));
}

template <typename T>
static void st_launch(const vivim_structure_loss_params& p, bool bwd, hipStream_t stream) {
    constexpr int E = 16 / (int)sizeof(T);
    const int tiles_x = (int)st_tiles_x(p), tiles = (int)structure_loss_tiles(p);
    const dim3 grid((unsigned)((int64_t)p.batch * tiles)), block(kStThreads);
    const float inv_nc = (float)(1.0 / ((double)p.batch * p.classes));
    // a thread's 16 bytes start at pixel y * width + x0 with x0 a multiple of E: whole vectors when the rows are
    const bool rows16 = p.width % E == 0;
    int flags = 0;
    if (rows16 && sl_aligned16(p.logits, sizeof(T), {p.logits_batch_stride, p.logits_c_stride})) flags |= kStVecLogits;
    if (!bwd) {
        hipLaunchKernelGGL((structure_loss_kernel<T, false>), grid, block, 0, stream, p, tiles_x, tiles, flags, inv_nc);
        hipLaunchKernelGGL(structure_loss_finalize_kernel, dim3(1), block, 0, stream, p, tiles);
        return;
    }
    if (rows16 && sl_aligned16(p.dlogits, sizeof(T), {p.dlogits_batch_stride, p.dlogits_c_stride})) flags |= kStVecDlogits;
    hipLaunchKernelGGL((structure_loss_kernel<T, true>), grid, block, 0, stream, p, tiles_x, tiles, flags, inv_nc);
}

static bool structure_loss_dispatch(const vivim_structure_loss_params& p, bool bwd, hipStream_t stream) {
    return with_itype(p.itype, [&](auto t) { st_launch<decltype(t)>(p, bwd, stream); });
}

}  // namespace vivim

// ---- the C entry points
using vivim::kStMaxC;

static bool structure_loss_sizes_ok(const vivim_structure_loss_params* p) {
    return p->batch > 0 && p->classes > 0 && p->height > 0 && p->width > 0;
}

// every refusal the forward and the backward of the structure loss share, before any launch
static int check_structure_loss(const vivim_structure_loss_params* p, const char* fn) {
    if (p == nullptr) return fail(VIVIM_ERR_INVALID, "%s: params is NULL", fn);
    if (int rc = check_struct_bytes(fn, "vivim_structure_loss_params", p->struct_bytes, sizeof(*p))) return rc;
    if (!dtype_ok(p->itype) || (p->ttype != 0 && p->ttype != 1))
        return fail(VIVIM_ERR_INVALID, "%s: itype = %d, ttype = %d: logits are fp32 / fp16 / bf16 (0 / 1 / 2), targets int64 / uint8 (0 / 1)",
                    fn, p->itype, p->ttype);
    if (!structure_loss_sizes_ok(p))
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, classes = %d, height = %d, width = %d: every size must be positive", fn, p->batch,
                    p->classes, p->height, p->width);
    if (p->classes > kStMaxC)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: %d classes: the kernels are built for 1 to %d classes", fn, p->classes, kStMaxC);
    if (p->first_class < 0 || p->first_class > 255)
        return fail(VIVIM_ERR_INVALID, "%s: first_class = %d: labels are compared as values in [0, 256)", fn, p->first_class);
    // pixel offsets inside a plane, tile origins + halo, and the grid are 32-bit integers
    if ((int64_t)p->height * p->width > INT32_MAX - 4096 || (int64_t)p->batch * vivim::structure_loss_tiles(*p) > INT32_MAX)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, height = %d, width = %d: the index range overflows int32", fn, p->batch, p->height,
                    p->width);
    const uintptr_t ib = elem_bytes(p->itype);
    if (p->logits == nullptr || !aligned(p->logits, ib))
        return fail(VIVIM_ERR_INVALID, "%s: logits at %p: need a %d-byte aligned pointer", fn, p->logits, (int)ib);
    if (p->target == nullptr || !aligned(p->target, p->ttype == 0 ? 8 : 1))
        return fail(VIVIM_ERR_INVALID, "%s: target at %p: need a %d-byte aligned pointer", fn, p->target, p->ttype == 0 ? 8 : 1);
    return VIVIM_OK;
}

extern "C" {

size_t vivim_structure_loss_workspace_bytes(const vivim_structure_loss_params* p) {
    if (p == nullptr || p->struct_bytes != (int32_t)sizeof(vivim_structure_loss_params) || !structure_loss_sizes_ok(p) ||
        p->classes > kStMaxC || !dtype_ok(p->itype))
        return 0;
    return vivim::structure_loss_workspace_bytes(*p);
}

int vivim_structure_loss_fwd(const vivim_structure_loss_params* p, void* stream) {
    const char* fn = "structure_loss_fwd";
    if (int rc = check_structure_loss(p, fn)) return rc;
    if (p->loss == nullptr || !aligned(p->loss, 4)) return fail(VIVIM_ERR_INVALID, "%s: loss at %p: need a 4-byte aligned pointer", fn, p->loss);
    if (!aligned(p->coef, 4))                                          // NULL: not wanted
        return fail(VIVIM_ERR_INVALID, "%s: coef at %p: need a 4-byte aligned pointer (or NULL)", fn, p->coef);
    const size_t need = vivim::structure_loss_workspace_bytes(*p);
    if (int rc = check_workspace(fn, "vivim_structure_loss_workspace_bytes", p->workspace, p->workspace_bytes, 8, need)) return rc;
    return after_dispatch(vivim::structure_loss_dispatch(*p, false, as_stream(stream)), fn,
                          "%s not implemented for input type %d", fn, p->itype);
}

int vivim_structure_loss_bwd(const vivim_structure_loss_params* p, void* stream) {
    const char* fn = "structure_loss_bwd";
    if (int rc = check_structure_loss(p, fn)) return rc;
    const uintptr_t ib = elem_bytes(p->itype);
    if (p->coef == nullptr || !aligned(p->coef, 4)) return fail(VIVIM_ERR_INVALID, "%s: coef at %p: need a 4-byte aligned pointer", fn, p->coef);
    if (p->grad_out == nullptr || !aligned(p->grad_out, 4))
        return fail(VIVIM_ERR_INVALID, "%s: grad_out at %p: need a 4-byte aligned pointer", fn, p->grad_out);
    if (p->dlogits == nullptr || !aligned(p->dlogits, ib))
        return fail(VIVIM_ERR_INVALID, "%s: dlogits at %p: need a %d-byte aligned pointer", fn, p->dlogits, (int)ib);
    return after_dispatch(vivim::structure_loss_dispatch(*p, true, as_stream(stream)), fn,
                          "%s not implemented for input type %d", fn, p->itype);
}

}  // extern "C"
