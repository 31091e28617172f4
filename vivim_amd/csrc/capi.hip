// capi.hip -- the extern "C" boundary of libvivim_hip.so (see include/vivim_hip.h, frozen at ABI version 8, and one
// include/vivim_hip_ext_<feature>.h per feature added since).
// Host-side checks mirror the TORCH_CHECKs of the reference bindings that still make sense below the
// tensor layer (selective_scan.cpp:233-304, 352-438; causal_conv1d.cpp:135-163, 198-238).
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include "ops.cuh"

using vivim::Launch;
using vivim::conv_channel_last;
using vivim::elem_bytes;
using vivim::vec_elems;

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define VCHECK(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) return fail(VIVIM_ERR_INVALID, "%s: check failed: %s", __func__, #cond); \
    } while (0)

static int after_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VIVIM_ERR_LAUNCH, "%s: launch failed: %s", what, hipGetErrorString(e));
    return VIVIM_OK;
}

static bool dtype_ok(int t) { return t == VIVIM_F32 || t == VIVIM_F16 || t == VIVIM_BF16; }
static bool aligned(const void* q, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }
static bool aligned16(const void* q) { return aligned(q, 16); }
static hipStream_t as_stream(void* stream) { return static_cast<hipStream_t>(stream); }

// the refusal of a missing, short or misaligned workspace: `fn` is the entry point, `query` the call that sizes it
static int bad_workspace(const char* fn, const char* query, long long bytes, const void* at, int align, size_t need) {
    return fail(VIVIM_ERR_INVALID, "%s: workspace of %lld bytes at %p: need a %d-byte aligned one of %s() = %zu", fn, bytes, at, align,
                query, need);
}
// the same for a workspace that the params struct carries, with its own alignment; VIVIM_OK: it will do
static int check_workspace(const char* fn, const char* query, const void* ws, int64_t bytes, int align, size_t need) {
    if (ws == nullptr || !aligned(ws, align) || bytes < 0 || (size_t)bytes < need) return bad_workspace(fn, query, bytes, ws, align, need);
    return VIVIM_OK;
}
// a params struct of another library version; `name` is the struct's
static int check_struct_bytes(const char* fn, const char* name, int32_t struct_bytes, size_t size) {
    if (struct_bytes != (int32_t)size)
        return fail(VIVIM_ERR_INVALID, "%s: struct_bytes = %d, this library's %s has %zu", fn, struct_bytes, name, size);
    return VIVIM_OK;
}

// mode: the full forward, the backward (its `f` half), or the lean forward (no checkpoints; out_z alone when z is given)
enum SsmCheck { kSsmFwd, kSsmBwd, kSsmFwdLean };
static int check_ssm_fwd(const vivim_ssm_fwd_params* p, SsmCheck mode) {
    const bool is_bwd = mode == kSsmBwd;
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype));
    VCHECK(p->batch > 0 && p->dim > 0 && p->seqlen > 0 && p->dstate > 0 && p->n_groups > 0);
    VCHECK(p->dstate <= 256);                       // selective_scan.cpp:262
    VCHECK(p->dim % p->n_groups == 0);
    VCHECK(p->u && p->delta && p->A && p->B && p->C);
    if (mode == kSsmFwdLean) {
        if (p->x != nullptr)
            return fail(VIVIM_ERR_INVALID, "selective_scan_fwd_lean: x must be NULL (this entry point writes no checkpoints; "
                        "vivim_selective_scan_fwd is the call that fills x)");
        if (p->z) {
            VCHECK(p->out_z != nullptr);
            if (p->out != nullptr)
                return fail(VIVIM_ERR_INVALID, "selective_scan_fwd_lean: with z only out_z is written, out must be NULL");
        } else {
            VCHECK(p->out != nullptr);
        }
    } else {
        VCHECK(p->x != nullptr || (is_bwd && p->seqlen <= vivim::scan_ckpt_len(*p)));
        if (!is_bwd) VCHECK(p->out != nullptr);
        if (p->z) {
            if (!is_bwd) VCHECK(p->out_z != nullptr);
            else VCHECK(p->out != nullptr);             // selective_scan.cpp:423 (saved out needed for dz)
        }
    }
    if (p->is_variable_B != p->is_variable_C)
        return fail(VIVIM_ERR_UNSUPPORTED,
                    "selective_scan: mixed constant/variable B and C is not built (Vivim uses variable B and C)");
    if (!p->is_variable_B) VCHECK(p->n_groups == 1);
    return VIVIM_OK;
}

// the checks on logits, target and classes that the segmentation loss (`name` "seg_loss") and metrics ("seg_metrics") share;
// the loss's gamma is refused where it always was, between the class count and the grid bound
template <class P> static int check_seg_inputs(const P* p, const char* name) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && (p->ttype == 0 || p->ttype == 1));
    VCHECK(p->batch > 0 && p->pixels > 0);
    if (p->classes < 2 || p->classes > 8)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: %d classes: the kernels are built for 2 to 8 classes", name, p->classes);
    if constexpr (std::is_same<P, vivim_seg_loss_params>::value)
        if (p->gamma != 2.0f)
            return fail(VIVIM_ERR_UNSUPPORTED, "seg_loss: gamma = %g: the kernels are built for gamma = 2 only", (double)p->gamma);
    VCHECK((int64_t)p->batch * 64 <= INT32_MAX);                  // one workgroup index per (image, block)
    VCHECK(p->logits && aligned(p->logits, p->itype == VIVIM_F32 ? 4 : 2));
    VCHECK(p->target && aligned(p->target, p->ttype == 0 ? 8 : 1));
    return VIVIM_OK;
}

namespace vivim {
static int g_tune[2] = {-1, -1};     // host-side; accessed with relaxed atomics
static int tuning_get(int which, const char* env) {
    int v = __atomic_load_n(&g_tune[which], __ATOMIC_RELAXED);
    if (v < 0) {
        const char* e = getenv(env);
        v = e ? atoi(e) : 0;
        if (v < 0) v = 0;
        __atomic_store_n(&g_tune[which], v, __ATOMIC_RELAXED);
    }
    return v;
}
int tuning_fwd_variant() { return tuning_get(0, "VIVIM_FWD_VARIANT"); }
int tuning_bwd_variant() { return tuning_get(1, "VIVIM_BWD_VARIANT"); }
}  // namespace vivim

extern "C" {

int vivim_set_tuning(int which, int value) {
    if (which < 0 || which > 1 || value < 0) return -1;
    const int prev = which == 0 ? vivim::tuning_fwd_variant() : vivim::tuning_bwd_variant();
    __atomic_store_n(&vivim::g_tune[which], value, __ATOMIC_RELAXED);
    return prev;
}
int vivim_abi_version(void) { return VIVIM_ABI_VERSION; }
const char* vivim_last_error(void) { return g_err; }
int vivim_scan_chunk_len(int itype) { return vivim::scan_chunk_len(itype); }
int vivim_scan_ckpt_len(const vivim_ssm_fwd_params* f) { return f ? vivim::scan_ckpt_len(*f) : 0; }
size_t vivim_scan_bwd_workspace_bytes(const vivim_ssm_fwd_params* f) {
    return f ? vivim::scan_bwd_workspace_bytes(*f) : 0;
}
size_t vivim_scan_fwd_workspace_bytes(const vivim_ssm_fwd_params* f) {
    return f ? vivim::scan_fwd_workspace_bytes(*f) : 0;
}
size_t vivim_sizeof(int which) {
    static const size_t sizes[] = {
        sizeof(vivim_ssm_fwd_params), sizeof(vivim_ssm_bwd_params), sizeof(vivim_conv_fwd_params), sizeof(vivim_conv_bwd_params),
        sizeof(vivim_dwconv_params), sizeof(vivim_dwconv_wgrad_params), sizeof(vivim_dir_params), sizeof(vivim_conv_update_params),
        sizeof(vivim_state_update_params), sizeof(vivim_layernorm_params), sizeof(vivim_wgrad_nt_params),
        sizeof(vivim_add_layernorm_params), sizeof(vivim_seg_loss_params), sizeof(vivim_seg_metrics_params),
        sizeof(vivim_upsample_params)};
    return which >= 0 && which < (int)(sizeof(sizes) / sizeof(sizes[0])) ? sizes[which] : 0;
}

int vivim_selective_scan_fwd(const vivim_ssm_fwd_params* p, void* stream) {
    if (int rc = check_ssm_fwd(p, kSsmFwd)) return rc;
    if (!vivim::ssm_fwd_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "selective_scan_fwd not implemented for input type %d", p->itype);
    return after_launch("selective_scan_fwd");
}

int vivim_selective_scan_fwd_lean(const vivim_ssm_fwd_params* p, void* last_state, void* stream) {
    if (int rc = check_ssm_fwd(p, kSsmFwdLean)) return rc;
    if (!vivim::ssm_fwd_lean_dispatch(*p, last_state, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "selective_scan_fwd_lean not implemented for input type %d", p->itype);
    return after_launch("selective_scan_fwd_lean");
}

static int check_ssm_bwd(const vivim_ssm_bwd_params* p) {
    VCHECK(p != nullptr);
    if (int rc = check_ssm_fwd(&p->f, kSsmBwd)) return rc;
    VCHECK(p->dout && p->du && p->ddelta && p->dA && p->dB && p->dC);
    VCHECK((p->f.D == nullptr) == (p->dD == nullptr));
    VCHECK((p->f.delta_bias == nullptr) == (p->ddelta_bias == nullptr));
    VCHECK((p->f.z == nullptr) == (p->dz == nullptr));
    return VIVIM_OK;
}

int vivim_selective_scan_bwd(const vivim_ssm_bwd_params* p, void* stream) {
    if (int rc = check_ssm_bwd(p)) return rc;
    if (!vivim::ssm_bwd_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "selective_scan_bwd not implemented for input type %d", p->f.itype);
    return after_launch("selective_scan_bwd");
}

size_t vivim_scan_bwd_det_workspace_bytes(const vivim_ssm_fwd_params* f) {
    return f && f->batch > 0 && f->dim > 0 && f->seqlen > 0 && f->dstate > 0 && f->n_groups > 0
               ? vivim::scan_bwd_det_workspace_bytes(*f) : 0;
}

size_t vivim_scan_bwd_det_call_workspace_bytes(const vivim_ssm_bwd_params* p) {
    return check_ssm_bwd(p) == VIVIM_OK ? vivim::scan_bwd_det_call_workspace_bytes(*p) : 0;
}

int vivim_selective_scan_bwd_det(const vivim_ssm_bwd_params* p, void* det_ws, size_t det_ws_bytes, void* stream) {
    if (int rc = check_ssm_bwd(p)) return rc;
    switch (vivim::ssm_bwd_det_dispatch(*p, det_ws, det_ws_bytes, as_stream(stream))) {
        case Launch::ok: break;
        case Launch::bad_workspace:
            return bad_workspace("selective_scan_bwd_det", "vivim_scan_bwd_det_call_workspace_bytes", det_ws_bytes, det_ws, 16,
                                 vivim::scan_bwd_det_call_workspace_bytes(*p));
        case Launch::unsupported: return fail(VIVIM_ERR_UNSUPPORTED, "selective_scan_bwd_det not implemented for input type %d", p->f.itype);
    }
    return after_launch("selective_scan_bwd_det");
}

static int check_conv(const vivim_conv_fwd_params* p) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && dtype_ok(p->wtype));
    VCHECK(p->batch > 0 && p->dim > 0 && p->seqlen > 0);
    VCHECK(p->batch <= 65535 && p->dim <= 65535);
    if (!(p->width >= 2 && p->width <= 4))          // causal_conv1d.cpp:157
        return fail(VIVIM_ERR_INVALID, "causal_conv1d only supports width between 2 and 4");
    VCHECK(p->x && p->weight);
    if (p->x_l_stride != 1 && p->x_c_stride != 1)   // causal_conv1d.cpp:151-152
        return fail(VIVIM_ERR_INVALID, "causal_conv1d: x must have unit stride along seqlen or along channels");
    return VIVIM_OK;
}

int vivim_causal_conv1d_fwd(const vivim_conv_fwd_params* p, void* stream) {
    if (int rc = check_conv(p)) return rc;
    VCHECK(p->out != nullptr);
    const bool cl = conv_channel_last(*p);
    if (cl) { VCHECK(p->out_c_stride == 1); } else { VCHECK(p->out_l_stride == 1); }
    if (!vivim::conv_fwd_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "causal_conv1d_fwd not implemented for input type %d / weight type %d",
                    p->itype, p->wtype);
    return after_launch("causal_conv1d_fwd");
}

static int check_conv_bwd(const vivim_conv_bwd_params* p) {
    VCHECK(p != nullptr);
    if (int rc = check_conv(&p->f)) return rc;
    VCHECK(p->dout && p->dx && p->dweight);
    const bool cl = conv_channel_last(p->f);
    if (cl) { VCHECK(p->dout_c_stride == 1 && p->dx_c_stride == 1); }      // causal_conv1d.cpp:221, 237
    else    { VCHECK(p->dout_l_stride == 1 && p->dx_l_stride == 1); }      // causal_conv1d.cpp:220, 236
    VCHECK((p->f.bias == nullptr) == (p->dbias == nullptr));
    return VIVIM_OK;
}

size_t vivim_causal_conv1d_bwd_det_workspace_bytes(const vivim_conv_fwd_params* f) {
    return check_conv(f) == VIVIM_OK ? vivim::conv_bwd_det_workspace_bytes(*f) : 0;
}

int vivim_causal_conv1d_bwd_det(const vivim_conv_bwd_params* p, void* det_ws, size_t det_ws_bytes, void* stream) {
    if (int rc = check_conv_bwd(p)) return rc;
    switch (vivim::conv_bwd_det_dispatch(*p, det_ws, det_ws_bytes, as_stream(stream))) {
        case Launch::ok: break;
        case Launch::bad_workspace:
            return bad_workspace("causal_conv1d_bwd_det", "vivim_causal_conv1d_bwd_det_workspace_bytes", det_ws_bytes, det_ws, 16,
                                 vivim::conv_bwd_det_workspace_bytes(p->f));
        case Launch::unsupported:
            return fail(VIVIM_ERR_UNSUPPORTED, "causal_conv1d_bwd_det not implemented for input type %d / weight type %d",
                        p->f.itype, p->f.wtype);
    }
    return after_launch("causal_conv1d_bwd_det");
}

int vivim_causal_conv1d_bwd(const vivim_conv_bwd_params* p, void* stream) {
    if (int rc = check_conv_bwd(p)) return rc;
    if (!vivim::conv_bwd_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "causal_conv1d_bwd not implemented for input type %d / weight type %d",
                    p->f.itype, p->f.wtype);
    return after_launch("causal_conv1d_bwd");
}

static int check_dw_dims(int batch, int depth, int height, int width, int channels, int kd, int itype) {
    VCHECK(dtype_ok(itype));
    VCHECK(batch > 0 && depth > 0 && height > 0 && width > 0 && channels > 0);
    VCHECK(kd == 1 || kd == 3);
    VCHECK(batch <= 65535);
    return VIVIM_OK;
}

int vivim_dwconv_fwd(const vivim_dwconv_params* p, void* stream) {
    VCHECK(p != nullptr);
    if (int rc = check_dw_dims(p->batch, p->depth, p->height, p->width, p->channels, p->kd, p->itype)) return rc;
    VCHECK(p->x && p->wt && p->y);
    const int64_t cv = vec_elems(p->itype);
    VCHECK(p->channels % cv == 0 && p->x_token_stride % cv == 0 && p->x_batch_stride % cv == 0 &&
           p->y_token_stride % cv == 0 && p->y_batch_stride % cv == 0);
    VCHECK(aligned16(p->x) && aligned16(p->y));
    VCHECK(p->act >= 0 && p->act <= 2 && (p->act == 0 || p->flip == 0));
    if (p->act == 2)
        VCHECK(p->aux && aligned16(p->aux) && p->aux_token_stride % cv == 0 &&
               p->aux_batch_stride % cv == 0);
    if (!vivim::dwconv_fwd_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "dwconv_fwd not implemented for input type %d", p->itype);
    return after_launch("dwconv_fwd");
}

static int check_dw_wgrad(const vivim_dwconv_wgrad_params* p) {
    VCHECK(p != nullptr);
    if (int rc = check_dw_dims(p->batch, p->depth, p->height, p->width, p->channels, p->kd, p->itype)) return rc;
    VCHECK(p->x && p->dy && p->dwt);
    VCHECK(p->channels % 2 == 0 && p->x_token_stride % 2 == 0 && p->x_batch_stride % 2 == 0 &&
           p->dy_token_stride % 2 == 0 && p->dy_batch_stride % 2 == 0);
    VCHECK(aligned(p->x, 8) && aligned(p->dy, 8));
    return VIVIM_OK;
}

size_t vivim_dwconv_wgrad_det_workspace_bytes(const vivim_dwconv_wgrad_params* p) {
    if (!p || p->batch <= 0 || p->depth <= 0 || p->height <= 0 || p->width <= 0 || p->channels <= 0 || (p->kd != 1 && p->kd != 3))
        return 0;
    return vivim::dwconv_wgrad_det_workspace_bytes(*p);
}

int vivim_dwconv_wgrad_det(const vivim_dwconv_wgrad_params* p, void* det_ws, size_t det_ws_bytes, void* stream) {
    if (int rc = check_dw_wgrad(p)) return rc;
    switch (vivim::dwconv_wgrad_det_dispatch(*p, det_ws, det_ws_bytes, as_stream(stream))) {
        case Launch::ok: break;
        case Launch::bad_workspace:
            return bad_workspace("dwconv_wgrad_det", "vivim_dwconv_wgrad_det_workspace_bytes", det_ws_bytes, det_ws, 16,
                                 vivim::dwconv_wgrad_det_workspace_bytes(*p));
        case Launch::unsupported: return fail(VIVIM_ERR_UNSUPPORTED, "dwconv_wgrad_det not implemented for input type %d", p->itype);
    }
    return after_launch("dwconv_wgrad_det");
}

int vivim_dwconv_wgrad(const vivim_dwconv_wgrad_params* p, void* stream) {
    if (int rc = check_dw_wgrad(p)) return rc;
    if (!vivim::dwconv_wgrad_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "dwconv_wgrad not implemented for input type %d", p->itype);
    return after_launch("dwconv_wgrad");
}

static int check_dir(const vivim_dir_params* p) {
    VCHECK(p != nullptr);
    VCHECK(p->itype == VIVIM_F32 || p->itype == VIVIM_F16 || p->itype == VIVIM_BF16);
    VCHECK(p->batch > 0 && p->channels > 0 && p->seqlen > 0 && p->nframes > 0 && p->csplit > 0);
    VCHECK(p->batch <= 65535 && p->channels <= 65535);
    VCHECK(p->seqlen % p->nframes == 0 && p->channels % p->csplit == 0);
    VCHECK(p->src && p->dst);
    const int64_t e = vec_elems(p->itype);                      // 16-byte vectors on both sides
    VCHECK(p->seqlen % e == 0);
    VCHECK(aligned16(p->src) && aligned16(p->dst));
    VCHECK(p->flat_batch_stride % e == 0 && p->flat_c_stride % e == 0 && p->stk_batch_stride % e == 0 &&
           p->stk_half_stride % e == 0 && p->stk_dir_stride % e == 0 && p->stk_c_stride % e == 0);
    return VIVIM_OK;
}

int vivim_dir_scatter(const vivim_dir_params* p, void* stream) {
    if (int rc = check_dir(p)) return rc;
    if (!vivim::dir_dispatch<false>(*p, as_stream(stream))) return fail(VIVIM_ERR_UNSUPPORTED, "dir_scatter: bad itype");
    return after_launch("dir_scatter");
}

int vivim_dir_gather(const vivim_dir_params* p, void* stream) {
    if (int rc = check_dir(p)) return rc;
    if (!vivim::dir_dispatch<true>(*p, as_stream(stream))) return fail(VIVIM_ERR_UNSUPPORTED, "dir_gather: bad itype");
    return after_launch("dir_gather");
}

int vivim_causal_conv1d_update(const vivim_conv_update_params* p, void* stream) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && dtype_ok(p->wtype));
    VCHECK(p->batch > 0 && p->dim > 0 && p->batch <= 65535);
    if (p->width < 2 || p->width > 4)
        return fail(VIVIM_ERR_UNSUPPORTED, "causal_conv1d only supports width between 2 and 4");   // causal_conv1d.cpp:295
    VCHECK(p->x && p->conv_state && p->weight && p->out);
    vivim::conv_update_launch(*p, as_stream(stream));
    return after_launch("causal_conv1d_update");
}

int vivim_selective_state_update(const vivim_state_update_params* p, void* stream) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && (p->stype == VIVIM_F32 || p->stype == p->itype));
    VCHECK(p->batch > 0 && p->dim > 0 && p->dstate > 0 && p->batch <= 65535);
    VCHECK(p->state && p->x && p->dt && p->A && p->B && p->C && p->out);
    vivim::state_update_launch(*p, as_stream(stream));
    return after_launch("selective_state_update");
}

static int check_layernorm(const vivim_layernorm_params* p) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && (p->otype == VIVIM_F32 || p->otype == p->itype));
    VCHECK(p->batch > 0 && p->seqlen > 0 && p->channels > 0 && p->batch <= 65535);
    if (p->channels > 512)
        return fail(VIVIM_ERR_UNSUPPORTED, "layernorm_cm: more than 512 channels do not fit the backward's two LDS tiles");
    const int64_t e = vec_elems(p->itype);                       // 16-byte vectors along the tokens of x / dx
    VCHECK(p->seqlen % e == 0 && p->x_batch_stride % e == 0 && p->x_c_stride % e == 0);
    VCHECK(p->x && aligned16(p->x) && p->mean && p->rstd);
    return VIVIM_OK;
}

int vivim_layernorm_cm_fwd(const vivim_layernorm_params* p, void* stream) {
    if (int rc = check_layernorm(p)) return rc;
    VCHECK(p->y != nullptr);
    if (!vivim::layernorm_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "layernorm_cm_fwd not implemented for input type %d / output type %d", p->itype, p->otype);
    return after_launch("layernorm_cm_fwd");
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
    if (!vivim::layernorm_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "layernorm_cm_bwd not implemented for input type %d / output type %d", p->itype, p->otype);
    return after_launch("layernorm_cm_bwd");
}

int vivim_wgrad_nt(const vivim_wgrad_nt_params* p, void* stream) {
    VCHECK(p != nullptr);
    VCHECK(p->groups > 0 && p->groups <= 65535 && p->m > 0 && p->n > 0 && p->k > 0);
    VCHECK(p->a && p->b && p->out);
    if (p->itype != VIVIM_F16 && p->itype != VIVIM_BF16)
        return fail(VIVIM_ERR_UNSUPPORTED, "wgrad_nt takes f16 or bf16 operands (type %d given): f32 products stay on the library GEMM", p->itype);
    VCHECK(p->k % 8 == 0 && p->a_row_stride % 8 == 0 && p->b_row_stride % 8 == 0 && p->a_group_stride % 8 == 0 &&
           p->b_group_stride % 8 == 0);
    VCHECK(aligned16(p->a) && aligned16(p->b));
    VCHECK((int64_t)((p->m + 63) / 64) * ((p->n + 15) / 16) <= 65535);
    if (!vivim::wgrad_nt_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "wgrad_nt not implemented for type %d", p->itype);
    return after_launch("wgrad_nt");
}

// what the forward and the backward of the residual-add LayerNorm share; `e` <- elements per 16-byte vector of x / x_new / dres / dx
static int check_add_layernorm(const vivim_add_layernorm_params* p, int64_t* e) {
    VCHECK(p != nullptr);
    VCHECK(dtype_ok(p->itype) && dtype_ok(p->btype) && (p->weight == nullptr || dtype_ok(p->otype)));
    VCHECK(p->batch > 0 && p->seqlen > 0 && p->channels > 0 && p->batch <= 65535);
    if (p->channels > 512)
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm: more than 512 channels do not fit the backward's two LDS tiles");
    if (p->btype != p->itype && p->itype != VIVIM_F32)
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm: branch type %d with x type %d is not built (the branch has x's type, or x is f32)",
                    p->btype, p->itype);
    if (p->weight && p->otype != VIVIM_F32 && p->otype != p->itype)
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm: output type %d with x type %d is not built (f32 or x's type)", p->otype, p->itype);
    *e = vec_elems(p->itype);
    VCHECK(p->seqlen % *e == 0);
    return VIVIM_OK;
}

int vivim_add_layernorm_cm_fwd(const vivim_add_layernorm_params* p, void* stream) {
    int64_t e = 0;
    if (int rc = check_add_layernorm(p, &e)) return rc;
    VCHECK(p->x && p->branch && p->x_new && aligned16(p->x) && aligned16(p->x_new));
    VCHECK(p->x_batch_stride % e == 0 && p->x_c_stride % e == 0 && p->x_new_batch_stride % e == 0 && p->x_new_c_stride % e == 0);
    if (p->weight) VCHECK(p->y && p->mean && p->rstd);
    if (!vivim::add_layernorm_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm_fwd not implemented for x type %d / branch type %d / output type %d", p->itype,
                    p->btype, p->otype);
    return after_launch("add_layernorm_cm_fwd");
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
    if (!vivim::add_layernorm_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "add_layernorm_cm_bwd not implemented for x type %d / branch type %d / output type %d", p->itype,
                    p->btype, p->otype);
    return after_launch("add_layernorm_cm_bwd");
}

// what the forward and the backward of the segmentation loss share
static int check_seg_loss(const vivim_seg_loss_params* p) {
    if (int rc = check_seg_inputs(p, "seg_loss")) return rc;
    VCHECK(p->alpha && aligned(p->alpha, 4));
    return VIVIM_OK;
}

size_t vivim_seg_loss_workspace_bytes(const vivim_seg_loss_params* p) {
    return p && p->batch > 0 && p->pixels > 0 && p->classes > 0 && dtype_ok(p->itype) ? vivim::seg_loss_workspace_bytes(*p) : 0;
}

int vivim_seg_loss_fwd(const vivim_seg_loss_params* p, void* stream) {
    if (int rc = check_seg_loss(p)) return rc;
    VCHECK(p->loss && aligned(p->loss, 4));
    VCHECK(aligned(p->coef, 4));                                    // NULL: not wanted
    const size_t need = vivim::seg_loss_workspace_bytes(*p);
    if (int rc = check_workspace("seg_loss_fwd", "vivim_seg_loss_workspace_bytes", p->workspace, p->workspace_bytes, 4, need)) return rc;
    if (!vivim::seg_loss_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "seg_loss_fwd not implemented for input type %d / %d classes", p->itype, p->classes);
    return after_launch("seg_loss_fwd");
}

int vivim_seg_loss_bwd(const vivim_seg_loss_params* p, void* stream) {
    if (int rc = check_seg_loss(p)) return rc;
    const uintptr_t ib = elem_bytes(p->itype);
    VCHECK(p->coef && aligned(p->coef, 4));
    VCHECK(p->grad_out && aligned(p->grad_out, 4));
    VCHECK(p->dlogits && aligned(p->dlogits, ib));
    if (!vivim::seg_loss_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "seg_loss_bwd not implemented for input type %d / %d classes", p->itype, p->classes);
    return after_launch("seg_loss_bwd");
}

size_t vivim_seg_metrics_workspace_bytes(const vivim_seg_metrics_params* p) {
    return p && p->batch > 0 && p->pixels > 0 && p->classes > 0 && dtype_ok(p->itype) ? vivim::seg_metrics_workspace_bytes(*p) : 0;
}

int vivim_seg_metrics(const vivim_seg_metrics_params* p, void* stream) {
    if (int rc = check_seg_inputs(p, "seg_metrics")) return rc;
    VCHECK(p->counts && aligned(p->counts, 4));
    VCHECK(aligned(p->state, 8));         // NULL: not wanted (pred: any address)
    const size_t need = vivim::seg_metrics_workspace_bytes(*p);
    if (int rc = check_workspace("seg_metrics", "vivim_seg_metrics_workspace_bytes", p->workspace, p->workspace_bytes, 4, need)) return rc;
    if (!vivim::seg_metrics_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "seg_metrics not implemented for input type %d / %d classes", p->itype, p->classes);
    return after_launch("seg_metrics");
}

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
    // the kernels index inside an image, and build their windows and their grid, with 32-bit integers
    VCHECK((int64_t)p->channels * p->in_h * p->in_w <= INT32_MAX && (int64_t)p->channels * p->out_h * p->out_w <= INT32_MAX);
    VCHECK((2 * (int64_t)p->in_h + 3) * p->out_h <= INT32_MAX && (2 * (int64_t)p->in_w + 3) * p->out_w <= INT32_MAX);
    VCHECK((int64_t)p->batch * p->channels <= INT32_MAX && (int64_t)p->batch * p->out_h <= INT32_MAX);
    VCHECK(vivim::upsample_blocks(*p, bwd) <= INT32_MAX);
    return VIVIM_OK;
}

int vivim_upsample_bilinear2d_fwd(const vivim_upsample_params* p, void* stream) {
    if (int rc = check_upsample(p, false)) return rc;
    if (!vivim::upsample_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "upsample_bilinear2d_fwd not implemented for type %d", p->itype);
    return after_launch("upsample_bilinear2d_fwd");
}

int vivim_upsample_bilinear2d_bwd(const vivim_upsample_params* p, void* stream) {
    if (int rc = check_upsample(p, true)) return rc;
    if (!vivim::upsample_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "upsample_bilinear2d_bwd not implemented for type %d", p->itype);
    return after_launch("upsample_bilinear2d_bwd");
}

// every refusal of the fused decode head, before any launch
static int check_decode_head(const vivim_decode_head_params* p) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes("decode_head_fwd", "vivim_decode_head_params", p->struct_bytes, sizeof(*p))) return rc;
    VCHECK(dtype_ok(p->itype));
    VCHECK(p->batch > 0 && p->hidden > 0 && p->classes > 0 && p->out_h > 0 && p->out_w > 0);
    VCHECK(p->n_maps >= 1 && p->n_maps <= 4);
    VCHECK(p->classes <= 8);
    if (p->hidden > vivim::decode_head_max_hidden())
        return fail(VIVIM_ERR_INVALID, "decode_head_fwd: hidden = %d: bias and w_out are kept in LDS, which holds up to %d channels",
                    p->hidden, vivim::decode_head_max_hidden());
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

int vivim_decode_head_fwd(const vivim_decode_head_params* p, void* stream) {
    if (int rc = check_decode_head(p)) return rc;
    if (!vivim::decode_head_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "decode_head_fwd not implemented for type %d", p->itype);
    return after_launch("decode_head_fwd");
}

// every refusal the forward and the backward of the token-major LayerNorm share, before any launch
static int check_token_layernorm(const vivim_token_layernorm_params* p, const char* fn) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_token_layernorm_params", p->struct_bytes, sizeof(*p))) return rc;
    VCHECK(dtype_ok(p->itype) && dtype_ok(p->otype));
    VCHECK(p->rows > 0);
    if (p->channels < 1)
        return fail(VIVIM_ERR_INVALID, "%s: channels = %d: a row has at least one channel", fn, p->channels);
    if (p->channels > 1024)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: channels = %d: a row of more than 1024 channels does not fit the lanes' registers", fn,
                    p->channels);
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

int vivim_token_layernorm_fwd(const vivim_token_layernorm_params* p, void* stream) {
    if (int rc = check_token_layernorm(p, "token_layernorm_fwd")) return rc;
    VCHECK(p->y != nullptr && aligned(p->y, p->otype == VIVIM_F32 ? 4 : 2));
    VCHECK(aligned(p->bias, 4));                                     // NULL: zeros
    VCHECK((p->mean == nullptr) == (p->rstd == nullptr) && aligned(p->mean, 4) && aligned(p->rstd, 4));
    if (p->y_row_stride < p->channels)
        return fail(VIVIM_ERR_INVALID, "token_layernorm_fwd: y_row_stride = %lld is less than the %d channels of a row",
                    (long long)p->y_row_stride, p->channels);
    if (!vivim::token_layernorm_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "token_layernorm_fwd not implemented for input type %d / output type %d", p->itype, p->otype);
    return after_launch("token_layernorm_fwd");
}

size_t vivim_token_layernorm_bwd_workspace_bytes(const vivim_token_layernorm_params* p) {
    return p && p->rows > 0 && p->channels > 0 && p->channels <= 1024 ? vivim::token_layernorm_bwd_workspace_bytes(*p) : 0;
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
    if (!vivim::token_layernorm_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "token_layernorm_bwd not implemented for input type %d / output type %d", p->itype, p->otype);
    return after_launch("token_layernorm_bwd");
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
    if (p->channels > 1024)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: channels = %d: a row of more than 1024 channels does not fit the lanes' registers", fn,
                    p->channels);
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
    if (!vivim::token_add_norm_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for branch type %d / residual type %d", fn, p->btype, p->rtype);
    return after_launch(fn);
}

size_t vivim_token_add_norm_bwd_workspace_bytes(const vivim_token_add_norm_params* p) {
    return p && p->rows > 0 && p->channels > 0 && p->channels <= 1024 ? vivim::token_add_norm_bwd_workspace_bytes(*p) : 0;
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
    if (!vivim::token_add_norm_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for branch type %d / residual type %d", fn, p->btype, p->rtype);
    return after_launch(fn);
}

// ---- fused clip + AdamW step (optimizer.hip)
static int check_opt_common(const vivim_opt_step_params* p, const char* fn) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_opt_step_params", p->struct_bytes, sizeof(*p))) return rc;
    VCHECK(p->state != nullptr && aligned(p->state, 4));
    if (p->total_blocks < 0) return fail(VIVIM_ERR_INVALID, "%s: total_blocks = %d", fn, p->total_blocks);
    return VIVIM_OK;
}

// the tensors and map rows of one multi-tensor call
static int check_opt_tensors(const vivim_opt_step_params* p, const char* fn, size_t grad_align = 4) {
    if (p->count <= 0 || p->count > VIVIM_OPT_MAX_TENSORS)
        return fail(VIVIM_ERR_INVALID, "%s: count = %d, a call takes 1 to %d tensors", fn, p->count, VIVIM_OPT_MAX_TENSORS);
    VCHECK(p->grads != nullptr && p->numel != nullptr && p->block_map != nullptr);
    VCHECK(aligned(p->block_map, 4) && p->first_tensor >= 0);
    for (int i = 0; i < p->count; ++i) {
        if (p->numel[i] <= 0) return fail(VIVIM_ERR_INVALID, "%s: numel[%d] = %lld", fn, i, (long long)p->numel[i]);
        VCHECK(aligned(p->grads[i], grad_align));
    }
    if (p->first_block < 0 || p->n_blocks <= 0 || (int64_t)p->first_block + p->n_blocks > p->total_blocks)
        return fail(VIVIM_ERR_INVALID, "%s: map rows %d .. %d + %d of %d", fn, p->first_block, p->first_block, p->n_blocks, p->total_blocks);
    return VIVIM_OK;
}

static int check_opt_workspace(const vivim_opt_step_params* p, const char* fn) {
    const size_t need = 8 * (size_t)p->total_blocks;
    if (need && (p->workspace == nullptr || !aligned(p->workspace, 8) || p->workspace_bytes < (int64_t)need))
        return bad_workspace(fn, "vivim_opt_step_workspace_bytes", (long long)p->workspace_bytes, p->workspace, 8, need);
    return VIVIM_OK;
}

// the hyper-parameters of a step: the betas, and for the `update` itself lr, eps and weight_decay
static int check_opt_hyper(const vivim_opt_step_params* p, const char* fn, bool update) {
    if (!(p->beta1 >= 0.0 && p->beta1 < 1.0 && p->beta2 >= 0.0 && p->beta2 < 1.0))
        return fail(VIVIM_ERR_INVALID, "%s: betas = (%g, %g), each must be in [0, 1)", fn, p->beta1, p->beta2);
    if (update && !(p->lr >= 0.0 && p->eps >= 0.0 && p->weight_decay >= 0.0))
        return fail(VIVIM_ERR_INVALID, "%s: lr = %g, eps = %g, weight_decay = %g: none may be negative", fn, p->lr, p->eps, p->weight_decay);
    return VIVIM_OK;
}

size_t vivim_opt_step_workspace_bytes(const vivim_opt_step_params* p) {
    return p && p->struct_bytes == (int32_t)sizeof(vivim_opt_step_params) && p->total_blocks > 0 ? 8 * (size_t)p->total_blocks : 0;
}

int vivim_opt_grad_stats(const vivim_opt_step_params* p, void* stream) {
    const char* fn = "opt_grad_stats";
    if (int rc = check_opt_common(p, fn)) return rc;
    if (int rc = check_opt_tensors(p, fn)) return rc;
    if (int rc = check_opt_workspace(p, fn)) return rc;
    vivim::opt_grad_stats_launch(*p, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_finalise(const vivim_opt_step_params* p, void* stream) {
    const char* fn = "opt_finalise";
    if (int rc = check_opt_common(p, fn)) return rc;
    if (int rc = check_opt_hyper(p, fn, false)) return rc;
    if (p->has_max_norm && !(p->max_norm >= 0.0)) return fail(VIVIM_ERR_INVALID, "%s: max_norm = %g", fn, p->max_norm);
    if (int rc = check_opt_workspace(p, fn)) return rc;
    vivim::opt_finalise_launch(*p, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_adamw(const vivim_opt_step_params* p, void* stream) {
    const char* fn = "opt_adamw";
    if (int rc = check_opt_common(p, fn)) return rc;
    VCHECK(p->params != nullptr && p->exp_avg != nullptr && p->exp_avg_sq != nullptr);
    VCHECK(aligned(p->params, 8) && aligned(p->exp_avg, 8) && aligned(p->exp_avg_sq, 8));
    if (int rc = check_opt_tensors(p, fn)) return rc;
    if (int rc = check_opt_hyper(p, fn, true)) return rc;
    vivim::opt_adamw_launch(*p, as_stream(stream));
    return after_launch(fn);
}

// ---- the same step for 16-bit parameters with fp32 masters: vivim_opt_mw_params is vivim_opt_step_params + masters + dtype
static int check_opt_mw(const vivim_opt_mw_params* p, const char* fn, vivim_opt_step_params& q) {
    VCHECK(p != nullptr);
    if (int rc = check_struct_bytes(fn, "vivim_opt_mw_params", p->struct_bytes, sizeof(*p))) return rc;
    static_assert(offsetof(vivim_opt_mw_params, masters) == sizeof(vivim_opt_step_params), "the common fields come first");
    memcpy(&q, p, sizeof(q));
    q.struct_bytes = (int32_t)sizeof(q);
    if (int rc = check_opt_common(&q, fn)) return rc;
    if (p->dtype != VIVIM_F16 && p->dtype != VIVIM_BF16)
        return fail(VIVIM_ERR_INVALID, "%s: dtype = %d, master weights are for 1 (fp16) and 2 (bf16)", fn, p->dtype);
    return VIVIM_OK;
}

int vivim_opt_grad_stats_mw(const vivim_opt_mw_params* p, void* stream) {
    const char* fn = "opt_grad_stats_mw";
    vivim_opt_step_params q;
    if (int rc = check_opt_mw(p, fn, q)) return rc;
    if (int rc = check_opt_tensors(&q, fn, 2)) return rc;
    if (int rc = check_opt_workspace(&q, fn)) return rc;
    vivim::opt_grad_stats_mw_launch(q, p->dtype, as_stream(stream));
    return after_launch(fn);
}

int vivim_opt_adamw_mw(const vivim_opt_mw_params* p, void* stream) {
    const char* fn = "opt_adamw_mw";
    vivim_opt_step_params q;
    if (int rc = check_opt_mw(p, fn, q)) return rc;
    VCHECK(q.params != nullptr && q.exp_avg != nullptr && q.exp_avg_sq != nullptr && p->masters != nullptr);
    VCHECK(aligned(q.params, 8) && aligned(q.exp_avg, 8) && aligned(q.exp_avg_sq, 8) && aligned(p->masters, 8));
    if (int rc = check_opt_tensors(&q, fn, 2)) return rc;
    if (int rc = check_opt_hyper(&q, fn, true)) return rc;
    vivim::opt_adamw_mw_launch(q, p->masters, p->dtype, as_stream(stream));
    return after_launch(fn);
}

// ---- include/vivim_hip_ext.h: the structure loss, the first feature added after ABI version 8 ----

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
    if (p->classes > 8)
        return fail(VIVIM_ERR_UNSUPPORTED, "%s: %d classes: the kernels are built for 1 to 8 classes", fn, p->classes);
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

size_t vivim_structure_loss_workspace_bytes(const vivim_structure_loss_params* p) {
    if (p == nullptr || p->struct_bytes != (int32_t)sizeof(vivim_structure_loss_params) || !structure_loss_sizes_ok(p) || p->classes > 8 ||
        !dtype_ok(p->itype))
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
    if (!vivim::structure_loss_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for input type %d", fn, p->itype);
    return after_launch(fn);
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
    if (!vivim::structure_loss_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for input type %d", fn, p->itype);
    return after_launch(fn);
}

// ---- include/vivim_hip_ext_head.h: the training head's upsample + dropout + concat ----

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
    // (a row's last workgroup counts up to 255 positions past its end)
    bool fits = out_image <= INT32_MAX - 256 && (int64_t)p->batch * p->out_h <= INT32_MAX;
    for (int s = 0; s < p->n_maps; ++s)
        fits = fits && (2 * (int64_t)p->map_h[s] + 3) * p->out_h <= INT32_MAX && (2 * (int64_t)p->map_w[s] + 3) * p->out_w <= INT32_MAX;
    if (!fits || vivim::head_concat_blocks(*p, bwd) > INT32_MAX)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, out (%d, %d), out_pixel_stride = %lld: the index range overflows int32", fn, p->batch,
                    p->out_h, p->out_w, (long long)p->out_pixel_stride);
    return VIVIM_OK;
}

int vivim_head_concat_fwd(const vivim_head_concat_params* p, void* stream) {
    const char* fn = "head_concat_fwd";
    if (int rc = check_head_concat(p, fn, false)) return rc;
    if (!vivim::head_concat_dispatch(*p, false, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for type %d", fn, p->itype);
    return after_launch(fn);
}

int vivim_head_concat_bwd(const vivim_head_concat_params* p, void* stream) {
    const char* fn = "head_concat_bwd";
    if (int rc = check_head_concat(p, fn, true)) return rc;
    if (!vivim::head_concat_dispatch(*p, true, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for type %d", fn, p->itype);
    return after_launch(fn);
}

// ---- include/vivim_hip_ext_binary_metrics.h: the validation metrics of the binary recipe ----

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
    if (pixels > INT32_MAX - 4096 || (int64_t)p->batch * 32 > INT32_MAX)
        return fail(VIVIM_ERR_INVALID, "%s: batch = %d, height * width = %lld: the index range overflows int32", fn, p->batch, (long long)pixels);
    if (p->pred_batch_stride < pixels || p->gt_batch_stride < pixels)
        return fail(VIVIM_ERR_INVALID, "%s: pred_batch_stride = %lld, gt_batch_stride = %lld: an image has %lld elements", fn,
                    (long long)p->pred_batch_stride, (long long)p->gt_batch_stride, (long long)pixels);
    return VIVIM_OK;
}

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
    if (!vivim::binary_metrics_dispatch(*p, as_stream(stream)))
        return fail(VIVIM_ERR_UNSUPPORTED, "%s not implemented for type %d", fn, p->ptype);
    return after_launch(fn);
}

}  // extern "C"
