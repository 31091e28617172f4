/*
 * vivim_hip.h -- C ABI of libvivim_hip.so: the MI355X (gfx950) drop-in for the two CUDA extension
 * modules on Vivim's Temporal-Mamba hot path.
 *
 * Each entry point replaces one function the reference binds with pybind11 (all citations are
 * file:line under /root/reference):
 *
 *   vivim_selective_scan_fwd  <- selective_scan_cuda.fwd   mamba/csrc/selective_scan/selective_scan.cpp:226-336
 *                                params struct SSMParamsBase mamba/csrc/selective_scan/selective_scan.h:26-69
 *   vivim_selective_scan_bwd  <- selective_scan_cuda.bwd   mamba/csrc/selective_scan/selective_scan.cpp:338-492
 *                                params struct SSMParamsBwd  mamba/csrc/selective_scan/selective_scan.h:71-101
 *   vivim_causal_conv1d_fwd   <- causal_conv1d_cuda.causal_conv1d_fwd  causal-conv1d/csrc/causal_conv1d.cpp:130-189
 *                                params struct ConvParamsBase causal-conv1d/csrc/causal_conv1d.h:9-35
 *   vivim_causal_conv1d_bwd   <- causal_conv1d_cuda.causal_conv1d_bwd  causal-conv1d/csrc/causal_conv1d.cpp:191-268
 *                                params struct ConvParamsBwd  causal-conv1d/csrc/causal_conv1d.h:37-52
 *
 * Contract (same as the reference bindings after their ATen part):
 *   - every pointer is a DEVICE pointer on the current device; strides are in ELEMENTS; the token
 *     (seqlen) axis of every activation tensor has unit stride; batch / channel strides are free
 *     (Vivim passes halves of `xz`, strides (L, B*L, 1) -- mamba_simple.py:204-208).
 *   - the call only enqueues kernels on `stream` (a hipStream_t, NULL = default stream): it never
 *     synchronises, allocates or frees, and keeps no per-call state (re-entrant).  The one piece of process-global
 *     mutable state is the kernel-selection override of vivim_set_tuning() (tests / tuning only, default 0 = automatic):
 *     it also changes vivim_scan_ckpt_len(), so it must not be changed between a forward call and its backward call or
 *     while another thread is inside the library.
 *   - outputs are caller-allocated.  Accumulated outputs (dA, dB, dC, dD, ddelta_bias, dweight,
 *     dbias) are float32 and MUST be zero-filled by the caller before the call, exactly as the
 *     reference binding does (selective_scan.cpp:458-466, causal_conv1d.cpp:247-249).
 *   - returns 0 on success; otherwise a VIVIM_ERR_* code, and vivim_last_error() returns a
 *     thread-local message naming the failed check (the reference raises RuntimeError there).
 *
 * Differences from the reference structs, on purpose: strides are int64 (a 288 GB HBM3E part holds
 * tensors past 2^32 elements; the reference uses uint32, selective_scan.h:27); the input dtype is an
 * explicit enum instead of a C++ template dispatch; `x` (scan checkpoints) has OUR chunk length,
 * vivim_scan_ckpt_len(), instead of the reference's fixed 2048 (selective_scan.cpp:307).
 */
#ifndef VIVIM_HIP_H
#define VIVIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIVIM_ABI_VERSION 8

typedef enum { VIVIM_F32 = 0, VIVIM_F16 = 1, VIVIM_BF16 = 2 } vivim_dtype_t;

enum {
    VIVIM_OK = 0,
    VIVIM_ERR_INVALID = 1,      /* failed shape / stride / pointer check */
    VIVIM_ERR_UNSUPPORTED = 2,  /* valid in the reference but not built here (see message) */
    VIVIM_ERR_LAUNCH = 3        /* hipGetLastError() after the launch */
};

/* ---- selective scan, forward (selective_scan.h:26-69) --------------------------------------- */
typedef struct {
    int32_t batch, dim, seqlen, dstate, n_groups;
    int32_t itype;              /* vivim_dtype_t of u, delta, z, out, out_z and of variable B / C */
    int32_t is_variable_B;      /* B is (batch, n_groups, dstate, seqlen) itype; else (dim, dstate) f32 */
    int32_t is_variable_C;
    int32_t delta_softplus;
    int32_t _pad0;
    int64_t u_batch_stride, u_d_stride;
    int64_t delta_batch_stride, delta_d_stride;
    int64_t z_batch_stride, z_d_stride;
    int64_t out_batch_stride, out_d_stride;
    int64_t out_z_batch_stride, out_z_d_stride;
    int64_t A_d_stride, A_dstate_stride;
    int64_t B_batch_stride, B_group_stride, B_dstate_stride;   /* constant B: batch/group stride unused, */
    int64_t C_batch_stride, C_group_stride, C_dstate_stride;   /* B_d_stride == B_group_stride slot     */
    const void *u, *delta;      /* (batch, dim, seqlen) itype */
    const void *A;              /* (dim, dstate) f32 */
    const void *B, *C;
    const void *D;              /* (dim) f32 or NULL */
    const void *delta_bias;     /* (dim) f32 or NULL */
    const void *z;              /* (batch, dim, seqlen) itype or NULL */
    void *out;                  /* (batch, dim, seqlen) itype: y + D*u, before gating.  The reference allocates out / out_z with
                                   delta's / z's strides (selective_scan.cpp:311-313); a shape that gets the short checkpoint
                                   rows (vivim_scan_ckpt_len() == 16 * (dstate / 16)) needs every (channel, token) byte offset
                                   of out / out_z inside one batch element below 2^32 - 2^16, as it already holds for delta / z
                                   there: other strides return VIVIM_ERR_UNSUPPORTED */
    void *out_z;                /* out * silu(z); required iff z != NULL */
    void *x;                    /* (batch, dim, n_chunks, dstate) f32 contiguous: state after each chunk of
                                   vivim_scan_ckpt_len() tokens; x[:, :, -1, :] is the final state
                                   (the reference's x[:, :, -1, 1::2], selective_scan_interface.py:40) */
    void *workspace;            /* forward only: device scratch of >= vivim_scan_fwd_workspace_bytes() bytes or NULL
                                   (NULL selects a kernel that needs none); ignored inside vivim_ssm_bwd_params.f */
    int64_t workspace_bytes;
} vivim_ssm_fwd_params;

/* ---- selective scan, backward (selective_scan.h:71-101) ------------------------------------- */
typedef struct {
    vivim_ssm_fwd_params f;     /* forward tensors; f.out = SAVED forward `out` (needed iff z != NULL);
                                   f.out_z = optional recomputed out_z destination (may be NULL);
                                   f.x = forward checkpoints (required when seqlen > chunk_len) */
    int64_t dout_batch_stride, dout_d_stride;
    int64_t du_batch_stride, du_d_stride;
    int64_t ddelta_batch_stride, ddelta_d_stride;
    int64_t dz_batch_stride, dz_d_stride;
    int64_t dA_d_stride, dA_dstate_stride;
    int64_t dB_batch_stride, dB_group_stride, dB_dstate_stride;
    int64_t dC_batch_stride, dC_group_stride, dC_dstate_stride;
    const void *dout;           /* (batch, dim, seqlen) itype */
    void *du, *ddelta;          /* itype */
    void *dz;                   /* itype; required iff z != NULL (may alias a caller view of dxz) */
    void *dA;                   /* (dim, dstate) f32, pre-zeroed */
    void *dB, *dC;              /* f32, pre-zeroed: (batch, n_groups, dstate, seqlen) if variable else (dim, dstate) */
    void *dD;                   /* (dim) f32 pre-zeroed, or NULL iff D == NULL */
    void *ddelta_bias;          /* (dim) f32 pre-zeroed, or NULL iff delta_bias == NULL */
    void *workspace;            /* device scratch of >= vivim_scan_bwd_workspace_bytes() bytes, or NULL: the
                                   kernel then walks the whole sequence inside one workgroup per 16 channels
                                   (correct, but far fewer workgroups in flight).  Contents are don't-care. */
    int64_t workspace_bytes;
} vivim_ssm_bwd_params;

/* ---- causal depthwise conv1d (causal_conv1d.h:9-52) ------------------------------------------ */
typedef struct {
    int32_t batch, dim, seqlen, width;   /* width in [2, 4] (causal_conv1d.cpp:157) */
    int32_t itype;                       /* dtype of x, out, dout, dx */
    int32_t wtype;                       /* dtype of weight and bias */
    int32_t silu_activation;
    int32_t _pad0;
    int64_t x_batch_stride, x_c_stride, x_l_stride;         /* x_l_stride == 1 (channel-first), or x_c_stride == 1 and
                                                               x_l_stride > 1 (channel-last, causal_conv1d.cpp:151):
                                                               out / dout / dx must then have unit channel stride too */
    int64_t out_batch_stride, out_c_stride, out_l_stride;
    int64_t weight_c_stride, weight_width_stride;
    const void *x;              /* (batch, dim, seqlen) */
    const void *weight;         /* (dim, width) */
    const void *bias;           /* (dim) or NULL */
    void *out;                  /* forward output; unused by the backward */
} vivim_conv_fwd_params;

typedef struct {
    vivim_conv_fwd_params f;
    int64_t dout_batch_stride, dout_c_stride, dout_l_stride;
    int64_t dx_batch_stride, dx_c_stride, dx_l_stride;
    int64_t dweight_c_stride, dweight_width_stride;
    const void *dout;
    void *dx;                   /* itype, may be a strided caller view (causal_conv1d.cpp:232-238) */
    void *dweight;              /* (dim, width) f32 pre-zeroed */
    void *dbias;                /* (dim) f32 pre-zeroed, or NULL iff bias == NULL */
} vivim_conv_bwd_params;

/* ---- depthwise 3x3 / 3x3x3 convolution on token-major tensors ---------------
 * Replaces the ATen call behind modeling/vivim.py:57-68 (DWConv: nn.Conv3d(dim, dim, 3, 1, 1, groups=dim) applied
 * to x.transpose(1, 2).view(B, C, nf, H, W)); the reference has no kernel of its own there.
 * x, y: (batch, depth*height*width, channels), channels contiguous, token stride and batch stride free.
 * wt: (kd*9, channels) f32, TAP-major: wt[(kd*3 + kh)*3 + kw][c] = conv.weight[c][0][kd][kh][kw].
 * flip = 1 correlates with the reversed tap order: the input gradient of the same convolution.
 * act (ABI v7) fuses the Mlp's activation (modeling/vivim.py:99-106: act(dwconv(fc1(x))), act = nn.GELU, erf form) into
 * the convolution's epilogue: 0 y = conv; 1 y = gelu(conv); 2 y = aux * gelu'(conv) -- the gradient with respect to the
 * pre-activation, the convolution recomputed instead of stored (aux = the gradient of the activation's output, laid out
 * like y).  act != 0 requires flip == 0. */
typedef struct {
    int32_t batch, depth, height, width, channels;
    int32_t kd;                 /* 1 (2-D, 3x3) or 3 (3-D, 3x3x3) */
    int32_t itype;              /* dtype of x and y; channels % (16 / sizeof) == 0 and 16-byte aligned rows */
    int32_t flip;
    int64_t x_batch_stride, x_token_stride;
    int64_t y_batch_stride, y_token_stride;
    const void *x, *wt, *bias;  /* bias (channels) f32 or NULL */
    void *y;
    int32_t act, _pad1;
    const void *aux;            /* act == 2: (batch, tokens, channels) itype, 16-byte aligned rows; else ignored */
    int64_t aux_batch_stride, aux_token_stride;
} vivim_dwconv_params;

typedef struct {
    int32_t batch, depth, height, width, channels;
    int32_t kd;
    int32_t itype;              /* dtype of x and dy; channels % 2 == 0 */
    int32_t _pad0;
    int64_t x_batch_stride, x_token_stride;
    int64_t dy_batch_stride, dy_token_stride;
    const void *x, *dy;
    void *dwt;                  /* (kd*9, channels) f32 tap-major, pre-zeroed */
    void *dbias;                /* (channels) f32 pre-zeroed, or NULL */
} vivim_dwconv_wgrad_params;

/* The three scan directions of the v3 block (mamba_simple.py:220-262) as index maps over the token axis of a
 * frame-major clip, l = t*hw + p with t < nframes, p < hw = seqlen / nframes:
 *   direction 0: l            (forward in time)
 *   direction 1: seqlen-1-l   (xz.flip(-1), :231 / out_b.flip(-1), :264)
 *   direction 2: p*nframes+t  (chunk(nframes) + stack(-1) + flatten, :245-247; inverse at :261)
 * scatter: dst[b][c / csplit][g][c % csplit][m_g(l)] = scale * src[b][c][l]   for g = 0, 1, 2    (one read, three writes)
 * gather : dst[b][c][l] = scale * sum_g src[b][c / csplit][g][c % csplit][m_g(l)]               (three reads, one write)
 * They replace flip + stack/permute copies and the out + out_b + out_s sum, and are each other's gradient. */
typedef struct {
    int32_t batch, channels, seqlen, nframes;
    int32_t csplit;              /* channels per half: the stacked tensor is (batch, channels/csplit, 3, csplit, seqlen) */
    int32_t itype;               /* VIVIM_F32 / F16 / BF16 */
    float scale;
    int32_t _pad0;
    int64_t flat_batch_stride, flat_c_stride;                  /* the (batch, channels, seqlen) side; unit seqlen stride */
    int64_t stk_batch_stride, stk_half_stride, stk_dir_stride, stk_c_stride;   /* the stacked side; unit seqlen stride */
    const void *src;
    void *dst;
} vivim_dir_params;

/* ---- single-token steps for streaming inference ------------------------------------------
 * causal_conv1d_update (causal_conv1d.cpp:270-327, causal_conv1d_update.cu:26-66): conv_state is shifted left by one
 * along width, x is appended, out = sum_w conv_state[w] * weight[w] (+ bias) (silu). */
typedef struct {
    int32_t batch, dim, width;           /* width in [2, 4] */
    int32_t itype;                       /* x, conv_state, out */
    int32_t wtype;                       /* weight, bias */
    int32_t silu_activation;
    int64_t x_batch_stride, x_c_stride;
    int64_t state_batch_stride, state_c_stride, state_w_stride;
    int64_t weight_c_stride, weight_width_stride;
    int64_t out_batch_stride, out_c_stride;
    const void *x;              /* (batch, dim) */
    void *conv_state;           /* (batch, dim, width), updated in place */
    const void *weight;         /* (dim, width) */
    const void *bias;           /* (dim) or NULL */
    void *out;                  /* (batch, dim) */
} vivim_conv_update_params;

/* selective_state_update (mamba_ssm/ops/triton/selective_state_update.py:21-155): dt' = (softplus)(dt + dt_bias);
 * state = state * exp(dt' * A) + dt' * B * x (in place); out = sum_n state * C + D * x, gated by silu(z). */
typedef struct {
    int32_t batch, dim, dstate;
    int32_t itype;                       /* x, dt, B, C, z, out */
    int32_t stype;                       /* state: VIVIM_F32 or the same as itype */
    int32_t dt_softplus;
    int64_t state_batch_stride, state_d_stride, state_n_stride;
    int64_t x_batch_stride, x_d_stride, dt_batch_stride, dt_d_stride;
    int64_t A_d_stride, A_n_stride;
    int64_t B_batch_stride, B_n_stride, C_batch_stride, C_n_stride;
    int64_t z_batch_stride, z_d_stride, out_batch_stride, out_d_stride;
    void *state;                /* (batch, dim, dstate), updated in place */
    const void *x, *dt;         /* (batch, dim) */
    const void *A;              /* (dim, dstate) f32 */
    const void *B, *C;          /* (batch, dstate) */
    const void *D;              /* (dim) f32 or NULL */
    const void *z;              /* (batch, dim) or NULL */
    const void *dt_bias;        /* (dim) f32 or NULL */
    void *out;                  /* (batch, dim) */
} vivim_state_update_params;

/* ---- LayerNorm over the channels of a CHANNEL-major token tensor ---------------------------------------
 * Replaces the ATen calls behind modeling/vivim.py:155-156 (self.norm(x_flat) with x_flat = x.reshape(B, C, L).transpose(-1, -2):
 * a (B, L, C) view with strides (C*L, 1, L)); the reference has no kernel of its own there.
 *   forward : y[b][t][c] = (x[b][c][t] - mean[b][t]) * rstd[b][t] * weight[c] + bias[c]      mean / rstd over c, biased variance
 *   backward: dx[b][c][t] (channel-major like x), dweight[c] += sum dy * xhat, dbias[c] += sum dy   (f32, pre-zeroed by the caller;
 *             the per-tile partial sums go through `workspace`, vivim_layernorm_bwd_workspace_bytes() of it, added up by a
 *             second small kernel on the same stream: required whenever dweight or dbias is given)
 * x, dx: itype, unit token stride, 16-byte aligned rows, seqlen a whole number of 16-byte pieces; y, dy: otype = VIVIM_F32 (what
 * autocast makes of layer_norm) or itype, unit channel stride; channels <= 512. */
typedef struct {
    int32_t batch, seqlen, channels;
    int32_t itype, otype;
    float eps;
    int64_t x_batch_stride, x_c_stride;      /* x: (batch, channels, seqlen) memory, token stride 1 */
    int64_t y_batch_stride, y_token_stride;  /* y and dy: (batch, seqlen, channels), channel stride 1 */
    int64_t dx_batch_stride, dx_c_stride;    /* dx: laid out like x */
    const void *x;
    const void *weight, *bias;               /* (channels) f32, or NULL (1 / 0) */
    void *y;                                 /* forward output */
    void *mean, *rstd;                       /* (batch, seqlen) f32: written by the forward, read by the backward */
    const void *dy;                          /* backward input */
    void *dx;                                /* backward outputs */
    void *dweight, *dbias;                   /* (channels) f32 pre-zeroed, or NULL */
    void *workspace;                         /* backward scratch (see above), 16-byte aligned; contents undefined afterwards */
} vivim_layernorm_params;

/* ---- residual add fused with the LayerNorm above (MambaLayer's `x + drop_path(branch)` followed by norm2; opt-in) ----------
 * Write s[b] for scale[b], 1 when `scale` is NULL (the per-sample DropPath factor mask / keep).
 *   forward : x_new[b][c][t] = x[b][c][t] + s[b] * branch[b][t][c]   (one f32 fma, rounded once to itype; channel-major like x)
 *             y = LayerNorm over c of x_new AS STORED, token-major like `branch`; mean / rstd saved
 *   backward: dx[b][c][t] = LNbwd(dy; x_new, mean, rstd, weight) + dres[b][c][t]   (dres: the gradient reaching x_new from later in
 *             the network, channel-major; dy or dres may be NULL, not both), dbranch[b][t][c] = s[b] * dx (NULL: not wanted),
 *             dweight / dbias through `workspace` exactly as vivim_layernorm_cm_bwd
 * Add-only mode, weight == NULL: the forward writes x_new alone (y, mean, rstd are not touched); the backward writes
 * dbranch = s * dres transposed and nothing else (dx IS dres: the caller passes it on).
 * x, x_new, dres, dx: itype, unit token stride, 16-byte aligned rows, seqlen a whole number of 16-byte pieces.  branch, dbranch:
 * btype, unit channel stride; btype == itype, or itype f32 with an f16 / bf16 branch (what autocast produces).  y, dy: otype =
 * VIVIM_F32 or itype, unit channel stride.  channels <= 512; anything else returns VIVIM_ERR_UNSUPPORTED. */
typedef struct {
    int32_t batch, seqlen, channels;
    int32_t itype, btype, otype;
    float eps;
    int32_t _pad0;
    int64_t x_batch_stride, x_c_stride;              /* x: (batch, channels, seqlen) memory, token stride 1 */
    int64_t x_new_batch_stride, x_new_c_stride;      /* x_new: laid out like x (forward output, backward input) */
    int64_t branch_batch_stride, branch_token_stride;   /* branch: (batch, seqlen, channels), channel stride 1 */
    int64_t y_batch_stride, y_token_stride;          /* y and dy: (batch, seqlen, channels), channel stride 1 */
    int64_t dres_batch_stride, dres_c_stride;        /* dres, dx: laid out like x */
    int64_t dx_batch_stride, dx_c_stride;
    int64_t dbranch_batch_stride, dbranch_token_stride;
    const void *x, *branch;                          /* forward inputs */
    const void *scale;                               /* (batch) f32, or NULL (1) */
    const void *weight, *bias;                       /* (channels) f32; weight NULL selects the add-only mode, bias NULL is 0 */
    void *x_new;                                     /* written by the forward, read by the backward */
    void *y;                                         /* forward output */
    void *mean, *rstd;                               /* (batch, seqlen) f32: written by the forward, read by the backward */
    const void *dy, *dres;                           /* backward inputs */
    void *dx, *dbranch;                              /* backward outputs */
    void *dweight, *dbias;                           /* (channels) f32 pre-zeroed, or NULL */
    void *workspace;                                 /* vivim_add_layernorm_bwd_workspace_bytes() of scratch, 16-byte aligned */
} vivim_add_layernorm_params;

/* ---- weight-gradient products of the fused inner op's backward (mamba_ssm/ops/selective_scan_interface.py:273, 276) ------------
 * out[g][i][j] += sum_t a[g][i][t] * b[g][j][t]: both operands with unit stride along t (the grouped op keeps everything
 * channel-major), t = every token of every clip.  Replaces the two einsum calls there (ddelta_proj_weight: a = ddelta (d, B*l),
 * b = x_dbl[:, :R]^T; dx_proj_weight: a = dx_dbl^T, b = conv1d_out (d, B*l)) with a split-k MFMA kernel; f16 / bf16 operands,
 * f32 accumulation and output (pre-zeroed by the caller: the splits add atomically).  k % 8 == 0, 16-byte aligned rows. */
typedef struct {
    int32_t groups, m, n, k;
    int32_t itype;                              /* VIVIM_F16 or VIVIM_BF16, both operands */
    int32_t _pad0;
    int64_t a_group_stride, a_row_stride;       /* elements */
    int64_t b_group_stride, b_row_stride;
    int64_t out_group_stride, out_row_stride;   /* out: (groups, m, n) f32, unit stride along n */
    const void *a, *b;
    void *out;
} vivim_wgrad_nt_params;

/* ---- recall-focused segmentation loss: 0.4 * class-balanced focal + 0.6 * Tversky over softmax(logits) (opt-in) ---------------
 * The train step's loss (vivim_amd/train_step.py: recall_focused_loss) as three launches: partial sums, finalise, gradient.
 * Per pixel i of image n, classes c < C, label t; everything in f32, logits widened on load:
 *   m = max_c x_c    e_c = exp(x_c - m)    S = sum_c e_c    p_c = e_c / S    q_c = (sum_{k != c} e_k) / S   (never 1 - p_c)
 *   y_c = (t == c)   -- labels are only COMPARED with c, never used as an index: a label outside [0, C) gives y_c = 0 for every c
 *   phi = sum_c alpha_c * ( y_c ? q_c^2 * -ln(p_c + eps) : p_c^2 * -ln(q_c + eps) )                       (gamma = 2)
 *   TP[n,c] = sum_i y_c p_c    FP[n,c] = sum_i (1 - y_c) p_c    FN[n,c] = sum_i y_c q_c
 *   den = TP + tversky_alpha * FP + tversky_beta * FN + smooth
 *   loss = focal_weight * sum_{n,i} phi / (N * pixels) + tversky_weight * (1 - sum_{n,c} ((TP + smooth) / den) / (N * C))
 * forward : writes loss (one f32) and, unless coef is NULL, coef[n][c] = { G1, G0 } = d((TP + smooth) / den) / d p_c at a pixel of
 *           class c / of another class:  G1 = (den - (TP + smooth) * (1 - tversky_beta)) / den^2,  G0 = -(TP + smooth) * tversky_alpha / den^2
 * backward: g_c = focal_weight / (N * pixels) * alpha_c * ( y_c ?  2 q_c ln(p_c + eps) - q_c^2 / (p_c + eps)
 *                                                               : -2 p_c ln(q_c + eps) + p_c^2 / (q_c + eps) )
 *                 - tversky_weight / (N * C) * ( y_c ? G1 : G0 )
 *           dlogits_c = *grad_out * p_c * ( q_c * g_c - sum_{k != c} p_k g_k )      the softmax is recomputed, nothing is kept per pixel;
 *           *grad_out is read on the device (no host synchronisation) and multiplied in f32 before the one rounding to itype.
 * Determinism: no float atomics.  Every workgroup stores its partial sums into slot (image, block) of `workspace` and one
 * workgroup adds the slots in slot order, so loss, coef and dlogits are pure functions of the inputs and the shape.
 * logits, dlogits: (batch, classes, pixels) with unit pixel stride, itype; 16-byte vectors where base and strides allow, element
 * accesses otherwise (any alignment of the element type is accepted).  target: (batch, pixels), unit pixel stride.
 * classes outside 2..8 and gamma != 2 return VIVIM_ERR_UNSUPPORTED. */
typedef struct {
    int32_t batch, classes, pixels;
    int32_t itype;                                   /* logits / dlogits: vivim_dtype_t */
    int32_t ttype;                                   /* target: 0 = int64, 1 = uint8 */
    float gamma;                                     /* 2 */
    float focal_weight, tversky_weight;              /* 0.4, 0.6 in the train step */
    float tversky_alpha, tversky_beta, smooth, eps;  /* 0.3, 0.7, 1e-6, 1e-6 */
    int64_t logits_batch_stride, logits_c_stride;    /* elements */
    int64_t dlogits_batch_stride, dlogits_c_stride;
    int64_t target_batch_stride;
    const void *logits, *target;
    const void *alpha;                               /* (classes) f32 class weights of the focal term */
    void *loss;                                      /* one f32: forward output */
    void *coef;                                      /* (batch, classes, 2) f32: forward output (NULL: not wanted), backward input */
    void *workspace;                                 /* forward scratch, vivim_seg_loss_workspace_bytes() of it, 4-byte aligned */
    int64_t workspace_bytes;
    const void *grad_out;                            /* one f32 on the device: backward input */
    void *dlogits;                                   /* backward output */
} vivim_seg_loss_params;

/* ---- Validation metrics of a batch of logits (vivim_seg_metrics; csrc/seg_metrics.hip): argmax + confusion counts ----------
 * Per pixel i of image n: pred = the FIRST index of the maximum of the C logits, compared in their own values (widening to f32 is
 * exact); a NaN counts as the maximum and the first NaN wins (numpy.argmax's rule; no softmax).  With the label t:
 *   tp[n,c] = #(pred == c and t == c)    fp[n,c] = #(pred == c and t != c)    fn[n,c] = #(pred != c and t == c)
 * Labels are only COMPARED with c: a label outside [0, C) is a pixel of no class and adds to fp of the class predicted there only.
 * Outputs: counts (batch, classes, 3) int32 = {tp, fp, fn}; pred (optional) the prediction map, one uint8 per pixel; state
 * (optional) (classes, 7) f64, owned and zeroed by the caller, ADDED into: for n = 0 .. batch-1 in that order and every class
 * present in image n's label map (tp + fn > 0), with HW = pixels and tn = HW - tp - fp - fn,
 *   state[c][0] += dice        = 2 tp / (2 tp + fp + fn)              state[c][1] += jaccard = tp / (tp + fp + fn)
 *   state[c][2] += precision   = tp + fp == 0 ? 0 : tp / (tp + fp)    state[c][3] += recall  = tp / (tp + fn)
 *   state[c][4] += f_measure   = 2 precision recall / (precision + recall + 1e-5)
 *   state[c][5] += specificity = tp + fn == HW ? 0 : tn / (tn + fp)   state[c][6] += 1
 * Determinism: integer counts, no atomics; every workgroup stores its counts into slot (image, block) of `workspace`, one
 * workgroup adds the slots in slot order, and the order over n is fixed, so counts, pred and state are pure functions of the inputs.
 * logits: (batch, classes, pixels) with unit pixel stride, itype; 16-byte vectors where base and strides allow, element accesses
 * otherwise.  target: (batch, pixels), pred: (batch, pixels), unit pixel stride.  classes outside 2..8 return VIVIM_ERR_UNSUPPORTED. */
typedef struct {
    int32_t batch, classes, pixels;
    int32_t itype;                                   /* logits: vivim_dtype_t */
    int32_t ttype;                                   /* target: 0 = int64, 1 = uint8 */
    int32_t _pad0;
    int64_t logits_batch_stride, logits_c_stride;    /* elements */
    int64_t target_batch_stride, pred_batch_stride;
    const void *logits, *target;
    void *counts;                                    /* (batch, classes, 3) int32, 4-byte aligned */
    void *pred;                                      /* (batch, pixels) uint8, any alignment; NULL: not wanted */
    void *state;                                     /* (classes, 7) f64, 8-byte aligned, added into; NULL: not wanted */
    void *workspace;                                 /* vivim_seg_metrics_workspace_bytes() of it, 4-byte aligned */
    int64_t workspace_bytes;
} vivim_seg_metrics_params;

/* ---- Bilinear 2-D upsampling, align_corners = False, no explicit scale factors (csrc/upsample.hip; opt-in in Vivim) ----------
 * ATen's definition, per axis in fp32:  r = float(n_in) / float(n_out);  src = max(0, r * (o + 0.5) - 0.5);  i0 = (int)src;
 * i1 = i0 + (i0 < n_in - 1);  l1 = src - i0;  l0 = 1 - l1.
 *   forward : y[oh][ow] = l0h * (l0w * x[i0h][i0w] + l1w * x[i0h][i1w]) + l1h * (l0w * x[i1h][i0w] + l1w * x[i1h][i1w]), fp32, rounded
 *             once to itype
 *   backward: dx = the transpose of that linear map applied to dy, in GATHER form: every dx element adds, in ascending output
 *             order, the dy elements whose taps (recomputed with the forward's own expressions) name it.
 * Determinism: no atomics and no workspace; y and dx are pure functions of the inputs and the shape.
 * layout 0, planes: x / dx are (batch, channels, in_h, in_w) and y / dy (batch, channels, out_h, out_w), each image contiguous.
 * layout 1, channels-last: x / dx are (batch, in_h, in_w, channels) MEMORY and y / dy (batch, out_h, out_w, channels), each image
 * dense; 16-byte accesses when channels is a whole number of them and bases and batch strides are 16-byte aligned, element
 * accesses otherwise (element-size alignment is the only requirement).  Batch strides are free, in elements.
 * Upsampling only: out_h >= in_h and out_w >= in_w, else VIVIM_ERR_UNSUPPORTED.  An image (channels * h * w elements, input and
 * output), (2 * n_in + 3) * n_out per axis and the number of workgroups must fit 31 bits, else VIVIM_ERR_INVALID. */
typedef struct {
    int32_t batch, channels, in_h, in_w, out_h, out_w;
    int32_t itype;                                   /* x, y, dy, dx: vivim_dtype_t */
    int32_t layout;                                  /* 0 = planes, 1 = channels-last */
    int64_t x_batch_stride, y_batch_stride;          /* of x and dx / of y and dy, in elements */
    const void *x;                                   /* forward input */
    void *y;                                         /* forward output */
    const void *dy;                                  /* backward input */
    void *dx;                                        /* backward output */
} vivim_upsample_params;

/* ---- Eval-mode decode head: upsample, add, ReLU and the class projection in one kernel (csrc/decode_head.hip; opt-in in Vivim) --
 * With BatchNorm's running statistics, linear_fuse and the per-stage projections folded into the maps m_s (vivim_amd/decode_head.py):
 *   h[k]      = max(0, bias[k] + sum over maps s of  l0h * (l0w * m_s[i0h][i0w][k] + l1w * m_s[i0h][i1w][k])
 *                                                  + l1h * (l0w * m_s[i1h][i0w][k] + l1w * m_s[i1h][i1w][k]))        fp32
 *   logits[c] = b_out[c] + sum over k of w_out[c][k] * h[k]                                        fp32, rounded once to itype
 * per output pixel, the taps (i0, i1, l0, l1) per axis being those of the bilinear upsampling above (in_h = map_h[s],
 * out_h = out_h, likewise for w).  A map of the output's own size is read with one tap of weight 1.
 * maps[s]: (batch, map_h[s], map_w[s], hidden) MEMORY, each image dense (channels-last), n_maps of them (1..4); logits:
 * (batch, classes, out_h, out_w), each image contiguous planes.  Batch strides are free, in elements, and at least one image.
 * bias (hidden), w_out (classes, hidden) and b_out (classes; NULL: zeros) are contiguous fp32.
 * 16-byte accesses to the maps when hidden is a whole number of them and every map's base and batch stride are 16-byte
 * aligned, element accesses otherwise (element-size alignment is the only requirement).
 * Determinism: no atomics and no workspace; every logit is reduced by one wave in a fixed order.
 * Limits: 1 <= classes <= 8 and 1 <= hidden <= 1024 (bias and w_out live in LDS), else VIVIM_ERR_INVALID; a map larger than
 * the output on an axis returns VIVIM_ERR_UNSUPPORTED; an image of any map or of the logits and the number of workgroups
 * (batch * ceil(out_h / 8) * ceil(out_w / 8)) must fit 31 bits, else VIVIM_ERR_INVALID.
 * This struct has no vivim_sizeof row: the caller sets struct_bytes = sizeof(vivim_decode_head_params) and any other value is
 * refused with VIVIM_ERR_INVALID. */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_decode_head_params) as the caller compiled it */
    int32_t batch, hidden, classes, n_maps, out_h, out_w;
    int32_t itype;                                   /* maps and logits: vivim_dtype_t */
    int32_t map_h[4], map_w[4];
    int64_t map_batch_stride[4];                     /* in elements */
    int64_t logits_batch_stride;
    const void *maps[4];
    const void *bias, *w_out, *b_out;                /* fp32 */
    void *logits;
} vivim_decode_head_params;

/* ---- LayerNorm over the channels of TOKEN-major rows (csrc/token_layernorm.hip; the SegFormer blocks' norms, opt-in in Vivim) --
 * x is `rows` rows of `channels` elements, channel stride 1, one row stride (a (B, N, C) tensor whose leading dimensions collapse).
 *   forward : y[r][c] = (x[r][c] - mean[r]) * rstd[r] * weight[c] + bias[c]     fp32, rounded once to otype
 *             mean[r] = sum_c x[r][c] / channels, rstd[r] = 1 / sqrt(sum_c (x[r][c] - mean[r])^2 / channels + eps): the mean first,
 *             then the squared differences from it, on the row held in registers (never E[x^2] - mean^2).  mean / rstd are
 *             written when both are given; both NULL is the call no backward follows.
 *   backward: dx[r][c] = rstd[r] * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * weight, xhat = (x - mean) * rstd, in itype;
 *             dweight[c] = sum_r dy * xhat, dbias[c] = sum_r dy: WRITTEN, not added to (no pre-zeroing), either may be NULL.
 * Determinism: no atomics.  Every workgroup of the backward stores its partial dweight / dbias sums into its own slot of
 * `workspace` and a second kernel on the same stream adds the slots in slot order, so the results are a function of the inputs
 * and the shape alone.  Workspace, required when dweight or dbias is given (vivim_token_layernorm_bwd_workspace_bytes):
 *     min(1024, ceil(rows / 4)) slots * 2 * channels * sizeof(float)  bytes, 4-byte aligned; contents undefined afterwards.
 * Types: x, dx: itype; y, dy: otype; weight, bias, mean, rstd, dweight, dbias: fp32.  otype == itype, otype == VIVIM_F32, or
 * itype == VIVIM_F32 with an f16 / bf16 otype (the consumer's autocast cast done in the kernel); any other pair and
 * channels > 1024 return VIVIM_ERR_UNSUPPORTED.  Row strides are in elements and at least `channels`.
 * 16-byte accesses when channels is a whole number of 16-byte pieces of itype and every address and row stride of the call is
 * 16-byte aligned; element accesses otherwise (element-size alignment is then the only requirement).
 * This struct has no vivim_sizeof row: the caller sets struct_bytes = sizeof(vivim_token_layernorm_params) and any other value
 * is refused with VIVIM_ERR_INVALID. */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_token_layernorm_params) as the caller compiled it */
    int32_t rows, channels;
    int32_t itype, otype;                            /* vivim_dtype_t */
    float eps;
    int64_t x_row_stride, y_row_stride;              /* in elements; channel stride 1 everywhere */
    int64_t dy_row_stride, dx_row_stride;
    const void *x;
    const void *weight, *bias;                       /* (channels) f32; bias NULL is 0 */
    void *y;                                         /* forward output */
    void *mean, *rstd;                               /* (rows) f32: written by the forward (or both NULL), read by the backward */
    const void *dy;                                  /* backward input */
    void *dx;                                        /* backward outputs */
    void *dweight, *dbias;                           /* (channels) f32, written; or NULL */
    void *workspace;                                 /* backward scratch (see above) */
} vivim_token_layernorm_params;

/* ---- Residual add + LayerNorm / RMSNorm over TOKEN-major rows (csrc/token_layernorm.hip: the same kernels as above with the
 * residual part compiled in; `hidden = drop_path(branch) + residual; LayerNorm(hidden)` of the SegFormer blocks, opt-in in Vivim) --
 * All tensors are `rows` rows of `channels` elements, channel stride 1, one row stride each.
 *   forward : h[r][c] = res[r][c] + scale[r / rows_per_sample] * branch[r][c]      fp32, rounded once to rtype -> res_out
 *             res NULL: h = scale * branch (rounded to rtype when res_out is given); scale NULL: a factor of 1.
 *             Statistics and y are taken from h AS STORED (the backward recomputes from the saved res_out):
 *             LayerNorm (rms = 0): y = (h - mean) * rstd * weight + bias, the mean first, then the squared differences from it;
 *             RMSNorm   (rms = 1): y = h * rstd * weight (+ bias), rstd = 1 / sqrt(sum_c h^2 / channels + eps), mean is written as 0.
 *             weight NULL: the add alone -- res_out is written, y / mean / rstd are not touched.
 *             mean / rstd are written when both are given; both NULL is the call no backward follows.
 *   backward: dh = LNbwd(dy) + dres, LNbwd as vivim_token_layernorm_bwd (RMS: rstd * (g - xhat * mean_c(g * xhat)), xhat = h * rstd,
 *             g = dy * weight); dy (gradient of y) or dres (gradient arriving at res_out) may be NULL, not both.
 *             dres_in = dh in rtype, dbranch = scale * dh in btype (exactly 0 where scale is 0); each written when given.
 *             dweight[c] = sum_r dy * xhat, dbias[c] = sum_r dy: WRITTEN through the slots, as above, either may be NULL.
 *             weight NULL: the add's backward alone -- dy must be NULL, res_out / mean / rstd are not read.
 * Types: branch, y, dy, dbranch: btype; res, res_out, dres, dres_in: rtype; scale, weight, bias, mean, rstd, dweight, dbias: fp32.
 * (btype, rtype) is (f32, f32), (f16, f16), (bf16, bf16), (f16, f32) or (bf16, f32); any other pair and channels > 1024 return
 * VIVIM_ERR_UNSUPPORTED.  Row strides are in elements and at least `channels`; only those of given tensors are looked at.
 * scale is (rows / rows_per_sample) fp32; with it rows_per_sample > 0 must divide rows.
 * Determinism and workspace: as vivim_token_layernorm_params (vivim_token_add_norm_bwd_workspace_bytes, the same formula).
 * 16-byte accesses when channels is a whole number of 16-byte pieces of the narrower of the two types and every address and
 * row stride of the call is 16-byte aligned, each stream checked on its own; element accesses otherwise.
 * No vivim_sizeof row: the caller sets struct_bytes = sizeof(vivim_token_add_norm_params), any other value is refused. */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_token_add_norm_params) as the caller compiled it */
    int32_t rows, channels, rows_per_sample;
    int32_t btype, rtype, otype;                     /* vivim_dtype_t; otype must equal btype */
    int32_t rms;                                     /* 0 LayerNorm, 1 RMSNorm */
    float eps;
    int32_t _pad0;
    int64_t branch_row_stride, res_row_stride, res_out_row_stride, y_row_stride;      /* in elements */
    int64_t dy_row_stride, dres_row_stride, dres_in_row_stride, dbranch_row_stride;
    const void *branch;                              /* forward input */
    const void *res;                                 /* forward input or NULL */
    const void *scale;                               /* (rows / rows_per_sample) f32 or NULL */
    const void *weight, *bias;                       /* (channels) f32; weight NULL: the add alone; bias NULL is 0 */
    void *res_out;                                   /* forward output; the backward reads it */
    void *y;                                         /* forward output */
    void *mean, *rstd;                               /* (rows) f32: written by the forward (or both NULL), read by the backward */
    const void *dy, *dres;                           /* backward inputs; one may be NULL */
    void *dres_in, *dbranch;                         /* backward outputs, each or NULL */
    void *dweight, *dbias;                           /* (channels) f32, written; or NULL */
    void *workspace;                                 /* backward scratch (see above) */
} vivim_token_add_norm_params;

/* ---- Fused clip + AdamW step (csrc/optimizer.hip; vivim_amd/optimizer.py: FusedStepAdamW, opt-in) ----------------------------
 * The optimizer end of a train step without a host synchronisation: unscale, non-finite detection, global L2 norm, clipping,
 * AdamW with decoupled weight decay, the step counter and GradScaler's dynamic loss scale.  All tensors are dense fp32.
 *
 * The record (`state`): VIVIM_OPT_STATE_WORDS 4-byte words on the device, owned by the caller, zero except word 0 at the start:
 *   0 f32 loss scale (65536 for fp16 training, 1 otherwise)   1 i32 growth counter (good scaled steps since the last change)
 *   2 i32 step count t (steps applied, shared by all tensors) 3 f32 total norm of the unscaled gradients, last statistics pass
 *   4 i32 found_inf of the last step                          5 f32 factor every gradient of the last step was multiplied with
 *   6 f32 bc1 = 1 - beta1^t                                   7 f32 bc2s = sqrt(1 - beta2^t)
 *   8 i32 skipped steps                                       9 f32 clip coefficient of the last step     10 .. 15 reserved (0)
 *
 * The tables.  `params`, `exp_avg`, `exp_avg_sq` are DEVICE arrays of device pointers, one entry per tensor of the whole list;
 * `block_map` is a DEVICE array of total_blocks (tensor, chunk) int32 pairs, tensors ascending: workgroup b works on elements
 * chunk * VIVIM_OPT_CHUNK .. of its tensor.  They change only when a tensor moves and are built once.  The gradients' addresses
 * change every step: `grads` and `numel` are HOST arrays of `count` entries for tensors first_tensor .. first_tensor + count - 1,
 * copied into the kernel arguments of the launch (at most VIVIM_OPT_MAX_TENSORS per call, under 4 KB; nothing is staged, the
 * arrays may be reused as soon as the call returns).  A longer list is cut into several calls, each with the map rows
 * first_block .. first_block + n_blocks - 1 of its own tensors.  A NULL gradient leaves its tensor out of the step.
 *
 *   vivim_opt_grad_stats: per map row, sum (g * inv_scale)^2 in fp32 (inv_scale = 1 / record[0] when `scaled`, else 1; a
 *     thread's chain is 16 additions, then a wave and a workgroup sum) and whether any g is inf / nan, STORED into slot
 *     `row` of the workspace (2 words per row; vivim_opt_step_workspace_bytes = 8 * total_blocks).  No atomics.
 *   vivim_opt_finalise (one workgroup): adds slots 0 .. total_blocks - 1 in a fixed order in fp64; norm = sqrt(sum);
 *     found_inf = any flag or a non-finite sum; clip = has_max_norm ? min(1, max_norm / (norm + 1e-6)) : 1;
 *     factor = found_inf ? 0 : inv_scale * clip; unless found_inf: t += 1, bc1 and bc2s recomputed in fp64; else skipped += 1.
 *     When `scaled`: found_inf halves the scale and zeroes the growth counter, otherwise the counter is incremented and at
 *     2000 the scale is doubled and the counter zeroed.  total_blocks = 0: no statistics pass was made -- found_inf = 0,
 *     clip = 1, factor = inv_scale, the norm is left as it was; t, bc1, bc2s advance.
 *   vivim_opt_adamw: nothing is written when record[4] is set; otherwise per element, fp32, one rounding per stored value:
 *     g' = g * factor;  m' = m + (1 - beta1)(g' - m);  v' = beta2 v + (1 - beta2) g'^2;
 *     p' = p (1 - lr * weight_decay) - (lr / bc1) * m' / (sqrt(v') / bc2s + eps).
 *     The constants (1 - beta1), (1 - beta2), (1 - lr * weight_decay) are formed in double and rounded once.
 * 16-byte accesses where the addresses of a chunk are 16-byte aligned, element accesses otherwise and for a chunk's tail.
 * Everything is bit-repeatable.  No vivim_sizeof row: the caller sets struct_bytes = sizeof(vivim_opt_step_params). */
#define VIVIM_OPT_CHUNK 4096           /* elements per workgroup and map row */
#define VIVIM_OPT_MAX_TENSORS 248      /* tensors per call */
#define VIVIM_OPT_STATE_WORDS 16
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_opt_step_params) as the caller compiled it */
    int32_t count;                                   /* tensors of this call: 1 .. VIVIM_OPT_MAX_TENSORS */
    int32_t first_tensor;                            /* their position in the device tables */
    int32_t first_block, n_blocks;                   /* this call's rows of block_map */
    int32_t total_blocks;                            /* rows of block_map = slots of the workspace, all calls of a step together */
    int32_t scaled;                                  /* gradients carry the loss scale: unscale, run the scale policy */
    int32_t has_max_norm;
    double max_norm;
    double lr, beta1, beta2, eps, weight_decay;
    const void *const *grads;                        /* HOST array [count] of device pointers; NULL = no gradient this step */
    const int64_t *numel;                            /* HOST array [count], each > 0 */
    const void *params, *exp_avg, *exp_avg_sq;       /* DEVICE arrays of device pointers */
    const void *block_map;                           /* DEVICE int32 [total_blocks][2] */
    void *state;                                     /* DEVICE record */
    void *workspace;                                 /* DEVICE, 8 * total_blocks bytes, 8-byte aligned */
    int64_t workspace_bytes;
} vivim_opt_step_params;

/* ---- Master weights: the fused step for fp16 / bf16 parameters (vivim_amd/optimizer.py: FusedStepAdamW(master_weights=True)) ---
 * The model's parameter and its gradient are 16-bit tensors of type `dtype` (1 = VIVIM_F16, 2 = VIVIM_BF16); the value the
 * optimizer owns is an fp32 master.  vivim_opt_mw_params is vivim_opt_step_params field for field, then `masters` -- a DEVICE
 * array of device pointers like `params`, one entry per tensor of the whole list (entries of fp32 tensors are not read) -- and
 * `dtype`.  A call is homogeneous: every tensor first_tensor .. first_tensor + count - 1 has that type; the caller orders its
 * tables by type (fp32, fp16, bf16), cuts them so that no call straddles two, and sends the fp32 cuts to the entry points above.
 * The record, the block map, the workspace (and its query) and vivim_opt_finalise are shared by all cuts of a step.
 *
 *   vivim_opt_grad_stats_mw: as vivim_opt_grad_stats on g widened to fp32 (exact); the non-finite test reads the widened value.
 *   vivim_opt_adamw_mw: nothing is written when record[4] is set; otherwise g' = float(g) * factor, and m', v' and
 *     master' = master (1 - lr * weight_decay) - (lr / bc1) * m' / (sqrt(v') / bc2s + eps) by the arithmetic above, unchanged;
 *     master', m', v' are stored and params[i] receives p16 = master' rounded to nearest even (fp16: overflow gives +-inf,
 *     subnormals are rounded, not flushed) -- the 16-bit value autocast's cast of an fp32 parameter would have produced.
 * A thread works on the same four consecutive elements as in the fp32 kernels (8-byte accesses of the 16-bit tensors where
 * g and p16 are 8-byte and master, m, v 16-byte aligned; element accesses otherwise), and the sums run in the same order: the
 * results equal those of the fp32 entry points given the widened gradients, bit for bit.  Per element 2 + 12 bytes are read and
 * 12 + 2 written: the 28 bytes of the fp32 step.  The caller sets struct_bytes = sizeof(vivim_opt_mw_params). */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_opt_mw_params) as the caller compiled it */
    int32_t count;
    int32_t first_tensor;
    int32_t first_block, n_blocks;
    int32_t total_blocks;
    int32_t scaled;
    int32_t has_max_norm;
    double max_norm;
    double lr, beta1, beta2, eps, weight_decay;
    const void *const *grads;                        /* HOST array [count] of device pointers to `dtype` gradients; NULL = none */
    const int64_t *numel;                            /* HOST array [count], each > 0 */
    const void *params, *exp_avg, *exp_avg_sq;       /* DEVICE arrays of device pointers: `dtype` parameters, fp32 moments */
    const void *block_map;
    void *state;
    void *workspace;
    int64_t workspace_bytes;
    const void *masters;                             /* DEVICE array of device pointers: the fp32 masters */
    int32_t dtype;                                   /* 1 = VIVIM_F16, 2 = VIVIM_BF16 */
    int32_t _pad0;
} vivim_opt_mw_params;

int vivim_abi_version(void);
const char *vivim_last_error(void);

/* sizeof() of a params struct as this library was compiled, so a foreign-language binding can assert
 * its own layout: which = 0 ssm_fwd, 1 ssm_bwd, 2 conv_fwd, 3 conv_bwd, 4 dwconv, 5 dwconv_wgrad, 6 dir, 7 conv_update,
 * 8 state_update, 9 layernorm, 10 wgrad_nt, 11 add_layernorm, 12 seg_loss, 13 seg_metrics, 14 upsample; 0 for anything else. */
size_t vivim_sizeof(int which);

/* Tokens per checkpoint row of `x`: n_chunks = ceil(seqlen / vivim_scan_ckpt_len(f)).  Depends on the sizes and flags in
 * `f` (not on its pointers) and on the forward tuning value: 16 * (dstate / 16) for the shapes the lanes = states
 * backward takes (variable B / C, dstate 16 / 32 / 64), vivim_scan_chunk_len() otherwise.  The forward call, the
 * backward call and the allocation of `x` must see the same value. */
int vivim_scan_ckpt_len(const vivim_ssm_fwd_params *f);
/* The checkpoint length of the shapes the call above does not special-case. */
int vivim_scan_chunk_len(int itype);

/* Scratch the backward wants for splitting the token axis over workgroups (carries of the reverse
 * recurrence per (batch, channel, segment, state)); depends only on the sizes in `f`. */
size_t vivim_scan_bwd_workspace_bytes(const vivim_ssm_fwd_params *f);
/* Scratch the forward wants for its token-axis split (per-segment end states); 0 when the shape takes a kernel
 * that needs none. */
size_t vivim_scan_fwd_workspace_bytes(const vivim_ssm_fwd_params *f);

/* Kernel-selection override for tuning and tests: which = 0 forward scan (0 automatic, 1 n-split K=8, 2 n-split K=4,
 * 3 generic, 5 lanes=channels, 6 lanes=states), which = 1 backward scan (0 automatic, 1 / 2 lanes=tokens kernel with
 * 8 / 4 waves per workgroup, 3 generic, 4 lanes=states first generation, 5 lanes=states second generation = what
 * automatic takes for dstate 16 on 16-byte aligned rows).  Forward values 1-3 also select the long checkpoint rows
 * (vivim_scan_ckpt_len), which the lanes=states backward cannot use.  Returns the previous value, -1 on a bad argument.  Initial values come from VIVIM_FWD_VARIANT / VIVIM_BWD_VARIANT.  The forward workspace size depends on
 * the forward setting: query it after changing it. */
int vivim_set_tuning(int which, int value);

int vivim_selective_scan_fwd(const vivim_ssm_fwd_params *p, void *stream);
/* The forward for a call no backward follows (inference, torch.no_grad): the same kernels, family choice and token-axis
 * cut as vivim_selective_scan_fwd on the same tensors with an `out` laid out like `delta`, hence bit-identical results,
 * but no checkpoint tensor is written and, when z is given, no `out`: p->x must be NULL; with z, p->out_z is required and
 * p->out must be NULL; without z, p->out is required.  `last_state` is NULL or a contiguous fp32 (batch, dim, dstate)
 * buffer that receives the state after the last token (what the full call leaves in the last row of x).  Same workspace
 * contract and query (vivim_scan_fwd_workspace_bytes), same vivim_set_tuning(0, ...) override. */
int vivim_selective_scan_fwd_lean(const vivim_ssm_fwd_params *p, void *last_state, void *stream);
int vivim_selective_scan_bwd(const vivim_ssm_bwd_params *p, void *stream);
int vivim_causal_conv1d_fwd(const vivim_conv_fwd_params *p, void *stream);
int vivim_causal_conv1d_bwd(const vivim_conv_bwd_params *p, void *stream);
int vivim_dwconv_fwd(const vivim_dwconv_params *p, void *stream);            /* also the input gradient (flip = 1) */
int vivim_dwconv_wgrad(const vivim_dwconv_wgrad_params *p, void *stream);
int vivim_dir_scatter(const vivim_dir_params *p, void *stream);
int vivim_dir_gather(const vivim_dir_params *p, void *stream);
int vivim_causal_conv1d_update(const vivim_conv_update_params *p, void *stream);
int vivim_selective_state_update(const vivim_state_update_params *p, void *stream);
int vivim_layernorm_cm_fwd(const vivim_layernorm_params *p, void *stream);
int vivim_layernorm_cm_bwd(const vivim_layernorm_params *p, void *stream);
size_t vivim_layernorm_bwd_workspace_bytes(const vivim_layernorm_params *p);   /* from batch, seqlen, channels, itype */
int vivim_wgrad_nt(const vivim_wgrad_nt_params *p, void *stream);
int vivim_add_layernorm_cm_fwd(const vivim_add_layernorm_params *p, void *stream);
int vivim_add_layernorm_cm_bwd(const vivim_add_layernorm_params *p, void *stream);
size_t vivim_add_layernorm_bwd_workspace_bytes(const vivim_add_layernorm_params *p);   /* from batch, seqlen, channels, itype */
int vivim_seg_loss_fwd(const vivim_seg_loss_params *p, void *stream);
int vivim_seg_loss_bwd(const vivim_seg_loss_params *p, void *stream);
size_t vivim_seg_loss_workspace_bytes(const vivim_seg_loss_params *p);   /* from batch, classes, pixels, itype; 0 on bad sizes */
int vivim_seg_metrics(const vivim_seg_metrics_params *p, void *stream);
size_t vivim_seg_metrics_workspace_bytes(const vivim_seg_metrics_params *p);   /* from batch, classes, pixels, itype; 0 on bad sizes */
int vivim_upsample_bilinear2d_fwd(const vivim_upsample_params *p, void *stream);   /* reads x, writes y */
int vivim_upsample_bilinear2d_bwd(const vivim_upsample_params *p, void *stream);   /* reads dy, writes dx */
int vivim_decode_head_fwd(const vivim_decode_head_params *p, void *stream);        /* reads the maps, writes logits */
int vivim_token_layernorm_fwd(const vivim_token_layernorm_params *p, void *stream);   /* reads x, writes y (+ mean, rstd) */
int vivim_token_layernorm_bwd(const vivim_token_layernorm_params *p, void *stream);   /* writes dx (+ dweight, dbias) */
size_t vivim_token_layernorm_bwd_workspace_bytes(const vivim_token_layernorm_params *p);   /* from rows, channels; 0 on bad sizes */
int vivim_token_add_norm_fwd(const vivim_token_add_norm_params *p, void *stream);   /* writes res_out (+ y, mean, rstd) */
int vivim_token_add_norm_bwd(const vivim_token_add_norm_params *p, void *stream);   /* writes dres_in, dbranch (+ dweight, dbias) */
size_t vivim_token_add_norm_bwd_workspace_bytes(const vivim_token_add_norm_params *p);   /* from rows, channels; 0 on bad sizes */
int vivim_opt_grad_stats(const vivim_opt_step_params *p, void *stream);   /* reads the gradients, writes this call's slots */
int vivim_opt_finalise(const vivim_opt_step_params *p, void *stream);     /* reads the slots, updates the record */
int vivim_opt_adamw(const vivim_opt_step_params *p, void *stream);        /* reads the record and g, updates p, m, v */
size_t vivim_opt_step_workspace_bytes(const vivim_opt_step_params *p);    /* from total_blocks; 0 on bad sizes */
int vivim_opt_grad_stats_mw(const vivim_opt_mw_params *p, void *stream);  /* 16-bit gradients; writes this call's slots */
int vivim_opt_adamw_mw(const vivim_opt_mw_params *p, void *stream);       /* updates master, m, v; writes the 16-bit p */

/* Deterministic backward (for torch.use_deterministic_algorithms).  Same parameters, checks and results as
 * vivim_selective_scan_bwd, and the same kernel family, but every gradient that the default call adds up across
 * workgroups with float atomics (dA, dD, ddelta_bias, dB, dC) is a pure function of the inputs, the shapes and the
 * vivim_set_tuning values: each contributing workgroup stores its partial sum into its own slot of `det_ws` (slot
 * index from its coordinates, never from arrival order), and one fixed-order kernel adds the slots to the outputs.
 * The outputs must be pre-zeroed as for the default call; the contents of `det_ws` on entry do not matter and are
 * undefined afterwards.  A NULL, misaligned (< 16 bytes) or too small `det_ws` returns VIVIM_ERR_INVALID before
 * anything is launched.  The dB / dC adds of the lanes = states kernels stay when a B/C group has at most two
 * workgroups: 0 + a + b == 0 + b + a exactly.
 *
 * Workspace, in floats (depends on the sizes and flags in `f` and the tuning values, not on pointers): the larger of
 * the generic family's and the family the shape's plan prefers, where for slot counts SA (dA / dD / dbias) and
 * SB (dB / dC) a family needs  SA * dim * (dstate + 2) + 2 * SB * EB:
 *   generic:           SA = batch;  variable B/C: SB = ceil(dim / n_groups / 2), EB = batch * n_groups * dstate * seqlen;
 *                      constant B/C: SB = batch, EB = dim * dstate;
 *   lanes = tokens:    SA = batch * segments;  SB = workgroups per B/C group, EB = batch * n_groups * dstate * seqlen;
 *   lanes = states:    SA = batch * segments;  SB = workgroups per B/C group if more than two, else 0. */
size_t vivim_scan_bwd_det_workspace_bytes(const vivim_ssm_fwd_params *f);
/* The exact workspace of one call: the formula above for the family this call's pointers select (never more than the
 * shape-level bound above; 0 on bad params).  vivim_selective_scan_bwd_det accepts any workspace of at least this size.
 * The lanes = tokens kernel at 8 tokens per lane runs with 4-wave workgroups in this mode (the 8-wave build has no VGPR
 * left for the slot stores); it re-segments for that width and runs unsegmented (S = 1) if p->workspace is too small
 * for that segmentation (vivim_scan_bwd_workspace_bytes sizes it for the default plan). */
size_t vivim_scan_bwd_det_call_workspace_bytes(const vivim_ssm_bwd_params *p);
int vivim_selective_scan_bwd_det(const vivim_ssm_bwd_params *p, void *det_ws, size_t det_ws_bytes, void *stream);

/* Deterministic causal conv1d backward: same parameters, checks and dx as vivim_causal_conv1d_bwd; dweight / dbias
 * (pre-zeroed) come from per-(batch, token chunk) slots added in fixed order, no float atomics.  Workspace:
 * slots * dim * (width + 1) floats, slots = batch * ceil(seqlen / (256 * 16 / sizeof(itype))) for channel-first x and
 * batch * (token chunks of the channel-last kernel) for channel-last x.  Contract on det_ws as for the scan above. */
size_t vivim_causal_conv1d_bwd_det_workspace_bytes(const vivim_conv_fwd_params *f);
int vivim_causal_conv1d_bwd_det(const vivim_conv_bwd_params *p, void *det_ws, size_t det_ws_bytes, void *stream);
/* Deterministic depthwise-conv weight gradient: as vivim_dwconv_wgrad, dwt / dbias (pre-zeroed) from per-(batch,
 * token block) slots of (kd * 9 + 1) * channels floats added in fixed order.  Contract on det_ws as above. */
size_t vivim_dwconv_wgrad_det_workspace_bytes(const vivim_dwconv_wgrad_params *p);
int vivim_dwconv_wgrad_det(const vivim_dwconv_wgrad_params *p, void *det_ws, size_t det_ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VIVIM_HIP_H */
