// ops.cuh -- every vivim:: function that one .hip file defines and another calls (the scan's family launches excepted:
// scan_plan.cuh).  capi.hip includes it to call them and each defining file includes it too, so a declaration that no
// longer matches its definition does not compile.
//
// capi.hip refuses arguments before anything is launched; the functions here launch.  A *_dispatch returns false where no
// kernel is built for the call's types (capi has refused those, so this is a second line), a *_det_dispatch a Launch (det.cuh).
#pragma once
#include "det.cuh"
// every extension header: one per feature added after ABI version 8, each includes vivim_hip.h
#include "../../include/vivim_hip_ext.h"
#include "../../include/vivim_hip_ext_head.h"
#include "../../include/vivim_hip_ext_binary_metrics.h"

namespace vivim {

// ---- causal conv1d: conv1d.hip, which hands channel-last tensors to conv1d_cl.hip
// causal_conv1d.cpp:151: is_channel_last = x.stride(1) == 1 && x.stride(2) > 1
inline bool conv_channel_last(const vivim_conv_fwd_params& f) { return f.x_c_stride == 1 && f.x_l_stride > 1; }
bool conv_fwd_dispatch(const vivim_conv_fwd_params&, hipStream_t);
bool conv_bwd_dispatch(const vivim_conv_bwd_params&, hipStream_t);
size_t conv_bwd_det_workspace_bytes(const vivim_conv_fwd_params&);
Launch conv_bwd_det_dispatch(const vivim_conv_bwd_params&, void* ws, size_t bytes, hipStream_t);
bool conv_cl_fwd_dispatch(const vivim_conv_fwd_params&, hipStream_t);                        // conv1d_cl.hip
bool conv_cl_bwd_dispatch(const vivim_conv_bwd_params&, hipStream_t);
size_t conv_cl_bwd_det_slots(const vivim_conv_fwd_params&);
bool conv_cl_bwd_det_launch(const vivim_conv_bwd_params&, hipStream_t);       // dweight: the slots

// ---- selective scan: scan_plan.hip
bool ssm_fwd_dispatch(const vivim_ssm_fwd_params&, hipStream_t);
bool ssm_fwd_lean_dispatch(const vivim_ssm_fwd_params&, void* last_state, hipStream_t);
bool ssm_bwd_dispatch(const vivim_ssm_bwd_params&, hipStream_t);
Launch ssm_bwd_det_dispatch(const vivim_ssm_bwd_params&, void* det_ws, size_t det_ws_bytes, hipStream_t);
int scan_chunk_len(int itype);
int scan_ckpt_len(const vivim_ssm_fwd_params&);
size_t scan_fwd_workspace_bytes(const vivim_ssm_fwd_params&);
size_t scan_bwd_workspace_bytes(const vivim_ssm_fwd_params&);
size_t scan_bwd_det_workspace_bytes(const vivim_ssm_fwd_params&);
size_t scan_bwd_det_call_workspace_bytes(const vivim_ssm_bwd_params&);

// ---- decode step: update.hip
void conv_update_launch(const vivim_conv_update_params&, hipStream_t);
void state_update_launch(const vivim_state_update_params&, hipStream_t);

// ---- depthwise conv: dwconv.hip
bool dwconv_fwd_dispatch(const vivim_dwconv_params&, hipStream_t);
bool dwconv_wgrad_dispatch(const vivim_dwconv_wgrad_params&, hipStream_t);
size_t dwconv_wgrad_det_workspace_bytes(const vivim_dwconv_wgrad_params&);
Launch dwconv_wgrad_det_dispatch(const vivim_dwconv_wgrad_params&, void* ws, size_t bytes, hipStream_t);

// ---- direction scatter / gather: dirmap.hip
template <bool GATHER> bool dir_dispatch(const vivim_dir_params&, hipStream_t);

// ---- channel-major LayerNorm, plain and with the residual add: layernorm.hip
bool layernorm_dispatch(const vivim_layernorm_params&, bool bwd, hipStream_t);
size_t layernorm_bwd_workspace_bytes(const vivim_layernorm_params&);
bool add_layernorm_dispatch(const vivim_add_layernorm_params&, bool bwd, hipStream_t);
size_t add_layernorm_bwd_workspace_bytes(const vivim_add_layernorm_params&);

// ---- token-major LayerNorm, plain and with the residual add: token_layernorm.hip
bool token_layernorm_dispatch(const vivim_token_layernorm_params&, bool bwd, hipStream_t);
bool token_layernorm_pair_ok(int itype, int otype);
size_t token_layernorm_bwd_workspace_bytes(const vivim_token_layernorm_params&);
bool token_add_norm_dispatch(const vivim_token_add_norm_params&, bool bwd, hipStream_t);
bool token_add_norm_pair_ok(int btype, int rtype);
size_t token_add_norm_bwd_workspace_bytes(const vivim_token_add_norm_params&);

// ---- split-K weight gradient: wgrad.hip
bool wgrad_nt_dispatch(const vivim_wgrad_nt_params&, hipStream_t);

// ---- segmentation loss, metrics and structure loss: seg_loss.hip, seg_metrics.hip, structure_loss.hip
bool seg_loss_dispatch(const vivim_seg_loss_params&, bool bwd, hipStream_t);
size_t seg_loss_workspace_bytes(const vivim_seg_loss_params&);
bool seg_metrics_dispatch(const vivim_seg_metrics_params&, hipStream_t);
size_t seg_metrics_workspace_bytes(const vivim_seg_metrics_params&);
bool structure_loss_dispatch(const vivim_structure_loss_params&, bool bwd, hipStream_t);
size_t structure_loss_workspace_bytes(const vivim_structure_loss_params&);
int64_t structure_loss_tiles(const vivim_structure_loss_params&);

// ---- bilinear upsampling and the fused decode head: upsample.hip, decode_head.hip
bool upsample_dispatch(const vivim_upsample_params&, bool bwd, hipStream_t);
int64_t upsample_blocks(const vivim_upsample_params&, bool bwd);
bool decode_head_dispatch(const vivim_decode_head_params&, hipStream_t);
int64_t decode_head_blocks(const vivim_decode_head_params&);
int decode_head_max_hidden();

// ---- the training head's upsample + dropout + concat: head_concat.hip
bool head_concat_dispatch(const vivim_head_concat_params&, bool bwd, hipStream_t);
int64_t head_concat_blocks(const vivim_head_concat_params&, bool bwd);

// ---- validation metrics of the binary recipe: binary_metrics.hip
bool binary_metrics_dispatch(const vivim_binary_metrics_params&, hipStream_t);
size_t binary_metrics_workspace_bytes(const vivim_binary_metrics_params&);

// ---- fused clip + AdamW step, plain and with fp32 masters: optimizer.hip
void opt_grad_stats_launch(const vivim_opt_step_params&, hipStream_t);
void opt_finalise_launch(const vivim_opt_step_params&, hipStream_t);
void opt_adamw_launch(const vivim_opt_step_params&, hipStream_t);
void opt_grad_stats_mw_launch(const vivim_opt_step_params&, int dtype, hipStream_t);
void opt_adamw_mw_launch(const vivim_opt_step_params&, const void* masters, int dtype, hipStream_t);

}  // namespace vivim
