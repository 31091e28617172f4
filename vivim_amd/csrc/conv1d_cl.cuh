// conv1d_cl.cuh -- what conv1d_cl.hip defines and conv1d.hip calls: the causal conv1d on channel-last tensors.  These are
// the only functions of the library that cross from one kernel file to another (the scan's family launches excepted:
// scan_plan.cuh); every other *_dispatch, *_launch and *_workspace_bytes is static in the file of its kernels.
#pragma once
#include "common.cuh"

namespace vivim {

bool conv_cl_fwd_dispatch(const vivim_conv_fwd_params&, hipStream_t);
bool conv_cl_bwd_dispatch(const vivim_conv_bwd_params&, hipStream_t);
size_t conv_cl_bwd_det_slots(const vivim_conv_fwd_params&);
bool conv_cl_bwd_det_launch(const vivim_conv_bwd_params&, hipStream_t);       // dweight: the slots

}  // namespace vivim
