/* vivim_hip_ext.h -- entry points of libvivim_hip.so added after ABI version 8.
 *
 * The first extension header, hence no feature in its name: it holds the structure loss.
 * include/vivim_hip.h is frozen at ABI version 8: its structs, its functions, vivim_sizeof and
 * vivim_abi_version() stay as they are.  A feature added after version 8 gets a header of its own, include/vivim_hip_ext_<feature>.h,
 * a row in EXTENSIONS of vivim_amd/_lib.py, and a params struct that opens with `struct_bytes`: the caller sets it to sizeof of the
 * struct as it compiled it, the entry points refuse any other value, and there is no vivim_sizeof row.  Every such header is
 * exported from the same library, parsed by the same parser (parse_header) and bound by the same loop (lib()), so it is written in
 * the same restricted C: fixed-width fields, explicit padding, one `typedef struct { ... } vivim_*;` per params struct, plain
 * function declarations.
 *
 * The conventions of vivim_hip.h hold: every call returns VIVIM_OK or an error code with a message in vivim_last_error(),
 * checks its arguments on the host before any launch, and enqueues on `stream` (a hipStream_t) without synchronising. */
#ifndef VIVIM_HIP_EXT_H
#define VIVIM_HIP_EXT_H

#include "vivim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- structure loss: boundary-weighted BCE + weighted IoU (csrc/structure_loss.hip; vivim_amd/structure_loss.py) ----
 * For channel c the mask is m = (target == c + first_class); a label that matches no channel is a pixel of no class.
 *   k   = number of mask pixels in the 31 x 31 window centred on the pixel, clipped to the image (an integer <= 961)
 *   w   = 1 + 5 * |k / 961 - m|                       (avg_pool2d(kernel 31, stride 1, padding 15, count_include_pad))
 *   bce = max(x, 0) - x * m + log1p(exp(-|x|)),  s = sigmoid(x)
 *   per (image, channel):  S_w = sum w,  S_b = sum w * bce,  S_i = sum w * s * m,  S_d = sum w * (m ? 1 : s)
 *   loss = mean over (image, channel) of  S_b / S_w + 1 - (S_i + eps) / (S_d + eps)
 * Forward: one kernel of partial sums per (image, tile) stored into workspace slots, one finalise kernel that adds the slots in
 * slot order in fp64 and writes `loss` (one fp32) and, unless `coef` is NULL, the (batch, classes, 3) fp32 factors
 * 1 / S_w, 1 / (S_d + eps), (S_i + eps) / (S_d + eps)^2.  Backward: one kernel that recomputes k, w and s, reads `coef` and the
 * upstream gradient *grad_out (one fp32 on the device), multiplies in fp32 and rounds dlogits once.  No atomics: both
 * directions are bit-repeatable.  The pixels of a logits plane are contiguous (row stride = width); batch and channel
 * strides are free.  Strides are in elements. */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_structure_loss_params) as the caller compiled it */
    int32_t batch, classes, height, width;           /* classes: 1 to 8 */
    int32_t itype;                                   /* vivim_dtype_t of logits and dlogits */
    int32_t ttype;                                   /* target: 0 = int64, 1 = uint8 */
    int32_t first_class;                             /* the label of channel 0: 0 for the multiclass form, 1 for the binary one */
    float eps;                                       /* 1e-6 for the multiclass form, 1 for the binary one */
    int32_t _pad0;
    int64_t logits_batch_stride, logits_c_stride;
    int64_t dlogits_batch_stride, dlogits_c_stride;
    int64_t target_batch_stride;
    const void *logits;                              /* (batch, classes, height, width) */
    const void *target;                              /* (batch, height, width), rows contiguous */
    void *loss;                                      /* forward: one fp32 */
    void *coef;                                      /* forward writes (NULL: not wanted), backward reads: (batch, classes, 3) fp32 */
    void *workspace;                                 /* forward scratch, vivim_structure_loss_workspace_bytes() of it, 8-byte aligned */
    int64_t workspace_bytes;
    const void *grad_out;                            /* backward: the upstream gradient, one fp32 on the device */
    void *dlogits;                                   /* backward: (batch, classes, height, width), pixels contiguous */
} vivim_structure_loss_params;

size_t vivim_structure_loss_workspace_bytes(const vivim_structure_loss_params *p);   /* from the sizes and itype; 0 on bad sizes */
int vivim_structure_loss_fwd(const vivim_structure_loss_params *p, void *stream);
int vivim_structure_loss_bwd(const vivim_structure_loss_params *p, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VIVIM_HIP_EXT_H */
