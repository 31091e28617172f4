/* vivim_hip_ext_binary_metrics.h -- validation metrics of the binary (one-channel) recipe on the device: the threshold sweep
 * (dice, jaccard, precision, recall, F, specificity over 256 thresholds), S-measure, mean E-measure and MAE of a batch of
 * probability maps against their masks (csrc/binary_metrics.hip; vivim_amd/binary_metrics.py, whose docstring is the definition).
 *
 * An extension header.  include/vivim_hip.h is frozen at ABI version 8: its structs, its functions, vivim_sizeof and
 * vivim_abi_version() stay as they are.  A feature added after version 8 gets a header of its own, include/vivim_hip_ext_<feature>.h,
 * a row in EXTENSIONS of vivim_amd/_lib.py, and a params struct that opens with `struct_bytes`: the caller sets it to sizeof of the
 * struct as it compiled it, the entry points refuse any other value, and there is no vivim_sizeof row.  Every such header is
 * exported from the same library, parsed by the same parser (parse_header) and bound by the same loop (lib()), so it is written in
 * the same restricted C: fixed-width fields, explicit padding, one `typedef struct { ... } vivim_*;` per params struct, plain
 * function declarations.
 *
 * The conventions of vivim_hip.h hold: every call returns VIVIM_OK or an error code with a message in vivim_last_error(),
 * checks its arguments on the host before any launch, and enqueues on `stream` (a hipStream_t) without synchronising. */
#ifndef VIVIM_HIP_EXT_BINARY_METRICS_H
#define VIVIM_HIP_EXT_BINARY_METRICS_H

#include "vivim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `batch` images of height x width pixels, rows contiguous (pixel (r, c) of image n at pred + n * pred_batch_stride + r * width + c,
 * the mask likewise); strides in elements.  Per image nine fp64 values are written to values[n][0..9): Dice, Jaccard, Precision,
 * Recall, Fmeasure, specificity (each the mean over the 256 thresholds), Smeasure, Emeasure, MAE.
 *   thresholds  256 fp32 on the device: float32(linspace(1, 0, 256)), descending; the kernels compare with them, they do not
 *               recompute them
 *   hist        NULL, or int32 (batch, 4, 256): the sweep's histogram over the mask and over its complement (bin i counts the
 *               pixels that exceed exactly i + 1 thresholds), then the E-measure's two (bin = uint8(pn * 255))
 *   state       NULL, or 10 fp64: state[k] += values[n][k] for n = 0 .. batch-1 in that order, state[9] += batch
 * Five launches, no float atomics, no synchronisation, nothing copied to the host; equal inputs give equal bits. */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_binary_metrics_params) as the caller compiled it */
    int32_t batch, height, width;                    /* height * width >= 2 */
    int32_t ptype;                                   /* vivim_dtype_t of pred */
    int32_t gtype;                                   /* of gt: a vivim_dtype_t (g = gt > 0.5), or 3 = uint8 / bool (g = gt != 0) */
    int64_t pred_batch_stride, gt_batch_stride;      /* >= height * width */
    const void *pred, *gt, *thresholds;
    void *values;                                    /* fp64 (batch, 9), 8-byte aligned */
    void *hist;
    void *state;                                     /* 8-byte aligned */
    void *workspace;                                 /* 8-byte aligned, vivim_binary_metrics_workspace_bytes() bytes */
    int64_t workspace_bytes;
} vivim_binary_metrics_params;

size_t vivim_binary_metrics_workspace_bytes(const vivim_binary_metrics_params *p);    /* 0: the params are refused */
int vivim_binary_metrics(const vivim_binary_metrics_params *p, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VIVIM_HIP_EXT_BINARY_METRICS_H */
