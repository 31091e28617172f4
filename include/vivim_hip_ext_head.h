/* vivim_hip_ext_head.h -- the training decode head's entry points of libvivim_hip.so: upsample + dropout + concat in one launch.
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
#ifndef VIVIM_HIP_EXT_HEAD_H
#define VIVIM_HIP_EXT_HEAD_H

#include "vivim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- head concat: bilinear upsampling, per-element dropout and channel concat (csrc/head_concat.hip; vivim_amd/head_concat.py) ----
 * n_maps maps (batch, map_c[s], map_h[s], map_w[s]) in dense channels-last memory (pixel stride map_c[s]) become one tensor whose
 * pixel (n, oh, ow) lies at out + n * out_batch_stride + (oh * out_w + ow) * out_pixel_stride and holds map s in the channels
 * [chan_off[s], chan_off[s] + map_c[s]).  Per element, in fp32:
 *   v = th.l0 * (tw.l0 * a + tw.l1 * b) + th.l1 * (tw.l0 * d + tw.l1 * e)      the taps of vivim_upsample_bilinear2d_fwd
 *   y = round(keep ? v * scale[s] : 0)                                         keep[s] == NULL: every element is kept
 * and a map of the output's own size is y = round(keep ? x * scale[s] : 0) without tap arithmetic.  keep[s] is (batch, out_h,
 * out_w, map_c[s]) uint8, dense per image, nonzero = keep.  Channels of a pixel that no map covers are not written.
 * Backward: the transpose in gather form.  A dmaps[s] element adds weight * (keep ? dout * scale[s] : 0) over the outputs that
 * tap it, in ascending order, in fp32, and is rounded once: no atomics, no workspace, equal inputs give equal bits.  dout has
 * the layout of out (out_batch_stride, out_pixel_stride), dmaps[s] that of maps[s] with dmap_batch_stride[s].
 * Strides are in elements (keep: in bytes).  One launch per direction, whatever n_maps is. */
typedef struct {
    int32_t struct_bytes;                            /* sizeof(vivim_head_concat_params) as the caller compiled it */
    int32_t batch, n_maps, out_h, out_w;             /* n_maps: 1 to 4 */
    int32_t itype;                                   /* vivim_dtype_t of the maps, out, dout and dmaps */
    int32_t map_c[4], map_h[4], map_w[4];            /* map_h[s] <= out_h, map_w[s] <= out_w */
    int32_t chan_off[4];                             /* first channel of map s inside a pixel of out */
    float scale[4];                                  /* 1 / (1 - p) of map s as fp32; 1 without dropout */
    int64_t map_batch_stride[4], dmap_batch_stride[4], keep_batch_stride[4];
    int64_t out_batch_stride, out_pixel_stride;      /* out_pixel_stride >= every chan_off[s] + map_c[s] */
    const void *maps[4], *keep[4];                   /* keep[s] NULL: no mask for map s */
    void *out;                                       /* forward */
    const void *dout;                                /* backward */
    void *dmaps[4];                                  /* backward */
} vivim_head_concat_params;

int vivim_head_concat_fwd(const vivim_head_concat_params *p, void *stream);
int vivim_head_concat_bwd(const vivim_head_concat_params *p, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VIVIM_HIP_EXT_HEAD_H */
