// capi.hip -- what the extern "C" boundary of libvivim_hip.so has that is no feature's: the last-error text, the tuning
// values, the ABI version and the struct sizes.  Every other entry point stands with its argument checks at the end of the
// file that defines its kernels (capi.cuh).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "capi.cuh"

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
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
size_t vivim_sizeof(int which) {
    static const size_t sizes[] = {
        sizeof(vivim_ssm_fwd_params), sizeof(vivim_ssm_bwd_params), sizeof(vivim_conv_fwd_params), sizeof(vivim_conv_bwd_params),
        sizeof(vivim_dwconv_params), sizeof(vivim_dwconv_wgrad_params), sizeof(vivim_dir_params), sizeof(vivim_conv_update_params),
        sizeof(vivim_state_update_params), sizeof(vivim_layernorm_params), sizeof(vivim_wgrad_nt_params),
        sizeof(vivim_add_layernorm_params), sizeof(vivim_seg_loss_params), sizeof(vivim_seg_metrics_params),
        sizeof(vivim_upsample_params)};
    return which >= 0 && which < (int)(sizeof(sizes) / sizeof(sizes[0])) ? sizes[which] : 0;
}

}  // extern "C"
