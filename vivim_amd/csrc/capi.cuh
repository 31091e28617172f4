// capi.cuh -- what the extern "C" entry points of every kernel file share: the last-error text, the refusal helpers and the
// interface headers (include/vivim_hip.h, frozen at ABI version 8, and one include/vivim_hip_ext_<feature>.h per feature
// added since).  Nothing here belongs to one feature.
//
// An entry point stands at the end of the file that defines its kernels.  It refuses arguments before anything is
// launched, then calls the file's own *_dispatch: that returns false where no kernel is built for the call's types (the
// checks have refused those, so this is a second line), a *_det_dispatch a Launch (det.cuh).
#pragma once
#include <float.h>
#include <stddef.h>
#include "det.cuh"
#include "../../include/vivim_hip_ext.h"
#include "../../include/vivim_hip_ext_head.h"
#include "../../include/vivim_hip_ext_binary_metrics.h"

using vivim::Launch;
using vivim::elem_bytes;
using vivim::vec_elems;

// Writes the text that vivim_last_error() returns and hands `code` back.  Defined once, in capi.hip, beside the one
// thread-local buffer: a copy per file would leave vivim_last_error() empty for every feature but one.
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);

#define VCHECK(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) return fail(VIVIM_ERR_INVALID, "%s: check failed: %s", __func__, #cond); \
    } while (0)

inline int after_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VIVIM_ERR_LAUNCH, "%s: launch failed: %s", what, hipGetErrorString(e));
    return VIVIM_OK;
}

inline bool dtype_ok(int t) { return t == VIVIM_F32 || t == VIVIM_F16 || t == VIVIM_BF16; }
inline bool aligned(const void* q, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }
inline bool aligned16(const void* q) { return aligned(q, 16); }
inline hipStream_t as_stream(void* stream) { return static_cast<hipStream_t>(stream); }

// the refusal of a missing, short or misaligned workspace: `fn` is the entry point, `query` the call that sizes it
inline int bad_workspace(const char* fn, const char* query, long long bytes, const void* at, int align, size_t need) {
    return fail(VIVIM_ERR_INVALID, "%s: workspace of %lld bytes at %p: need a %d-byte aligned one of %s() = %zu", fn, bytes, at, align,
                query, need);
}
// the same for a workspace that the params struct carries, with its own alignment; VIVIM_OK: it will do
inline int check_workspace(const char* fn, const char* query, const void* ws, int64_t bytes, int align, size_t need) {
    if (ws == nullptr || !aligned(ws, align) || bytes < 0 || (size_t)bytes < need) return bad_workspace(fn, query, bytes, ws, align, need);
    return VIVIM_OK;
}
// a params struct of another library version; `name` is the struct's
inline int check_struct_bytes(const char* fn, const char* name, int32_t struct_bytes, size_t size) {
    if (struct_bytes != (int32_t)size)
        return fail(VIVIM_ERR_INVALID, "%s: struct_bytes = %d, this library's %s has %zu", fn, struct_bytes, name, size);
    return VIVIM_OK;
}

// The return code of entry `fn` from what its *_dispatch reported: `unsupported` and its arguments word the refusal of
// types that no kernel is built for.
template <typename... Args> inline int after_dispatch(bool launched, const char* fn, const char* unsupported, Args... args) {
    return launched ? after_launch(fn) : fail(VIVIM_ERR_UNSUPPORTED, unsupported, args...);
}
// The same for a deterministic entry and its *_det_dispatch: `query` sizes the slot workspace and answered `need` for this call.
template <typename... Args>
inline int after_det_dispatch(Launch launched, const char* fn, const char* query, const void* ws, size_t bytes, size_t need,
                              const char* unsupported, Args... args) {
    switch (launched) {
        case Launch::ok: break;
        case Launch::bad_workspace: return bad_workspace(fn, query, bytes, ws, 16, need);
        case Launch::unsupported: return fail(VIVIM_ERR_UNSUPPORTED, unsupported, args...);
    }
    return after_launch(fn);
}
