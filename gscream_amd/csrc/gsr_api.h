// gsr_api.h -- what an extern "C" entry point needs to report a failure (host code only).
//
// Every module defines its own entry points of include/gsraster.h at the end of its .hip file, beside the kernels whose index
// arithmetic their checks guard.  A failure is an int code + a message in the one thread-local buffer behind gsr_last_error():
// gsr_fail and the buffer are defined once, in api.hip, and stay inside the library.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gsraster.h"
#include "../../include/gsraster_jpeg_decode.h"

__attribute__((visibility("hidden"), format(printf, 2, 3))) int gsr_fail(int code, const char* fmt, ...);

#define GSR_HIP(expr, what)                                                                                     \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return gsr_fail(GSR_ERR_HIP, "%s: %s (%s)", what, hipGetErrorString(e_), #expr); \
    } while (0)
