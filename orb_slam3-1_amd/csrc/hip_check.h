// The library's one error path for HIP calls: orbx::fail records the message that orbx_last_error() returns (defined in
// orbx_extractor.hip) and ORBX_HIP returns ORBX_ERR_HIP from the enclosing function when a HIP call fails.  Host only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbslam3_hip.h"

namespace orbx {
int fail(int code, const char* fmt, ...);
}
using orbx::fail;

#define ORBX_HIP(expr)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(ORBX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
