// The library's one error path for HIP calls: orbx::fail records the message that orbx_last_error() returns (defined in
// orbx_extractor.hip) and ORBX_HIP returns ORBX_ERR_HIP from the enclosing function when a HIP call fails; ORBX_HIP_FIRST is for
// a sequence that cleanup follows: it keeps the first failure in r and skips the calls after it.  stage::check_device is the
// device check of every *_create.  Host only.
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

#define ORBX_HIP_FIRST(r, expr) do { if (!(r) && (expr) != hipSuccess) (r) = fail(ORBX_ERR_HIP, "%s failed", #expr); } while (0)

namespace stage {
// `device` names a HIP device of this process (the library has no CPU fallback: no device at all is an error of its own)
inline int check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ORBX_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(ORBX_ERR_ARG, "device %d out of range", device);
    return ORBX_OK;
}
}  // namespace stage
