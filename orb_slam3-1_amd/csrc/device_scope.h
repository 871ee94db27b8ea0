// Agent-scope accesses of single words that one workgroup hands to another on a different XCD, whose L2 is not coherent with
// this one's: write-through stores / cache-bypassing loads of exactly these words instead of a device-wide fence
// (lba::update_errors_body says what that fence cost).  Device only.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void st_agent(double* p, double v)
{
    __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double* p)
{
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
