// The HIP-side helpers every .hip file of the library shares: the error-returning call wrapper and
// the current-device guard.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "crt_internal.h"

// a failing HIP call returns CRT_E_HIP from the enclosing function, the call's text in the message
#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return ::crt::fail(CRT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace crt {

// makes `d` the calling thread's device for a scope, then the one it found
struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int d) { (void)hipGetDevice(&prev); (void)hipSetDevice(d); }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

}  // namespace crt
