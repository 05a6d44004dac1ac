// api_internal.hpp -- what the files that implement include/hbrbc.h share
// (api.hip, api_pairing.hip).  Internal to libhbrbc.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/hbrbc.h"

namespace hbrbc {

// Records the message hbrbc_last_error() returns (thread-local, api.hip) and
// returns `code`.
int fail(int code, const char *fmt, ...);

// HBRBC_E_NO_DEVICE (through fail) unless a HIP device is visible.
int have_device();

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace hbrbc

#define HB_HIP(call)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return hbrbc::fail(HBRBC_E_DEVICE, "%s failed: %s (%s:%d)", #call,                  \
                               hipGetErrorString(e_), __FILE__, __LINE__);                      \
    } while (0)
