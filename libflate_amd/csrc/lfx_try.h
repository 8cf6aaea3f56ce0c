// lfx_try.h — the two early-return macros of the host sources: a HIP call, or a kernel launcher (they return hipError_t as int),
// that fails leaves its text on the context `c` in scope and returns LFX_E_DEVICE.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lfx.h"

#define HIP_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            c->set_error(std::string(#expr) + ": " + hipGetErrorString(e_));          \
            return LFX_E_DEVICE;                                                      \
        }                                                                             \
    } while (0)
#define LAUNCH_TRY(call)                                                              \
    do {                                                                              \
        int e_ = (call);                                                              \
        if (e_) {                                                                     \
            c->set_error(std::string(#call) + ": " + hipGetErrorString((hipError_t)e_)); \
            return LFX_E_DEVICE;                                                      \
        }                                                                             \
    } while (0)
