// so100_host.hpp -- the host layer under both C ABIs of libso100sim.so (so100_sim.hip: include/so100_sim.h, so100_learn.hip:
// include/so100_learn.h): the message behind so100_last_error(), fail(), HIP_TRY, the device guard and the obs_dim launch switch.
// Host only: included by the two ABI files after their kernels, by nothing a kernel sees.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace so100 {

inline thread_local char g_last_error[512] = "";       // one slot per thread for the whole library: so100_last_error() returns it

// every failing ABI call leaves through here: formats the message, returns `code`
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
    return code;
}

// HIP_TRY(expr, code): "<hip error string> (HIP error <n>)";  HIP_TRY(expr, code, "so100_fn: "): the same behind that prefix
#define HIP_TRY(expr, code, ...) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return so100::fail(code, __VA_ARGS__ "%s (HIP error %ld)", hipGetErrorString(e_), (long)e_); } while (0)

// makes `dev` current for the scope of an ABI call and puts the caller's device back
struct DeviceGuard {
    int prev = -1, target = -1; bool ok = true;
    explicit DeviceGuard(int dev) : target(dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() { if (ok && prev != target) (void)hipSetDevice(prev); }
};

// first statements of an ABI call `fn` that touches the device
#define SO100_ON_DEVICE(dev, fn) so100::DeviceGuard g(dev); if (!g.ok) return so100::fail(SO100_E_NODEVICE, "%s: cannot select the device", fn)

// the kernels are templates on the observation width: runs `...` with a constexpr int OD = 15 or 8 in scope
#define SO100_WITH_OBS_DIM(od, ...) do { if ((od) == 15) { constexpr int OD = 15; __VA_ARGS__ } else { constexpr int OD = 8; __VA_ARGS__ } } while (0)

}  // namespace so100
