// Host plumbing shared by every host-side unit of libnrsc5hip: the calling thread's last-error text, FAIL / HIPCHK, the device guard.
#pragma once
#include <hip/hip_runtime.h>
#include "nrsc5hip.h"

namespace nrsc5 {
// The text behind nrsc5hip_last_error(): one thread-local buffer for the whole library, owned by engine.hip.
void set_last_error(const char *msg);
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   // sets the text, returns `code`

// Switches to a device for the scope of an entry point and restores the calling thread's current device on exit.
struct DeviceGuard {
    int prev = -1, want = -1;
    explicit DeviceGuard(int dev) : want(dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != want) (void)hipSetDevice(want); }
    ~DeviceGuard() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
};
struct DevTmp { void *p = nullptr; ~DevTmp() { if (p) (void)hipFree(p); } };      // a device allocation freed on every return path
}

#define FAIL(code, ...) return nrsc5::fail((code), __VA_ARGS__)
#define HIPCHK(expr)                                                                                                         \
    do {                                                                                                                     \
        hipError_t _e = (expr);                                                                                              \
        if (_e != hipSuccess) FAIL(NRSC5HIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
// for a constructor function: on failure run `cleanup` (free the half-built object), then fail
#define HIPCHK_OR(expr, cleanup)                                                                                             \
    do {                                                                                                                     \
        hipError_t _e = (expr);                                                                                              \
        if (_e != hipSuccess) { cleanup; FAIL(NRSC5HIP_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e)); }               \
    } while (0)
