// sng_device_scope.h -- the one way the library selects a device (sng_env.h's translation units, sng_comm.cpp).
#pragma once
#include <hip/hip_runtime.h>

namespace sng {

// A handle's device for the length of a call, the caller's current device restored after it: no entry point
// leaves the caller on another device (sng_step is called per step without a device guard of the caller's own).
struct DeviceScope {
    int prev = -1, dev;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) err = hipSetDevice(d);
    }
    ~DeviceScope() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

}  // namespace sng
