// tests/cpu/hip_lanes/psxhip_api_standin.h -- TEST INFRASTRUCTURE: stand-ins of a few lines for the functions of psxhip_api.cpp that
// the reader modules' host files and kernel files call (the error text, the device's presence), so that a lane program can include
// those files without the rest of the library.  The CPU "device" of hip_lanes_device.h is device 0 and the only one.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include "../../../include/psxav_hip.h"

namespace hip_lanes {
inline char last_error[1024] = "";
}

extern "C" void psxhip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(hip_lanes::last_error, sizeof hip_lanes::last_error, fmt, ap);
    va_end(ap);
}
extern "C" const char* psxhip_last_error(void) { return hip_lanes::last_error; }
extern "C" int psxhip_device_count(void) { return 1; }
int psxhip_ensure_device(int device) {
    if (device == 0) return PSXHIP_OK;
    psxhip_set_error("stand-in: device %d does not exist", device);
    return PSXHIP_EDEVICE;
}
