// host_util.h -- host-side helpers shared by the launchers: one-time kernel setup and device facts, keyed by the CURRENT
// device (a process that drives several GPUs must set a kernel's dynamic-LDS limit on each of them, and plans its launches
// for the CU count of the device it launches on).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

// Developer A/B switches (forcing a fallback path, planner constants, tile shapes): honoured only under SSC_DEV_SWITCHES=1.
// They select paths the test suite does not cover in combination -- lab tools (scripts/), not supported configurations;
// DESIGN.md section 7 lists the supported switches.
static inline const char* ssc_dev_getenv(const char* name) {
    static const bool on = [] { const char* e = getenv("SSC_DEV_SWITCHES"); return e != nullptr && e[0] == '1'; }();
    return on ? getenv(name) : nullptr;
}
// A developer switch as a number: the variable through atoi / atof when it is unlocked and set, `dflt` otherwise.  Switches
// are 0 / 1 or a number; anything else reads as atoi / atof read it (an empty or non-numeric value is 0).  Call sites keep the
// value in a function-local `static const`: read once per process, initialised thread-safely.
static inline int ssc_dev_int(const char* name, int dflt) {
    const char* e = ssc_dev_getenv(name);
    return e != nullptr ? atoi(e) : dflt;
}
static inline double ssc_dev_double(const char* name, double dflt) {
    const char* e = ssc_dev_getenv(name);
    return e != nullptr ? atof(e) : dflt;
}
// SSC_ARITH=fp32 (a supported configuration, not a developer switch): every contraction on the exact-fp32 MFMA kernels
static inline bool ssc_arith_fp32() {
    static const bool fp32 = [] { const char* e = getenv("SSC_ARITH"); return e != nullptr && (e[0] == 'f' || e[0] == 'F'); }();
    return fp32;
}

// true the first time this call site (its own `done` mask) runs on the current device
static inline bool ssc_first_on_device(unsigned long long* done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (*done & bit) return false;
    *done |= bit;
    return true;
}

// hipFuncAttributeMaxDynamicSharedMemorySize once per device; the error code of the call that made it (0 afterwards)
static inline int ssc_set_max_lds(const void* fn, int bytes, unsigned long long* done) {
    if (!ssc_first_on_device(done)) return 0;
    return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// What the launcher of a streaming forward kernel (fewchan / pw1x1 / c3x3 / s2n16 / tr4tiny / fewchan7 / tr4n16 .hip) decides for a
// descriptor its predicate admits: the launch reads it and ssc_conv_stream_plan reports it, so there is one copy of each choice.
struct ssc_stream_plan {
    int inst;               // instantiation index within the kernel (include/sketchycolor_hip.h at ssc_conv_stream_plan)
    int tiles;              // tiles of the launch (tr4tiny: blocks; tr4n16: over the four phases; pw1x1: over the column groups)
    int tiles_x, tiles_y;   // tiles across and down one image
    int grid_x, grid_y;     // the grid: grid_x * grid_y workgroups
};

// compute units of the current device
static inline int ssc_num_cu() {
    static int n[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    int& v = n[dev & 63];
    if (v == 0) {
        hipDeviceProp_t prop;
        v = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return v;
}
