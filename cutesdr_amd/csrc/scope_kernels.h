// scope_kernels.h -- launch interface of the batch test-bench scope's kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "scope_host.hpp"

namespace csdr {

struct ScopeArgs {
    const float *rows; long long stride;     // [channels][stride] fp32 real or complex fp32 pairs, stride in samples; never written
    const sc::ChanParam *par;                // [channels], device memory
    sc::ChanState *state;                    // [channels]
    int *ring;                               // [channels][2][kMaxW]: m_TimeBuf1/2
    int *screen;                             // [channels][2][kMaxW]: m_TimeScrnBuf1/2
    int w, channels;
};
hipError_t scope_put_launch(const ScopeArgs &a, int cpx, hipStream_t s);

struct ScopeScreenArgs {
    const int *screen;                       // [channels][2][kMaxW]
    const sc::ChanParam *par;                // [channels]: vert (only read when y is set)
    int *out; long long out_stride;          // [channels][2][out_stride]
    int *y; long long y_stride;              // [channels][2][y_stride] or nullptr
    int w, h, channels;
};
hipError_t scope_screens_launch(const ScopeScreenArgs &a, hipStream_t s);

}  // namespace csdr
