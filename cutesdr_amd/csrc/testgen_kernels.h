// testgen_kernels.h -- launch interface of the batch signal generator's kernel (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "testgen_host.hpp"

namespace csdr {

struct TestGenArgs {
    float *out; long stride;             // [channels][stride] complex fp32 pairs or fp32 mono, stride in samples
    const tg::ChanParam *par;            // [channels], device memory
    unsigned n;                          // samples of the call (every launch of the call spans all of them)
    int channels;
};
hipError_t testgen_launch(const TestGenArgs &a, int real, hipStream_t s);

}  // namespace csdr
