// fastfir_design_kernels.h -- launch interface of the device-side CFastFIR::SetupParameters (internal).
#pragma once
#include <hip/hip_runtime.h>

namespace csdr {

struct DesignJob {
    int slot;             // filter row of the object
    int pad;
    double nfc, nfs;      // half width and 2 pi centre of the pass band, normalised (host_math.hpp: fastfir_design_job)
};

struct DesignArgs {
    const DesignJob *jobs;      // pinned, device mapped: one per workgroup
    const double *win;          // fastfir_window(N/2+1)
    const double *tw;           // design_twiddles(N): [2j] = cos, [2j+1] = sin of 2 pi j / N, j < N/2, nearest doubles
    const int *perm, *perm2;    // device slot -> natural bin, generic / pipelined overlap-save kernel
    float *h, *h2;              // [filters][N] complex fp32 in those two orders
    const int *permg;           // gain slot -> natural bin (fastfir2_gain_bin_of)
    float *gain;                // [filters][N] fp32 real gains Re(H[k] (-j)^k) in that order (host_math.hpp: fastfir_gain)
    double *resp;               // [filters][N] complex fp64, natural order (N = 16384: also the transform's work row)
};

hipError_t fastfir_design_launch(int log2n, const DesignArgs &a, int njobs, hipStream_t stream);

}  // namespace csdr
