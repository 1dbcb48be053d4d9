// spurcal_kernels.h -- launch interface of K13, the batch NCO-spur calibration (spurcal_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include "wire_format.hpp"
#include "frontend_kernels.h"
#include "spurcal_host.hpp"

namespace csdr {
namespace spur {

constexpr int kRun = 16;                 // samples a thread steps: divides both datagram sizes (240, 256)
constexpr int kThreads = 256;
constexpr int kPass = kRun * kThreads;   // samples a workgroup takes at a time
constexpr int kPasses = 4;
constexpr int kTile = kPass * kPasses;   // samples per workgroup: 16384

// The samples of one put, per receiver: n complex samples as fp32 rows (`in`) or as datagrams (wire.pk set), arriving
// as reference calls of call_len samples.  nb_mask set: behind a blanked chain call, the sample rule of
// display_stream_kernels.h:13-17 (mask, state and history half that call's mask pass left).
struct Src {
    const float *in; long in_stride;    // [channels][in_stride] complex fp32; unused when wire.pk is set
    WireIn wire;
    int n, call_len;
    const unsigned *nb_mask; long nb_mask_stride;
    const NbChan *nb_state;
    const float *nb_hist;
};

inline int spurcal_tiles(int n) { return (n + kTile - 1) / kTile; }

// One put of every receiver: dc [channels][2] and rec [channels] advanced by spurcal_put's rule over the samples of
// `src`; part is scratch of the object's, [channels][spurcal_tiles(n)][2] doubles.  Two launches; n > 0.
hipError_t spurcal_put_launch(const Src &src, int channels, double *dc, Rec *rec, double *part, hipStream_t stream);
// channels lo .. hi - 1: spurcal_command
hipError_t spurcal_command_launch(double *dc, Rec *rec, int lo, int hi, int cmd, double vi, double vq, hipStream_t stream);

}  // namespace spur
}  // namespace csdr
