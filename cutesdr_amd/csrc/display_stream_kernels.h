// display_stream_kernels.h -- launch interface of the display stream's frame gather and carry (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "wire_format.hpp"

namespace csdr {

// The display stream of one call, per channel: sample s >= 0 is sample s of the call's row (complex fp32 `in`, or the
// datagrams of `wire` when wire.pk is set) minus the channel's DC offset (dc: optional [channels][2] doubles, the
// arithmetic of unpack_kernel: (float)((double)v - dc)); sample s in [-pos, 0) is carry[ch][pos + s], the partial frame
// the previous calls left (already corrected, as m_DataBuf is).
struct StreamSrc {
    const float *in; long in_stride;    // [channels][in_stride] complex fp32; unused when wire.pk is set
    WireIn wire;
    const double *dc;
    const float *carry; int pos;        // [channels][carry_stride] complex fp32, the first pos samples valid
    long carry_stride;
    int channels;
};

// out[ch][k * N + i] = stream sample start + k * step + i, for k < count, i < N
hipError_t display_gather_launch(const StreamSrc &a, long long start, long long step, int count, int N, float *out,
                                 hipStream_t stream);
// carry[ch][dst + i] = stream sample src + i, i < len (src >= 0: never reads the carry it writes)
hipError_t display_carry_launch(const StreamSrc &a, float *carry, int dst, long long src, int len, hipStream_t stream);

}  // namespace csdr
