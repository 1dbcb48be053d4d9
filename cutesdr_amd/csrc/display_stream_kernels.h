// display_stream_kernels.h -- launch interface of the display stream's frame gather and carry (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "wire_format.hpp"
#include "frontend_kernels.h"
#include "display_plan.hpp"

namespace csdr {

// The display stream of one call, per channel: sample s >= 0 is sample s of the call's row (complex fp32 `in`, or the
// datagrams of `wire` when wire.pk is set) minus the channel's DC offset (dc: optional [channels][2] doubles, the
// arithmetic of unpack_kernel: (float)((double)v - dc)); sample s in [-pos, 0) is carry[ch][pos + s], the partial frame
// the previous calls left (already corrected, as m_DataBuf is).
// Behind a blanked chain call (nb_mask set: the mask, state and history half that call's mask pass left, DcBlank in
// downconv_kernels.h) sample s >= 0, before the DC correction, is what the reference's in-place blanker hands over
// (interface/sdrinterface.cpp:884) -- the down-converter's rule, downconv_kernels.h:44-51, indexed by row = channel:
//     nb_state[ch].on ? (mask bit s set ? (0, 0) : raw[s - delay_n - 1]) : raw[s]     raw[j < 0] = nb_hist[ch][NB_HIST + j]
// so a blanked sample becomes -dc (:891-894), and the carry holds blanked, corrected samples.
struct StreamSrc {
    const float *in; long in_stride;    // [channels][in_stride] complex fp32; unused when wire.pk is set
    WireIn wire;
    const double *dc;
    const float *carry; int pos;        // [channels][carry_stride] complex fp32, the first pos samples valid
    long carry_stride;
    int channels;
    const unsigned *nb_mask; long nb_mask_stride;   // [channels][stride] words, bit s & 31 of word s >> 5; nullptr: no blanker
    const NbChan *nb_state;                         // [channels]: on, delay_n
    const float *nb_hist;                           // [channels][NB_HIST] complex: the inputs before the call
};

// out[ch][k * N + i] = stream sample start + k * step + i, for k < count, i < N
hipError_t display_gather_launch(const StreamSrc &a, long long start, long long step, int count, int N, float *out,
                                 hipStream_t stream);
// the row form: out[row][k * N + i] (rows max_count * N apart) = stream sample start + k * step + i of the row, for the
// nrows entries {row, count, start, step} of the device table d_rows; max_count is the largest count among them
hipError_t display_gather_rows_launch(const StreamSrc &a, const SpecRow *d_rows, int nrows, int max_count, int N, float *out,
                                      hipStream_t stream);
// carry[ch][dst + i] = stream sample src + i, i < len (src >= 0: never reads the carry it writes)
hipError_t display_carry_launch(const StreamSrc &a, float *carry, int dst, long long src, int len, hipStream_t stream);

}  // namespace csdr
