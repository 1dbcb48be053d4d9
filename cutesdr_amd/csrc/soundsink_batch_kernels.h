// soundsink_batch_kernels.h -- launch interface of the batch sound sink's resampling kernel (internal).
#pragma once
#include <hip/hip_runtime.h>

namespace csdr {

// one receiver's parameters of one put, built by the host under that receiver's lock
struct SinkBatchParam {
    double rate;                         // m_OutRatio * (1 + m_RateCorrection)
    float gain;                          // volume gain
    int n;                               // input samples of the row this put (0: the row is left alone)
};

struct SinkBatchArgs {
    const float *in; long in_stride;     // [channels][in_stride] fp32 (mono) or complex fp32 pairs (stereo), stride in floats
    float *hist;                         // [channels][RS_PERIODS * w]: the last 28 inputs of each row, updated in place
    double *t;                           // [channels] m_FloatTime of each receiver
    const float *sinc;                   // [RS_LEN]
    const SinkBatchParam *par;           // [channels]
    short *out; long out_stride;         // [channels][out_stride] int16 (L/R pairs when stereo), out_stride in shorts
    int *count;                          // [channels] resampled samples of each row
    int out_cap;                         // samples per output row
    int channels;
};
hipError_t soundsink_batch_launch(const SinkBatchArgs &a, int stereo, hipStream_t s);

}  // namespace csdr
