// fft_batch_plain64_kernels.h -- launch interface of the fp64 batch transforms (fft_batch_plain64_kernels.hip, K3q)
#pragma once
#include <hip/hip_runtime.h>

namespace csdr {

// plain fp64 transforms of nframes frames of every row, 512 ... 65536 points: frame k of row c at
// in + 2 (c in_stride + k N) doubles, its transform at the same place of out; in == out with equal strides is in place
struct PlainBatch64Args {
    const double *in; long in_stride;   // complex fp64 [channels][in_stride]
    double *out;      long out_stride;
    int channels, nframes, sign;        // sign=+1 CFft::FwdFFT, -1 RevFFT
    const double *tw;                   // fft64_tables (fft_tw64_host.hpp): [N] W_N^m up to PLAIN64_MAX_LOG2N,
                                        // above it [256] W_256^m, then [256] W_N^m
    double *work; int group;            // the four-step sizes: the intermediate of `group` frames of every row,
};                                      // [channels][group][N] complex; longer calls go through it in groups
// the largest size that runs as one workgroup per frame; the sizes above it take the four-step form
constexpr int PLAIN64_MAX_LOG2N = 12;
hipError_t fft_batch_plain64_launch(int log2n, const PlainBatch64Args &a, hipStream_t stream);

}  // namespace csdr
