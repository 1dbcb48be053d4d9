// soundsink_batch_kernels.hip -- the batch sound sink's device half (K5b in DESIGN.md): CFractResampler::Resample
// (reference dsp/fractresampler.cpp:144-249, the int16 overloads) for every receiver of a batch in one launch, each row
// at its own rate, from its own time accumulator and 28-sample history.
//
// The output times are the reference's sequential fp64 accumulation (`while ((int)t < n) { emit t; t += rate; }
// t -= n`, :157-178), one chain per receiver: counts and table indices depend on them bit for bit, so no closed form.
// One workgroup per receiver: lane 0 walks the chain and fills a chunk of times in LDS, the workgroup interpolates
// the chunk behind a barrier (28 taps from the sinc table, the index in fp64, the sum in fp32, gain, clip, truncate --
// the arithmetic of resample_batch_kernel), and again until the row is used up.  No second launch, no global scratch.
#include <hip/hip_runtime.h>
#include "soundsink_batch_kernels.h"
#include "resampler_kernels.h"
#include "ref_constants.hpp"

namespace csdr {

constexpr int SB_THREADS = 256;
constexpr int SB_CHUNK = 1024;           // output times per LDS chunk (8 KiB)

template <int W>                         // 1: mono rows -> int16; 2: complex rows -> L/R int16 pairs
__global__ __launch_bounds__(SB_THREADS) void soundsink_batch_kernel(SinkBatchArgs a)
{
    __shared__ double ts[SB_CHUNK];
    __shared__ int s_m;
    const int ch = blockIdx.x, tid = threadIdx.x;
    const SinkBatchParam p = a.par[ch];
    if (p.n <= 0) {                      // nothing in, nothing out, no state touched
        if (tid == 0) a.count[ch] = 0;
        return;
    }
    const float *in = a.in + (long)ch * a.in_stride;
    float *hist = a.hist + (long)ch * RS_PERIODS * W;
    short *out = a.out + (long)ch * a.out_stride;
    double t = 0.0;
    if (tid == 0) t = a.t[ch];
    int total = 0;
    for (;;) {
        if (tid == 0) {                  // the serial chain: fractresampler.cpp:157-178
            int m = 0;
            while (m < SB_CHUNK && (int)t < p.n) { ts[m++] = t; t += p.rate; }
            s_m = m;
        }
        __syncthreads();
        const int m = s_m;
        for (int i = tid; i < m; i += SB_THREADS) {
            const double ti = ts[i];
            const int it = (int)ti;
            float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 4
            for (int k = 1; k <= RS_PERIODS; k++) {
                const int j = it + k;
                const float w = a.sinc[(int)(((double)j - ti) * (double)RS_PTS)];     // fractresampler.cpp:166
                const float *x = j < RS_PERIODS ? hist + W * j : in + W * (j - RS_PERIODS);
                acc0 += x[0] * w;
                if (W == 2) acc1 += x[1] * w;
            }
            const int o = total + i;
            if (o < a.out_cap) {         // the host's n / rate + 8 <= queue rule keeps every row inside its slot
                const float x = fminf(fmaxf(acc0 * p.gain, -refc::RS_MAX_SOUNDCARDVAL_F), refc::RS_MAX_SOUNDCARDVAL_F);
                if (W == 2) {
                    const float y = fminf(fmaxf(acc1 * p.gain, -refc::RS_MAX_SOUNDCARDVAL_F), refc::RS_MAX_SOUNDCARDVAL_F);
                    out[2 * o] = (short)x; out[2 * o + 1] = (short)y;
                } else {
                    out[o] = (short)x;
                }
            }
        }
        total += m;
        if (m < SB_CHUNK) break;
        __syncthreads();                 // every lane is done with this chunk before lane 0 refills it
    }
    // the next put's history: the last 28 samples of [history | row] (fractresampler.cpp:179-182)
    float h = 0.f;
    const bool hl = tid < RS_PERIODS * W;
    if (hl) {
        const int j = p.n + tid / W, w = tid % W;
        h = j < RS_PERIODS ? hist[W * j + w] : in[W * (j - RS_PERIODS) + w];
    }
    __syncthreads();                     // every read of the old history is done
    if (hl) hist[tid] = h;
    if (tid == 0) {
        a.t[ch] = t - (double)p.n;
        a.count[ch] = total < a.out_cap ? total : a.out_cap;
    }
}

hipError_t soundsink_batch_launch(const SinkBatchArgs &a, int stereo, hipStream_t s)
{
    if (stereo) hipLaunchKernelGGL(soundsink_batch_kernel<2>, dim3(a.channels), dim3(SB_THREADS), 0, s, a);
    else hipLaunchKernelGGL(soundsink_batch_kernel<1>, dim3(a.channels), dim3(SB_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace csdr
