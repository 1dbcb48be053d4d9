// spectrum_kernels.h -- launch interface of the CFft kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "frontend_kernels.h"
#include "display_plan.hpp"

namespace csdr {

struct SpectrumArgs {
    const float *in;  long in_stride;   // complex fp32 [channels][in_stride], frames back to back
    const float *win;                   // [N] window (Hann*2, dsp/fft.cpp:196-198)
    const float *tw1, *tw2;             // twiddle tables as for the FastFIR kernel
    float *sum, *pwr;                   // [channels][N] running sum / mean power (display order)
    float *ave;                         // [channels][N] log10(mean + K_C) + K_B, in bels
    int *counters;                      // [channels][2]: ave_count, total_count
    int *overload;                      // [channels]
    int channels, nframes, ave_size;
    int nparts;                         // frame groups per channel (1: the frames of a channel run in one workgroup)
    float *part;                        // [channels][nparts][N] partial sums, nparts > 1 only
    float *alpha;                       // [channels][nparts] group weights + [channels] average count after the call (nparts > 1)
    float kc; double kb;
    // the display stream's loaders (spectrum_stream_launch only; the plain launch reads frame f at in + f N):
    // frame f of a channel is stream samples frame_start + f frame_step + i (frame_start >= 0), minus dc
    long frame_start, frame_step;
    const double *dc;                   // optional [channels][2] (I, Q), subtracted as unpack_kernel does
    const unsigned char *pk; long pk_stride;   // datagrams [channels][pk_stride] bytes (wire_format.hpp), or nullptr: `in`
    // behind a blanked chain call (StreamSrc in display_stream_kernels.h): the stream sample is the one delay_n + 1 behind,
    // zero under the mask.  The blanked loaders read no history: frame_start >= NB_MAX_WIDTH / 2 + 1 with them.
    const unsigned *nb_mask; long nb_mask_stride;   // [channels][stride] words; nullptr: no blanker
    const NbChan *nb_state;                         // [channels]: on, delay_n
    // the row form (display_plan.hpp): a table of the nrows ACTIVE rows of this launch.  A workgroup finds its channel
    // through its entry and takes nframes, ave_size, frame_start and frame_step from it; the fields above of those names
    // are not read.  part and alpha stay indexed by channel.  nullptr: the uniform form, every channel nframes frames.
    const SpecRow *rows = nullptr; int nrows = 0;
};
// The frame groups of a row of nframes frames in a launch with room for `room` workgroups per row: eight frames a group
// at least.  The host sizes the launch with it (capi_fft.hip, from the longest row) and the kernels find each row's own
// count with it, so what a row computes depends on its own frames alone.
__host__ __device__ inline int spectrum_groups(int nframes, int room)
{
    const int g = nframes / 8;
    return g < 1 ? 1 : (g < room ? g : room);
}
// The size classes, from the largest size that a kind of loader has a kernel for (the other sizes gather their frames,
// capi_fft.hip).  The display stream's loaders run in the sixteen-point kernels only: at 16384 points
// (spectrum_kernel<14>, 512 threads, at most 256 registers) the datagram loaders spilled 164 / 236 bytes and the DC row
// loader 12 bytes of scratch per lane.  The blanked loaders exist at 2048 and 4096 points: at 8192 points
// (spectrum32_kernel, 512 threads: at most 256 registers) the mask word per prefetched sample spilled -- 72 bytes of
// scratch per lane on fp32 rows, 16 on 16-bit and 124 on 24-bit datagrams.
constexpr int SPEC_MIN_LOG2N = 11, PLAIN_MAX_LOG2N = 14, STREAM_MAX_LOG2N = 13, BLANKED_MAX_LOG2N = 12;
// one launch per call (spectrum_launch, fft_plain_launch); the other sizes go through HBM in several (spectrum_generic_launch)
constexpr bool spectrum_single_launch(int log2n) { return log2n >= SPEC_MIN_LOG2N && log2n <= PLAIN_MAX_LOG2N; }
// The workgroups of one round on the chip: 4 / 2 / 1 per CU at 4096 / 8192 / 16384 points (their LDS images; 2048 points
// fit eight, and measure 2 % better with four).  (Until round 4 the target was 1024 workgroups for every size, as it still
// is for the multi-launch ones: at 16384 points that was four rounds, and a workgroup's start -- tables, window, sums, the
// first frame's latency -- costs five frames' time: 0.39 ms for 256 channels x 32 frames against 0.33; 8192 points -2 %.)
constexpr int spectrum_round_slots(int log2n)
{
    return !spectrum_single_launch(log2n) ? 1024 : 256 * (log2n <= 12 ? 4 : (log2n == 13 ? 2 : 1));
}
// the stream loaders (spectrum_stream_launch), and their blanked form (pkt_len 0: fp32 rows)
constexpr bool spectrum_stream_loaders_ok(int log2n) { return log2n >= SPEC_MIN_LOG2N && log2n <= STREAM_MAX_LOG2N; }
constexpr bool spectrum_stream_blanked_ok(int log2n, int pkt_len)
{
    return log2n >= SPEC_MIN_LOG2N && log2n <= BLANKED_MAX_LOG2N && (pkt_len == 0 || pkt_len == 1028 || pkt_len == 1444);
}
hipError_t spectrum_launch(int log2n, const SpectrumArgs &a, hipStream_t stream);
// 2048 ... 8192 points with the frame load of the display stream: fp32 rows (a.pk == nullptr) or datagrams of
// pkt_len 1028 / 1444 decoded in the load, frames at frame_start + f frame_step, DC subtracted
hipError_t spectrum_stream_launch(int log2n, const SpectrumArgs &a, int pkt_len, hipStream_t stream);

// plain transform of one N-point block: sign=+1 CFft::FwdFFT, -1 RevFFT; natural order in/out
hipError_t fft_plain_launch(int log2n, int sign, const float *in, float *out, const float *tw1,
                            const float *tw2, hipStream_t stream);

// plain transforms of nframes frames of every row (fft_batch_plain_kernels.hip), 512 ... 65536 points: frame k of row c
// at in + 2 (c in_stride + k N) floats, its transform at the same place of out; in == out with equal strides is in place
struct PlainBatchArgs {
    const float *in;  long in_stride;   // complex fp32 [channels][in_stride]
    float *out;       long out_stride;
    int channels, nframes, sign;        // sign=+1 CFft::FwdFFT, -1 RevFFT
    const float *tw1, *tw2;             // the object's tables (tw1 is W_N^i, i < 1024: all of it at 512 and 1024 points)
    const float *twp;                   // 32768 and 65536 points: [256] W_256^m, then [256] W_N^m
    float *work; int group;             // 32768 and 65536 points: the intermediate of `group` frames of every row,
};                                      // [channels][group][N] complex; longer calls go through it in groups
hipError_t fft_batch_plain_launch(int log2n, const PlainBatchArgs &a, hipStream_t stream);

// CFft::GetScreenIntegerFFTData (fft.cpp:308-410) for every channel: ave [channels][n] bels (display order)
// -> out [channels][out_stride] pixels; the bin range / pixel count come precomputed from the host
struct ScreenArgs {
    const float *ave; int *out; long out_stride;
    int n, channels, bin_min, bin_max, plot_w, max_h, invert;
    double off, gain;                   // MaxdB/10 and -10/(MaxdB-MindB)
};
hipError_t screen_launch(const ScreenArgs &a, hipStream_t stream);
// CPlotter's palette entry i (gui/plotter.cpp:67-83) as 0xFFRRGGBB
unsigned plotter_color(int i);
// levels [channels][stride] (0..255, or < 0 = pixel not touched) -> palette[255 - level] in rgb [channels][rgb_stride]
hipError_t waterfall_color_launch(const int *levels, long stride, unsigned *rgb, long rgb_stride, int w, int channels,
                                  hipStream_t stream);

// sizes outside 2048..16384 (512, 1024, 32768, 65536): multi-launch transform through HBM.
// work: [2][channels][N] complex for the spectrum, [2][N] for the plain transform
hipError_t spectrum_generic_launch(int log2n, const SpectrumArgs &a, float *work, hipStream_t stream,
                                   const SpecRow *h_rows = nullptr);
hipError_t fft_generic_plain_launch(int log2n, int sign, const float *in, float *out, float *work, hipStream_t stream);

}  // namespace csdr
