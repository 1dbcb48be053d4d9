// scope_kernels.h -- launch interface of the batch test-bench scope's kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "scope_host.hpp"

namespace csdr {

// the kinds of rows a put reads, one per DisplayData overload (gui/testbench.cpp:643, :583, :702, :761)
enum { SCOPE_REAL = 0, SCOPE_CPX = 1, SCOPE_MONO16 = 2, SCOPE_STEREO16 = 3 };
constexpr bool scope_kind_cpx(int kind) { return kind == SCOPE_CPX || kind == SCOPE_STEREO16; }      // m_NewDataIsCpx

struct ScopeArgs {
    const float *rows; long long stride;     // [channels][stride] fp32 real or complex fp32 pairs -- or int16 / int16 pairs behind the
                                             // same pointer (SCOPE_MONO16 / _STEREO16) --, stride in samples; never written
    const sc::ChanParam *par;                // [channels], device memory
    sc::ChanState *state;                    // [channels]
    int *ring;                               // [channels][2][kMaxW]: m_TimeBuf1/2
    int *screen;                             // [channels][2][kMaxW]: m_TimeScrnBuf1/2
    int w, channels;
    // the FFT view
    sc::FftState *fst;                       // [channels]
    float *carry;                            // [channels][2][kFftN] complex fp32: m_FftInBuf, two buffers switched per put
    float *bels;                             // [channels][kFftN]: m_pFFTAveBuf of the last used frame
    int *fscreen, *peak;                     // [channels][kMaxW] each: the last drawn y, m_FftPkBuf
    const float *win, *tw1, *tw2;            // the 2048-point tables of spectrum_passes.hpp: window, W_2048^i, W_1024^(i k)
    float kc; double kb;                     // CFft's K_C and K_B / 10 at 2048 points, dB compensation 0
    int max_count;                           // the largest number of used frames of a receiver in this call
};
// the put of every receiver: one launch, and one more for the used frames of the FFT-view receivers when there are any
hipError_t scope_put_launch(const ScopeArgs &a, int kind, hipStream_t s);

struct ScopeFftScreenArgs {
    const int *fscreen, *peak;               // [channels][kMaxW]
    const sc::ChanParam *par;                // [channels]: view
    int *out; long long out_stride;          // [channels][2][out_stride]: screen, peak
    int w, channels;
};
hipError_t scope_fft_screens_launch(const ScopeFftScreenArgs &a, hipStream_t s);

struct ScopeScreenArgs {
    const int *screen;                       // [channels][2][kMaxW]
    const sc::ChanParam *par;                // [channels]: vert (only read when y is set)
    int *out; long long out_stride;          // [channels][2][out_stride]
    int *y; long long y_stride;              // [channels][2][y_stride] or nullptr
    int w, h, channels;
};
hipError_t scope_screens_launch(const ScopeScreenArgs &a, hipStream_t s);

}  // namespace csdr
