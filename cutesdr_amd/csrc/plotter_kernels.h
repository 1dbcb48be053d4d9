// plotter_kernels.h -- launch interface of the batch plotter's kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "plotter_host.hpp"

namespace csdr {
namespace pl {

// what the device keeps per view: the pen depends on the FFT's overload flag, which only the device knows
struct ViewState {
    int ad_overload, counter;                            // m_ADOverLoad, m_ADOverloadOneShotCounter
    int pen;                                             // the last draw's pen: 1 red, 0 green
    int pad;
};

// one view of one draw call, as the host prepared it
struct ViewParam {
    int view, row;                                       // index into the states; spectrum row
    int draws;                                           // 1: running -- the pen step, and pixels when w > 0
    int w, h2d, wf_h;
    int bin_min, bin_max, bins;                          // pl::Map
    int group;                                           // lanes per pixel, a power of two up to 64
    int head;                                            // the ring row that receives the new line
    int ad_cmd;                                          // SetADOverload: -1 none, 0 / 1
    int smallest;                                        // pl::run_keeps_smallest: gain > 0, a run shows its smallest bel
    int pad;
    double gain, off;
    int *trace;                                          // [w]
    unsigned *ring;                                      // [wf_h][w]
};

struct DrawArgs {
    const ViewParam *par; int count;                     // the views of this call that have anything to do
    ViewState *state;                                    // [views]
    const float *ave;                                    // [channels][n] bels, display order; never written
    const int *over;                                     // [channels] overload words
    const unsigned *palette;                             // [256] m_ColorTbl
    int n, invert;
    int max_tiles;                                       // the largest number of workgroups a view of the call needs
};
hipError_t plotter_draw_launch(const DrawArgs &a, hipStream_t s);

// one row per view into out[v][stride]: src[0..w) where src is set, `fill` where it is not; w == 0: nothing
struct RowParam {
    const unsigned *src;
    int w;
    unsigned fill;
};
hipError_t plotter_rows_launch(const RowParam *par, int views, int max_w, unsigned *out, long long stride,
                               const ViewState *state, int *pen, hipStream_t s);
// a view's image unrolled: out[r][w] = ring row (head + r) % wf_h for r < filled, black below
hipError_t plotter_unroll_launch(const unsigned *ring, int w, int wf_h, int head, int filled, unsigned *out, hipStream_t s);

}  // namespace pl
}  // namespace csdr
