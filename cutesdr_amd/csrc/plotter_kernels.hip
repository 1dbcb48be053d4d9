// plotter_kernels.hip -- K11: CPlotter::draw (gui/plotter.cpp:408-480) of every running view of a plotter batch in one
// launch, and the readers' copy kernels.
//
// Layout of the draw.  blockIdx.y is a view of the call, blockIdx.x a tile of its pixels.  A pixel belongs to a group
// of g lanes, g the power of two at or above the view's bins per pixel (64 at the most, 1 where a pixel reads one
// bin): the workgroup's 256 threads hold 256 / g neighbouring pixels, whose runs of bins lie back to back in the row of
// bels, so a wave's load instruction covers one contiguous stretch of up to 256 bytes whatever g is.  Lane j of a group
// walks its pixel's run from entry j in steps of g, keeping the largest bel (the smallest in a view whose stale
// m_MindB lies above m_MaxdB, pl::run_keeps_smallest); log2(g) shuffles inside the group finish the segmented
// extremum; lane 0 of the group turns it into both levels (pl::level: the smallest level of a run is the level of
// that bel) and stores the waterfall pixel into the ring row the host chose and the trace pixel.  Each
// bel is read once, every pixel of [0, w) is stored exactly once, and nothing is accumulated through memory: no
// atomics, no fill pass, no buffer of levels, the same words on every run.  Thread 0 of a view's first tile takes the
// pen step (SetADOverload's command, then draw()'s one-shot counter) on the view's state words, which no other
// workgroup of the launch touches.
#include "plotter_kernels.h"

namespace csdr {
namespace pl {

__global__ __launch_bounds__(256) void plotter_draw_kernel(DrawArgs a)
{
    const ViewParam &p = a.par[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ViewState st = a.state[p.view];
        if (p.ad_cmd >= 0) { st.ad_overload = p.ad_cmd; st.counter = 0; }        // SetADOverload (plotter.h:43)
        if (p.draws) st.pen = pen_step(&st.ad_overload, &st.counter, a.over[p.row] != 0);
        a.state[p.view] = st;
    }
    const int g = p.group, per = 256 / g, w = p.w;
    if (!p.draws || (int)blockIdx.x * per >= w) return;                          // the same for the whole workgroup
    const int x = (int)blockIdx.x * per + (int)threadIdx.x / g, sub = (int)threadIdx.x & (g - 1);
    const bool live = x < w;
    Map m;
    m.bin_min = p.bin_min; m.bin_max = p.bin_max; m.bins = p.bins;
    int lo, hi;
    pixel_bins(m, a.n, a.invert, w, live ? x : w - 1, &lo, &hi);                 // a group past the edge repeats the last pixel
    const float *ave = a.ave + (size_t)p.row * (size_t)a.n;
    const int smallest = p.smallest;                    // a stale m_MindB above m_MaxdB: the level rises with the bel
    float top = run_start(smallest);
    for (int i = lo + sub; i <= hi; i += g) top = run_keep(top, ave[i], smallest);
    for (int d = g >> 1; d > 0; d >>= 1) top = run_keep(top, __shfl_xor(top, d), smallest);
    if (!live || sub != 0) return;
    if (p.wf_h > 0) p.ring[(size_t)p.head * (size_t)w + x] = a.palette[255 - level(255, p.gain, p.off, top)];   // :436-441
    p.trace[x] = level(p.h2d, p.gain, p.off, top);
}

hipError_t plotter_draw_launch(const DrawArgs &a, hipStream_t s)
{
    if (a.count < 1) return hipSuccess;
    hipLaunchKernelGGL(plotter_draw_kernel, dim3(a.max_tiles < 1 ? 1 : a.max_tiles, a.count), dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void plotter_rows_kernel(const RowParam *par, unsigned *out, long long stride,
                                                           const ViewState *state, int *pen)
{
    const int v = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    const RowParam &p = par[v];
    if (pen && x == 0) pen[v] = state[v].pen;
    if (x >= p.w) return;
    out[(long long)v * stride + x] = p.src ? p.src[x] : p.fill;
}
hipError_t plotter_rows_launch(const RowParam *par, int views, int max_w, unsigned *out, long long stride,
                               const ViewState *state, int *pen, hipStream_t s)
{
    if (max_w < 1 && !pen) return hipSuccess;
    hipLaunchKernelGGL(plotter_rows_kernel, dim3(max_w < 1 ? 1 : (max_w + 255) / 256, views), dim3(256), 0, s, par, out,
                       stride, state, pen);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void plotter_unroll_kernel(const unsigned *ring, int w, int wf_h, int head, int filled,
                                                             unsigned *out)
{
    const int r = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    out[(size_t)r * w + x] = r < filled ? ring[(size_t)((head + r) % wf_h) * w + x] : kBlack;
}
hipError_t plotter_unroll_launch(const unsigned *ring, int w, int wf_h, int head, int filled, unsigned *out, hipStream_t s)
{
    if (w < 1 || wf_h < 1) return hipSuccess;
    hipLaunchKernelGGL(plotter_unroll_kernel, dim3((w + 255) / 256, wf_h), dim3(256), 0, s, ring, w, wf_h, head, filled, out);
    return hipGetLastError();
}

}  // namespace pl
}  // namespace csdr
