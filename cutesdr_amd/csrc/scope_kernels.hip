// scope_kernels.hip -- K10: the batch test-bench scope's time view (reference gui/testbench.cpp: DisplayData :613-635
// / :673-694, ChkForTrigger :819-898, DrawTimePlot's vertical mapping :973-988).  One workgroup per receiver walks
// the emissions of the call, not its samples: where the sweep is longer than the screen only the emitted samples are
// read.  Everything a receiver carries from call to call is in ChanState, its ring and its screen; the settings of
// the call come in ChanParam (scope_host.hpp).
//
// The ring arithmetic of :884-894 worked out: the screen position of an emission is its number since the last reset
// modulo w, so when a display happens at emission d (before d is written) ring slot j holds the last emission whose
// position was j, and the w entries copied out are
//     triggered modes:  emissions d-w .. d-1 in order (d = trigger emission + max(Post, 1), Post = (7*w)/10)
//     TRIG_OFF:         the same w emissions rotated by Post (m_TrigBufPos = 0, d at screen position 0)
// with zeros for emissions before the reset (Reset clears the ring).  Emissions before this call come from the
// carried ring; their slots are overwritten only by emissions >= d.
#include "scope_kernels.h"

namespace csdr {
namespace {

constexpr int kThreads = 512;

template <int CPX> struct Row {
    const float *p; long long n;
    __device__ void get(long long s, int &re, int &im) const
    {
        s = s < n ? s : n - 1;                           // an emission's sample is < n by construction
        if (CPX) { const float2 v = ((const float2 *)p)[s]; re = sc::sat_int(v.x); im = sc::sat_int(v.y); }
        else { re = sc::sat_int(p[s]); im = 0; }
    }
};

template <int CPX> __global__ __launch_bounds__(kThreads) void scope_put_kernel(ScopeArgs a)
{
    const int c = blockIdx.x, tid = threadIdx.x, w = a.w;
    const sc::ChanParam par = a.par[c];
    sc::ChanState st = a.state[c];
    int *ring = a.ring + (size_t)c * 2 * sc::kMaxW, *screen = a.screen + (size_t)c * 2 * sc::kMaxW;
    __shared__ unsigned long long s_first;

    if (par.flags & sc::F_RESET) {                       // Reset(), :555-560
        for (int i = tid; i < 2 * sc::kMaxW; i += kThreads) ring[i] = 0;
        __syncthreads();
    }
    sc::apply_flags(st, par.flags);
    const long long n = par.n;
    if (n <= 0) {
        if (par.flags && tid == 0) a.state[c] = st;
        return;
    }
    const Row<CPX> row = {a.rows + (size_t)c * (size_t)a.stride * (CPX ? 2 : 1), n};
    const sc::Plan pl = sc::make_plan(st.inpos, st.pos, par.pix, par.sr, w, n);
    const long long E = pl.emits;
    const int pos0 = st.pos;

    long long trig = -1;
    if (sc::searches(st, par)) {                         // :837-846 / :858-867: the first crossing, in parallel
        if (tid == 0) s_first = ~0ull;
        __syncthreads();
        for (long long base = 0; base < E; base += kThreads) {
            const long long e = base + tid;
            bool hit = false;
            if (e < E) {
                int cur, prv, im;
                row.get(pl.sample(e), cur, im);
                if (e == 0) prv = st.prev; else row.get(pl.sample(e - 1), prv, im);
                hit = sc::crossing(par.mode, par.level, cur, prv);
            }
            if (__syncthreads_or(hit)) {
                const unsigned long long b = __ballot(hit);
                if (b && (tid & 63) == __ffsll((long long)b) - 1) atomicMin(&s_first, (unsigned long long)e);
                __syncthreads();
                trig = (long long)s_first;
                break;
            }
        }
    }
    const sc::Display d = sc::decide(st, par, w, E, trig);
    if (d.at >= 0) {                                     // :884-894
        for (int i = tid; i < w; i += kThreads) {
            int re, im, slot = 0;
            const long long e = sc::screen_source(d, i, w, pos0, &slot);
            if (e >= 0) row.get(pl.sample(e), re, im);
            else { re = ring[slot]; im = ring[sc::kMaxW + slot]; }
            screen[i] = re; screen[sc::kMaxW + i] = im;
        }
    }
    __syncthreads();                                     // the carried ring has been read
    const long long lo = E > w ? E - w : 0;              // :624-625: the last min(w, E) emissions
    for (long long e = lo + tid; e < E; e += kThreads) {
        int re, im;
        row.get(pl.sample(e), re, im);
        const int slot = (int)((pos0 + e) % w);
        ring[slot] = re; ring[sc::kMaxW + slot] = im;
    }
    if (tid == 0) {
        int im;
        if (E > 0) row.get(pl.sample(E - 1), st.prev, im);          // :897
        st.inpos = pl.inpos_end; st.pos = pl.pos_end;
        a.state[c] = st;
    }
}

// every receiver's last screen and, optionally, DrawTimePlot's vertical mapping (:973-988) of both halves
__global__ __launch_bounds__(256) void scope_screens_kernel(ScopeScreenArgs a)
{
    const int c = blockIdx.x;
    const int *scr = a.screen + (size_t)c * 2 * sc::kMaxW;
    const long long half = a.h / 2, vert = a.y ? a.par[c].vert : 1;
    for (int i = threadIdx.x; i < 2 * a.w; i += 256) {
        const int k = i >= a.w, x = k ? i - a.w : i;
        const int v = scr[k * sc::kMaxW + x];
        a.out[((size_t)c * 2 + k) * (size_t)a.out_stride + x] = v;
        if (a.y) {
            const long long y = vert ? half - (2 * half * (long long)v) / vert : half;
            a.y[((size_t)c * 2 + k) * (size_t)a.y_stride + x] = y > INT_MAX ? INT_MAX : y < INT_MIN ? INT_MIN : (int)y;
        }
    }
}

}  // namespace

hipError_t scope_put_launch(const ScopeArgs &a, int cpx, hipStream_t s)
{
    if (cpx) hipLaunchKernelGGL(scope_put_kernel<1>, dim3(a.channels), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(scope_put_kernel<0>, dim3(a.channels), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t scope_screens_launch(const ScopeScreenArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(scope_screens_kernel, dim3(a.channels), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace csdr
