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
//
// The FFT view (DisplayData's frequency branch :594-611 / :654-672, DrawFftPlot :1005-1068).  CTestBench runs its CFft
// with an average of 1 (SetFFTAve(0), :132; dsp/fft.cpp:103-113), so the bels after a used frame depend on that frame
// alone, and the peak hold is a per-pixel minimum, which commutes: the work item is one (receiver, used frame), a
// workgroup of ONE wave that holds the 2048-point frame as 64 lanes x 32 points (spectrum_passes.hpp, K3's transform).
// scope_put_kernel stays the launch in front: for an FFT-view receiver it applies the flags (peak back to h, ring
// zeroed), appends the call's tail to the carried partial frame and brings the counters up to date, all from the
// host's plan (sc::ChanParam) -- so a peak reset lands before this put's minima.  The new partial frame goes into the
// OTHER of two carry buffers, so the frame that begins in the old one can be read by scope_fft_kernel afterwards.
#define CSDR_FMA_BFLY 1
#define CSDR_PLAIN_CONST_FMA 1
#include "spectrum_passes.hpp"
#include "scope_kernels.h"

namespace csdr {
namespace {

constexpr int kThreads = 512;

// The four overloads of DisplayData as row kinds: 0 TYPEREAL (:643-695), 1 TYPECPX (:583-636), 2 TYPEMONO16 (:702-754),
// 3 TYPESTEREO16 (:761-814).  A kind says where row c begins, what an emission writes into the ring (get), what
// ChkForTrigger and m_PreviousSample see (trig) and what a sample is in m_FftInBuf (frame).  They differ only for
// TYPEMONO16: the trigger looks at pBuf[i<<1] (:741) -- index 2i inside the call's n samples, 0 past them (deviation (7):
// the reference reads past its buffer) -- and the FFT frame entry is (x, x) (:718-719).
template <int CPX> struct Row {
    const float *p; long long n;
    static __device__ const float *at(const ScopeArgs &a, int c)
    {
        if constexpr (CPX >= 2) return (const float *)((const short *)a.rows + (size_t)c * (size_t)a.stride * (CPX == 3 ? 2 : 1));
        else return a.rows + (size_t)c * (size_t)a.stride * (CPX ? 2 : 1);
    }
    __device__ void get(long long s, int &re, int &im) const
    {
        s = s < n ? s : n - 1;                           // an emission's sample is < n by construction
        if constexpr (CPX == 3) { const short2 v = ((const short2 *)p)[s]; re = v.x; im = v.y; }
        else if constexpr (CPX == 2) { re = ((const short *)p)[s]; im = 0; }
        else if (CPX) { const float2 v = ((const float2 *)p)[s]; re = sc::sat_int(v.x); im = sc::sat_int(v.y); }
        else { re = sc::sat_int(p[s]); im = 0; }
    }
    __device__ int trig(long long s) const
    {
        if constexpr (CPX == 2) { s = s < n ? s : n - 1; return 2 * s < n ? ((const short *)p)[2 * s] : 0; }
        else { int re, im; get(s, re, im); return re; }
    }
    static __device__ float2 frame(const float *row, long long s)
    {
        if constexpr (CPX == 3) { const short2 v = ((const short2 *)row)[s]; return make_float2((float)v.x, (float)v.y); }
        else if constexpr (CPX == 2) { const float x = (float)((const short *)row)[s]; return make_float2(x, x); }
        else return CPX ? ((const float2 *)row)[s] : make_float2(row[s], 0.f);
    }
};

template <int CPX> __global__ __launch_bounds__(kThreads) void scope_put_kernel(ScopeArgs a)
{
    const int c = blockIdx.x, tid = threadIdx.x, w = a.w;
    const sc::ChanParam par = a.par[c];
    sc::ChanState st = a.state[c];
    int *ring = a.ring + (size_t)c * 2 * sc::kMaxW, *screen = a.screen + (size_t)c * 2 * sc::kMaxW;
    __shared__ unsigned long long s_first;

    if (par.flags & (sc::F_RESET | sc::F_PEAK)) {        // Reset() :555-560, OnEnablePeak :336-341: in either view
        int *peak = a.peak + (size_t)c * sc::kMaxW;
        for (int i = tid; i < 2 * sc::kMaxW; i += kThreads) ring[i] = 0;
        for (int i = tid; i < sc::kMaxW; i += kThreads) peak[i] = par.h;
        if (par.flags & sc::F_RESET) {                   // ResetFFT (:573; dsp/fft.cpp:248-259), m_FftBufPos = 0 (:536)
            float *bels = a.bels + (size_t)c * sc::kFftN;
            for (int i = tid; i < sc::kFftN; i += kThreads) bels[i] = 0.f;
            if (tid == 0) { a.fst[c].pos = 0; a.fst[c].total = 0; }
        }
        __syncthreads();
    }
    sc::apply_flags(st, par.flags);
    if (par.view == sc::VIEW_FFT) {                      // :594-611 / :654-672 without the frames: scope_fft_kernel's
        if (par.n > 0) {
            const float *row = Row<CPX>::at(a, c);
            float2 *carry = (float2 *)a.carry + (size_t)c * 2 * sc::kFftN;
            // no frame completes: the samples join the partial frame; else the tail after the last complete frame
            // starts the other buffer
            float2 *dst = par.frames == 0 ? carry + (size_t)par.cur * sc::kFftN + par.fill : carry + (size_t)(par.cur ^ 1) * sc::kFftN;
            const int cnt = par.frames == 0 ? par.n : par.pos_end, from = par.n - cnt;
            for (int i = tid; i < cnt; i += kThreads)
                dst[i] = Row<CPX>::frame(row, from + i);
            if (tid == 0) {
                sc::FftState f = a.fst[c];
                f.pos = par.pos_end; f.total += par.count;
                if (par.count > 0) f.cpx = scope_kind_cpx(CPX);
                a.fst[c] = f;
                st.skipcounter = par.cnt_end; st.emits += (unsigned)par.count;     // emit NewFftData, :607
            }
        }
        if ((par.flags || par.n > 0) && tid == 0) a.state[c] = st;
        return;
    }
    const long long n = par.n;
    if (n <= 0) {
        if (par.flags && tid == 0) a.state[c] = st;
        return;
    }
    const Row<CPX> row = {Row<CPX>::at(a, c), n};
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
                const int cur = row.trig(pl.sample(e));
                const int prv = e == 0 ? st.prev : row.trig(pl.sample(e - 1));
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
        if (E > 0) st.prev = row.trig(pl.sample(E - 1));            // :897
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

// One used frame of one FFT-view receiver: blockIdx.y the receiver, blockIdx.x the frame's number k among the call's
// used frames (a receiver with fewer leaves at once: the counts differ by receiver only where the skip values do).
// Load (frame first + k step of the frames that complete; the call's first may begin in the carry), window and I/Q
// swap (dsp/fft.cpp:267-288), K3's transform, |X|^2, log10f(p + K_C) + K_B in K3's epilogue arithmetic (an average of
// 1: mean = p / 1), the bels in display order into LDS, then one lane per pixel reduces to y (sc::fft_pixel) and a plain
// vector atomicMin folds it into the peak.  The receiver's last used frame also writes the screen and the 2048 bels.
using FftCfg = SpecCfg<11>;
template <int CPX> __global__ __launch_bounds__(FftCfg::T) void scope_fft_kernel(ScopeArgs a)
{
    constexpr int N = sc::kFftN, R0 = FftCfg::R0, G = FftCfg::G;
    static_assert(FftCfg::N == N && FftCfg::T == 64, "one wave per frame");
    const int c = blockIdx.y, k = blockIdx.x, t = threadIdx.x;
    const sc::ChanParam &par = a.par[c];
    if (par.view != sc::VIEW_FFT || k >= par.count) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2f *lds = reinterpret_cast<v2f *>(smem_raw);
    v2f *tw2 = lds + FftCfg::LDS_DATA;
    for (int i = t; i < 1024; i += FftCfg::T) tw2[i] = reinterpret_cast<const v2f *>(a.tw2)[i];
    v2f w1[G];
#pragma unroll
    for (int e = 0; e < G; e++) w1[e] = reinterpret_cast<const v2f *>(a.tw1)[FftCfg::col(t, e)];
    const long long j = (long long)par.first + (long long)k * par.step;          // < par.frames
    const int fill = par.fill;
    const v2f *carry = reinterpret_cast<const v2f *>(a.carry) + ((size_t)c * 2 + par.cur) * N;
    const float *row = Row<CPX>::at(a, c);
    v2f x[32];
#pragma unroll
    for (int e = 0; e < G; e++)
#pragma unroll
        for (int n1 = 0; n1 < R0; n1++) {
            const int i = 1024 * n1 + FftCfg::col(t, e);
            const long long s = sc::fft_source(j, i, fill);                      // < par.n: frame j completes in the call
            v2f v;
            if (s < 0) v = carry[s + fill];
            else if constexpr (CPX >= 2) { const float2 f = Row<CPX>::frame(row, s); v = v2f{f.x, f.y}; }
            else if (CPX) v = reinterpret_cast<const v2f *>(row)[s];
            else v = v2f{row[s], 0.f};
            const float w = a.win[i];
            x[e * R0 + n1] = v2f{w * v.y, w * v.x};                              // I/Q swapped, fft.cpp:280-281
        }
    fft_fwd_passes<11>(x, lds, tw2, w1);
    __syncthreads();                                     // pass C has read its rows: the bels take their place
    float *bel = reinterpret_cast<float *>(smem_raw);
    const bool last = k == par.count - 1;
    float *out = a.bels + (size_t)c * N;
    int tt = t;
    asm volatile("" : "+v"(tt));
    const int k0 = tt >> 5, k1 = tt & 31;
    static_for<0, 32>([&](auto Rr) {
        constexpr int r = Rr.value;
        const int d = ((k0 + R0 * (k1 + 32 * r)) + N / 2) & (N - 1);             // display order, fft.cpp:564-589
        const float p = x[r].x * x[r].x + x[r].y * x[r].y;
        const float b = (float)((double)log10f(p + a.kc) + a.kb);      // sum - sum + p, over a count of 1
        bel[d] = b;
        if (last) out[d] = b;
    });
    __syncthreads();
    const sc::FftMap map = par.map;
    int *peak = a.peak + (size_t)c * sc::kMaxW, *screen = a.fscreen + (size_t)c * sc::kMaxW;
    for (int px = t; px < a.w; px += FftCfg::T) {
        const int y = sc::fft_pixel(map, a.w, px, [&](int i) { return (double)bel[i]; });
        atomicMin(&peak[px], y);                                                 // :1050-1051
        if (last) screen[px] = y;
    }
}

// every FFT-view receiver's last screen and its peak trace; a time-view receiver's rows are left alone
__global__ __launch_bounds__(256) void scope_fft_screens_kernel(ScopeFftScreenArgs a)
{
    const int c = blockIdx.x;
    if (a.par[c].view != sc::VIEW_FFT) return;
    for (int i = threadIdx.x; i < 2 * a.w; i += 256) {
        const int k = i >= a.w, x = k ? i - a.w : i;
        a.out[((size_t)c * 2 + k) * (size_t)a.out_stride + x] = (k ? a.peak : a.fscreen)[(size_t)c * sc::kMaxW + x];
    }
}

}  // namespace

template <int KIND> static void scope_put_kind(const ScopeArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(scope_put_kernel<KIND>, dim3(a.channels), dim3(kThreads), 0, s, a);
    if (a.max_count > 0)
        hipLaunchKernelGGL(scope_fft_kernel<KIND>, dim3(a.max_count, a.channels), dim3(FftCfg::T), FftCfg::LDS_BYTES, s, a);
}
hipError_t scope_put_launch(const ScopeArgs &a, int kind, hipStream_t s)
{
    switch (kind) {
    case SCOPE_REAL:     scope_put_kind<SCOPE_REAL>(a, s); break;
    case SCOPE_CPX:      scope_put_kind<SCOPE_CPX>(a, s); break;
    case SCOPE_MONO16:   scope_put_kind<SCOPE_MONO16>(a, s); break;
    case SCOPE_STEREO16: scope_put_kind<SCOPE_STEREO16>(a, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t scope_fft_screens_launch(const ScopeFftScreenArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(scope_fft_screens_kernel, dim3(a.channels), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t scope_screens_launch(const ScopeScreenArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(scope_screens_kernel, dim3(a.channels), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace csdr
