// fft_batch_plain_kernels.hip -- CFft::FwdFFT / RevFFT (dsp/fft.cpp:416-426) of many frames of many rows in one call
// (csdr_fft_batch_fwd / _rev): device rows in, device rows out, nothing of the display state touched.
//
//   2048 ... 16384 points   one workgroup per (row, frame) on fft_fwd_passes (spectrum_passes.hpp), as fft_plain_kernel
//   512, 1024 points        a frame is 64 threads x 8 / 16 points; four frames per workgroup; three Stockham passes
//                           (8 8 8 / 16 16 4) through 4.5 / 8.5 KB of LDS per frame, first pass read from and last pass
//                           written to global memory directly
//   32768, 65536 points     the four-step form N = 256 x N2 in two launches: (1) per workgroup 16 neighbouring columns
//                           n2 of the 256 x N2 input matrix: 256-point transforms over n1, times W_N^(n2 k1), to the work
//                           buffer as [k1][n2]; (2) per workgroup 16 neighbouring rows k1 of it: N2-point transforms over
//                           n2, bin k1 + 256 k2 out.  Every global access of a wave is a set of 128-byte stretches.
//
// The negative exponent (RevFFT) is the positive one on conjugated input, conjugated again on the way out.
// Every twiddle comes from a table rounded from fp64 (capi_fft.hip: fft_set_params); W_N^(n2 k1) is the product of two
// table entries, W_N^(256 hi) W_N^lo.
#define CSDR_FMA_BFLY 1
#define CSDR_PLAIN_CONST_FMA 1
#include "launch_once.hpp"
#include <type_traits>
#include "fft_core.hpp"
#include "spectrum_passes.hpp"
#include "spectrum_kernels.h"

namespace csdr {

struct FramePtr { const v2f *in; v2f *out; };
__device__ __forceinline__ FramePtr frame_ptr(const PlainBatchArgs &a, long row, long frame, int n)
{
    return FramePtr{reinterpret_cast<const v2f *>(a.in) + row * a.in_stride + frame * n,
                    reinterpret_cast<v2f *>(a.out) + row * a.out_stride + frame * n};
}

// ---------------------------------------------------------------- 2048 ... 16384 points
template <int LOG2N>
__global__ __launch_bounds__(SpecCfg<LOG2N>::T)
void fft_batch_plain_kernel(PlainBatchArgs a)
{
    using Cfg = SpecCfg<LOG2N>;
    constexpr int T = Cfg::T, R0 = Cfg::R0, G = Cfg::G;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2f *lds = reinterpret_cast<v2f *>(smem_raw);
    v2f *tw2 = lds + Cfg::LDS_DATA;
    const int t = threadIdx.x;
    const long row = blockIdx.x / (unsigned)a.nframes, frame = blockIdx.x - row * a.nframes;
    const FramePtr p = frame_ptr(a, row, frame, Cfg::N);
    const v2f *tw1g = reinterpret_cast<const v2f *>(a.tw1), *tw2g = reinterpret_cast<const v2f *>(a.tw2);
    for (int i = t; i < 1024; i += T) tw2[i] = tw2g[i];
    v2f w1[G];
#pragma unroll
    for (int e = 0; e < G; e++) w1[e] = tw1g[Cfg::col(t, e)];
    const float cj = a.sign > 0 ? 1.0f : -1.0f;
    v2f x[32];
#pragma unroll
    for (int e = 0; e < G; e++)
#pragma unroll
        for (int n1 = 0; n1 < R0; n1++) {
            const v2f s = p.in[1024 * n1 + Cfg::col(t, e)];
            x[e * R0 + n1] = v2f{s.x, cj * s.y};
        }
    __syncthreads();
    fft_fwd_passes<LOG2N>(x, lds, tw2, w1);
    const int k0 = t >> 5, k1 = t & 31;
    __syncthreads();                       // in == out allowed: every input of the frame was read before pass A ended
    static_for<0, 32>([&](auto Rr) {
        constexpr int k2 = Rr.value;
        p.out[k0 + R0 * (k1 + 32 * k2)] = v2f{x[k2].x, cj * x[k2].y};
    });
}

// ---------------------------------------------------------------- Stockham passes (512, 1024 points, and the four-step form)
// One autosort pass of radix R over an L-point transform whose earlier passes have the product NS: butterfly j < L / R
// takes points j + r L / R, turns point r by W_(NS R)^((j mod NS) r), and its R results go to (j - j mod NS) R + j mod NS
// + r NS.  The pass is not in place, and a transform has one LDS image: a thread loads and transforms ALL its
// butterflies (sk_load), the workgroup meets, then it stores them (sk_store).  A transform is worked on by TPF threads
// (tl of them); tw is the table W_(L TWS)^m.
template <int R, int L, int TPF> struct SkRegs {
    static constexpr int ITERS = (L / R + TPF - 1) / TPF;
    v2f y[ITERS][R];
};
template <int R, int NS, int L, int TPF, int TWS, class Ld>
__device__ __forceinline__ void sk_load(int tl, const v2f *tw, SkRegs<R, L, TPF> &g, Ld ld)
{
    static_for<0, SkRegs<R, L, TPF>::ITERS>([&](auto It) {
        const int j = tl + TPF * It.value;
        if ((L / R) % TPF == 0 || j < L / R) {
            const int k = j & (NS - 1);
            v2f (&y)[R] = g.y[It.value];
            static_for<0, R>([&](auto Rr) {
                constexpr int r = Rr.value;
                v2f v = ld(j + r * (L / R));
                if constexpr (r > 0 && NS > 1) v = cmul(v, tw[TWS * (L / (NS * R)) * k * r]);
                y[bitrev<R>(r)] = v;
            });
            dft_dit<R, +1>(y);
        }
    });
}
template <int R, int NS, int L, int TPF, class St>
__device__ __forceinline__ void sk_store(int tl, const SkRegs<R, L, TPF> &g, St st)
{
    static_for<0, SkRegs<R, L, TPF>::ITERS>([&](auto It) {
        const int j = tl + TPF * It.value;
        if ((L / R) % TPF == 0 || j < L / R) {
            const int k = j & (NS - 1), base = (j - k) * R + k;
            static_for<0, R>([&](auto Rr) { st(base + Rr.value * NS, g.y[It.value][Rr.value]); });
        }
    });
}

// ---------------------------------------------------------------- 512 and 1024 points
template <int LOG2N>
struct SmallCfg {
    static constexpr int N = 1 << LOG2N, FPW = 4, TPF = 64, T = FPW * TPF;
    static constexpr int RA = LOG2N == 9 ? 8 : 16, RB = RA, RC = N / (RA * RB);      // 8 8 8 / 16 16 4
    static constexpr int PS = LOG2N == 9 ? 3 : 4;             // one pad element per RA: the strided stores of passes A
    static constexpr int LF = N + (N >> PS);                  // and B meet no bank twice; a frame's image
    static __device__ __forceinline__ int pad(int i) { return i + (i >> PS); }
};
// frame q = row nframes + frame of the call's channels x nframes frames sits in workgroup q / FPW; the last workgroup
// may hold fewer than FPW frames: its idle waves load and store nothing but meet every barrier
template <int LOG2N>
__global__ __launch_bounds__(SmallCfg<LOG2N>::T)
void fft_batch_small_kernel(PlainBatchArgs a)
{
    using Cfg = SmallCfg<LOG2N>;
    constexpr int N = Cfg::N, TPF = Cfg::TPF, RA = Cfg::RA, RB = Cfg::RB, RC = Cfg::RC;
    __shared__ v2f lds[Cfg::FPW * Cfg::LF];
    __shared__ v2f tw[N];                                     // W_N^m: the object's tw1 holds it for N <= 1024
    const int t = threadIdx.x, b = t / TPF, tl = t % TPF;
    for (int i = t; i < N; i += Cfg::T) tw[i] = reinterpret_cast<const v2f *>(a.tw1)[i];
    const long total = (long)a.channels * a.nframes, q = (long)blockIdx.x * Cfg::FPW + b;
    const bool on = q < total;
    const long row = on ? q / a.nframes : 0, frame = on ? q - row * a.nframes : 0;
    const FramePtr p = frame_ptr(a, row, frame, N);
    const float cj = a.sign > 0 ? 1.0f : -1.0f;
    v2f *const my = lds + b * Cfg::LF;
    auto gld = [&](int i) { const v2f s = p.in[i]; return v2f{s.x, cj * s.y}; };
    auto gst = [&](int i, v2f v) { p.out[i] = v2f{v.x, cj * v.y}; };
    auto lld = [&](int i) { return my[Cfg::pad(i)]; };
    auto lst = [&](int i, v2f v) { my[Cfg::pad(i)] = v; };
    {
        SkRegs<RA, N, TPF> g;
        if (on) { sk_load<RA, 1, N, TPF, 1>(tl, tw, g, gld); sk_store<RA, 1, N, TPF>(tl, g, lst); }
    }
    __syncthreads();                                          // (the twiddle table too)
    {
        SkRegs<RB, N, TPF> g;
        if (on) sk_load<RB, RA, N, TPF, 1>(tl, tw, g, lld);
        __syncthreads();
        if (on) sk_store<RB, RA, N, TPF>(tl, g, lst);
    }
    __syncthreads();
    {
        SkRegs<RC, N, TPF> g;                                 // in == out allowed: the frame left global memory in pass A
        if (on) { sk_load<RC, RA * RB, N, TPF, 1>(tl, tw, g, lld); sk_store<RC, RA * RB, N, TPF>(tl, g, gst); }
    }
}

// ---------------------------------------------------------------- 32768 and 65536 points: N = 256 x N2
// 16 transforms side by side in a workgroup of 256 threads: thread t works on transform c = t & 15 as its thread
// tl = t >> 4, so that for every point index the 16 transforms' accesses are neighbours: 128 bytes of global memory,
// and point i of transform c at LDS element 17 i + c (the odd row length lets launch 2's transposing fill, which walks
// i within a row, meet no bank twice).
constexpr int FS_N1 = 256, FS_W = 16, FS_T = 256, FS_TPF = 16, FS_LDS = 256 * 17;

// launch 1: columns n2 = 16 tile + c of frame (row, frame0 + blockIdx.y)
template <int LOG2N>
__global__ __launch_bounds__(FS_T)
void fft_batch_cols_kernel(PlainBatchArgs a, int frame0)
{
    constexpr int N = 1 << LOG2N, N2 = N / FS_N1, L = FS_N1;
    __shared__ v2f lds[FS_LDS];
    __shared__ v2f tw[512];                                   // [256] W_256^m, [256] W_N^m
    const int t = threadIdx.x, c = t & 15, tl = t >> 4;
    for (int i = t; i < 512; i += FS_T) tw[i] = reinterpret_cast<const v2f *>(a.twp)[i];
    const long row = blockIdx.z, fr = blockIdx.y;
    const int n2 = FS_W * blockIdx.x + c;
    const v2f *const in = reinterpret_cast<const v2f *>(a.in) + row * a.in_stride + (frame0 + fr) * (long)N + n2;
    v2f *const wk = reinterpret_cast<v2f *>(a.work) + (row * a.group + fr) * (long)N + n2;
    const float cj = a.sign > 0 ? 1.0f : -1.0f;
    auto gld = [&](int i) { const v2f s = in[(long)i * N2]; return v2f{s.x, cj * s.y}; };
    auto lld = [&](int i) { return lds[17 * i + c]; };
    auto lst = [&](int i, v2f v) { lds[17 * i + c] = v; };
    // bin k1 of the column, times W_N^(n2 k1) = W_N^(256 hi) W_N^lo, to [k1][n2]
    auto gst = [&](int k1, v2f v) {
        const int m = n2 * k1;
        const v2f w = cmul(tw[(m >> 8) * (65536 / N)], tw[256 + (m & 255)]);
        wk[(long)k1 * N2] = cmul(v, w);
    };
    {
        SkRegs<16, L, FS_TPF> g;
        sk_load<16, 1, L, FS_TPF, 1>(tl, tw, g, gld);
        sk_store<16, 1, L, FS_TPF>(tl, g, lst);
    }
    __syncthreads();
    {
        SkRegs<16, L, FS_TPF> g;
        sk_load<16, 16, L, FS_TPF, 1>(tl, tw, g, lld);
        sk_store<16, 16, L, FS_TPF>(tl, g, gst);
    }
}

// launch 2: rows k1 = 16 tile + c of the intermediate of frame (row, frame0 + blockIdx.y)
template <int LOG2N>
__global__ __launch_bounds__(FS_T)
void fft_batch_rows_kernel(PlainBatchArgs a, int frame0)
{
    constexpr int N = 1 << LOG2N, N2 = N / FS_N1, L = N2, TWS = 256 / L;
    constexpr int RB = L / 16;                                // 256 = 16 x 16, 128 = 16 x 8
    __shared__ v2f lds[FS_LDS];
    __shared__ v2f tw[256];                                   // W_256^m
    const int t = threadIdx.x, c = t & 15, tl = t >> 4;
    tw[t] = reinterpret_cast<const v2f *>(a.twp)[t];
    const long row = blockIdx.z, fr = blockIdx.y;
    const int k1_0 = FS_W * blockIdx.x;
    const v2f *const wk = reinterpret_cast<const v2f *>(a.work) + (row * a.group + fr) * (long)N + (long)k1_0 * N2;
    v2f *const out = reinterpret_cast<v2f *>(a.out) + row * a.out_stride + (frame0 + fr) * (long)N + k1_0 + c;
    const float cj = a.sign > 0 ? 1.0f : -1.0f;
    // the 16 rows are one stretch of 16 N2 points: read as it lies, stored transposed
    for (int i = t; i < FS_W * L; i += FS_T) lds[17 * (i % L) + i / L] = wk[i];
    __syncthreads();
    auto lld = [&](int i) { return lds[17 * i + c]; };
    auto lst = [&](int i, v2f v) { lds[17 * i + c] = v; };
    auto gst = [&](int k2, v2f v) { out[(long)k2 * FS_N1] = v2f{v.x, cj * v.y}; };
    {
        SkRegs<16, L, FS_TPF> g;
        sk_load<16, 1, L, FS_TPF, TWS>(tl, tw, g, lld);
        __syncthreads();
        sk_store<16, 1, L, FS_TPF>(tl, g, lst);
    }
    __syncthreads();
    {
        SkRegs<RB, L, FS_TPF> g;
        sk_load<RB, 16, L, FS_TPF, TWS>(tl, tw, g, lld);
        sk_store<RB, 16, L, FS_TPF>(tl, g, gst);
    }
}

// ---------------------------------------------------------------- launchers
template <int LOG2N>
static hipError_t mid_launch(const PlainBatchArgs &a, hipStream_t s)
{
    using Cfg = SpecCfg<LOG2N>;
    const hipError_t e = CSDR_MAX_LDS_ONCE((&fft_batch_plain_kernel<LOG2N>), Cfg::LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fft_batch_plain_kernel<LOG2N>, dim3((unsigned)((long)a.channels * a.nframes)), dim3(Cfg::T),
                       Cfg::LDS_BYTES, s, a);
    return hipGetLastError();
}
template <int LOG2N>
static hipError_t small_launch(const PlainBatchArgs &a, hipStream_t s)
{
    using Cfg = SmallCfg<LOG2N>;
    const long total = (long)a.channels * a.nframes;
    hipLaunchKernelGGL(fft_batch_small_kernel<LOG2N>, dim3((unsigned)((total + Cfg::FPW - 1) / Cfg::FPW)), dim3(Cfg::T), 0, s, a);
    return hipGetLastError();
}
// the work buffer holds a.group frames of every row: the call's frames go through it in groups, in stream order
template <int LOG2N>
static hipError_t four_step_launch(const PlainBatchArgs &a, hipStream_t s)
{
    constexpr int N2 = (1 << LOG2N) / FS_N1;
    if (!a.work || !a.twp || a.group < 1 || a.channels > 65535) return hipErrorInvalidValue;
    for (int f0 = 0; f0 < a.nframes; f0 += a.group) {
        const int nf = a.nframes - f0 < a.group ? a.nframes - f0 : a.group;
        hipLaunchKernelGGL(fft_batch_cols_kernel<LOG2N>, dim3(N2 / FS_W, nf, a.channels), dim3(FS_T), 0, s, a, f0);
        hipLaunchKernelGGL(fft_batch_rows_kernel<LOG2N>, dim3(FS_N1 / FS_W, nf, a.channels), dim3(FS_T), 0, s, a, f0);
    }
    return hipGetLastError();
}

hipError_t fft_batch_plain_launch(int log2n, const PlainBatchArgs &a, hipStream_t stream)
{
    if (a.channels < 1 || a.nframes < 1 || (long)a.channels * a.nframes > 0x7fffffffl) return hipErrorInvalidValue;
    switch (log2n) {
    case 9: return small_launch<9>(a, stream);
    case 10: return small_launch<10>(a, stream);
    case 11: return mid_launch<11>(a, stream);
    case 12: return mid_launch<12>(a, stream);
    case 13: return mid_launch<13>(a, stream);
    case 14: return mid_launch<14>(a, stream);
    case 15: return four_step_launch<15>(a, stream);
    case 16: return four_step_launch<16>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace csdr
