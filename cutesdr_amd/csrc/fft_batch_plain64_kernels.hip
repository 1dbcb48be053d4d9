// fft_batch_plain64_kernels.hip -- K3q: CFft::FwdFFT / RevFFT (dsp/fft.cpp:416-426) of many frames of many rows in the
// reference's own precision (TYPECPX = two doubles): csdr_fft_batch_fwd_f64 / _rev_f64.  The fp64 sibling of
// fft_batch_plain_kernels.hip; nothing of the display state is touched.
//
//   512 ... 4096 points     a frame is one LDS image of N + N / RA 16-byte elements (36 KB for four frames at 512 points,
//                           68 KB per workgroup above: two workgroups per CU); 256 threads work on 4 / 4 / 2 / 1 frames;
//                           three Stockham passes (8 8 8 / 16 16 4 / 16 16 8 / 16 16 16), the first read from and the
//                           last written to global memory directly
//   8192 ... 65536 points   a frame's image alone would take 128 KB and more, one workgroup per CU: the four-step form
//                           N = N1 x N2 (64 x 128, 128 x 128, 256 x 128, 256 x 256) in two launches: (1) per workgroup 16
//                           neighbouring columns n2 of the N1 x N2 input matrix: N1-point transforms over n1, times
//                           W_N^(n2 k1), to the work buffer as [k1][n2]; (2) per workgroup 16 neighbouring rows k1 of it:
//                           N2-point transforms over n2, bin k1 + N1 k2 out.  Every global access of a 16-lane group is a
//                           256-byte stretch.
//
// The negative exponent (RevFFT) is the positive one on conjugated input, conjugated again on the way out.  Every pass
// twiddle is an entry of a table built in long double on the host (fft_tw64_host.hpp); W_N^(n2 k1) is the product of
// two entries, W_N^(256 hi) W_N^lo; the butterflies' own W_16^k are literals.  No fp32 value and no device sincos.
#include "launch_once.hpp"
#include "fft_plain64_passes.hpp"
#include "fft_batch_plain64_kernels.h"

namespace csdr {

struct FramePtr64 { const v2d *in; v2d *out; };
__device__ __forceinline__ FramePtr64 frame_ptr64(const PlainBatch64Args &a, long row, long frame, int n)
{
    return FramePtr64{reinterpret_cast<const v2d *>(a.in) + row * a.in_stride + frame * n,
                      reinterpret_cast<v2d *>(a.out) + row * a.out_stride + frame * n};
}

// ---------------------------------------------------------------- 512 ... 4096 points
// frame q = row nframes + frame of the call's channels x nframes frames sits in workgroup q / FPW; the last workgroup
// may hold fewer than FPW frames: its idle waves load and store nothing but meet every barrier
template <int LOG2N>
__global__ __launch_bounds__(Small64Cfg<LOG2N>::T)
void fft_batch64_small_kernel(PlainBatch64Args a)
{
    using Cfg = Small64Cfg<LOG2N>;
    constexpr int N = Cfg::N, TPF = Cfg::TPF, RA = Cfg::RA, RB = Cfg::RB, RC = Cfg::RC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2d *lds = reinterpret_cast<v2d *>(smem_raw);
    const v2d *tw = reinterpret_cast<const v2d *>(a.tw);      // W_N^m, read where it lies (64 KB at 4096 points)
    const int t = threadIdx.x, b = t / TPF, tl = t % TPF;
    const long total = (long)a.channels * a.nframes, q = (long)blockIdx.x * Cfg::FPW + b;
    const bool on = q < total;
    const long row = on ? q / a.nframes : 0, frame = on ? q - row * a.nframes : 0;
    const FramePtr64 p = frame_ptr64(a, row, frame, N);
    const double cj = a.sign > 0 ? 1.0 : -1.0;
    v2d *const my = lds + b * Cfg::LF;
    auto gld = [&](int i) { const v2d s = p.in[i]; return v2d{s.x, cj * s.y}; };
    auto gst = [&](int i, v2d v) { p.out[i] = v2d{v.x, cj * v.y}; };
    auto lld = [&](int i) { return my[Cfg::pad(i)]; };
    auto lst = [&](int i, v2d v) { my[Cfg::pad(i)] = v; };
    {
        SkRegs64<RA, N, TPF> g;
        if (on) { sk_load64<RA, 1, N, TPF, 1>(tl, tw, g, gld); sk_store64<RA, 1, N, TPF>(tl, g, lst); }
    }
    __syncthreads();
    {
        SkRegs64<RB, N, TPF> g;
        if (on) sk_load64<RB, RA, N, TPF, 1>(tl, tw, g, lld);
        __syncthreads();
        if (on) sk_store64<RB, RA, N, TPF>(tl, g, lst);
    }
    __syncthreads();
    {
        SkRegs64<RC, N, TPF> g;                               // in == out allowed: the frame left global memory in pass A
        if (on) { sk_load64<RC, RA * RB, N, TPF, 1>(tl, tw, g, lld); sk_store64<RC, RA * RB, N, TPF>(tl, g, gst); }
    }
}

// ---------------------------------------------------------------- 8192 ... 65536 points: N = N1 x N2
// 16 transforms side by side in a workgroup of 256 threads: thread t works on transform c = t & 15 as its thread
// tl = t >> 4, so that for every point index the 16 transforms' accesses are neighbours: 256 bytes of global memory,
// and point i of transform c at LDS element 17 i + c.  The odd row length lets launch 2's transposing fill, which walks
// i within a row, store eight neighbouring lanes 68 dwords apart: 4 j mod 32, eight different 4-bank quarters.

// launch 1: columns n2 = 16 tile + c of frame (row, frame0 + blockIdx.y)
template <int LOG2N>
__global__ __launch_bounds__(Four64Cfg<LOG2N>::T)
void fft_batch64_cols_kernel(PlainBatch64Args a, int frame0)
{
    using Cfg = Four64Cfg<LOG2N>;
    constexpr int N = Cfg::N, N2 = Cfg::N2, L = Cfg::N1, TPF = Cfg::TPF, TWS = 256 / L;
    constexpr int RA = Cfg::ra(L), RB = L / RA;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2d *lds = reinterpret_cast<v2d *>(smem_raw);
    v2d *tw = lds + 17 * L;                                   // [256] W_256^m, [256] W_N^m
    const int t = threadIdx.x, c = t & 15, tl = t >> 4;
    for (int i = t; i < 512; i += Cfg::T) tw[i] = reinterpret_cast<const v2d *>(a.tw)[i];
    const long row = blockIdx.z, fr = blockIdx.y;
    const int n2 = Cfg::W * blockIdx.x + c;
    const v2d *const in = reinterpret_cast<const v2d *>(a.in) + row * a.in_stride + (frame0 + fr) * (long)N + n2;
    v2d *const wk = reinterpret_cast<v2d *>(a.work) + (row * a.group + fr) * (long)N + n2;
    const double cj = a.sign > 0 ? 1.0 : -1.0;
    auto gld = [&](int i) { const v2d s = in[(long)i * N2]; return v2d{s.x, cj * s.y}; };
    auto lld = [&](int i) { return lds[17 * i + c]; };
    auto lst = [&](int i, v2d v) { lds[17 * i + c] = v; };
    // bin k1 of the column, times W_N^(n2 k1) = W_N^(256 hi) W_N^lo, to [k1][n2]
    auto gst = [&](int k1, v2d v) {
        const int m = n2 * k1;
        const v2d w = cmul64(tw[(m >> 8) * (65536 / N)], tw[256 + (m & 255)]);
        wk[(long)k1 * N2] = cmul64(v, w);
    };
    {
        SkRegs64<RA, L, TPF> g;
        sk_load64<RA, 1, L, TPF, TWS>(tl, tw, g, gld);
        sk_store64<RA, 1, L, TPF>(tl, g, lst);
    }
    __syncthreads();                                          // (the twiddle tables too)
    {
        SkRegs64<RB, L, TPF> g;
        sk_load64<RB, RA, L, TPF, TWS>(tl, tw, g, lld);
        sk_store64<RB, RA, L, TPF>(tl, g, gst);
    }
}

// launch 2: rows k1 = 16 tile + c of the intermediate of frame (row, frame0 + blockIdx.y)
template <int LOG2N>
__global__ __launch_bounds__(Four64Cfg<LOG2N>::T)
void fft_batch64_rows_kernel(PlainBatch64Args a, int frame0)
{
    using Cfg = Four64Cfg<LOG2N>;
    constexpr int N = Cfg::N, N1 = Cfg::N1, L = Cfg::N2, TPF = Cfg::TPF, TWS = 256 / L;
    constexpr int RA = Cfg::ra(L), RB = L / RA;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2d *lds = reinterpret_cast<v2d *>(smem_raw);
    v2d *tw = lds + 17 * L;                                   // W_256^m
    const int t = threadIdx.x, c = t & 15, tl = t >> 4;
    tw[t] = reinterpret_cast<const v2d *>(a.tw)[t];
    const long row = blockIdx.z, fr = blockIdx.y;
    const int k1_0 = Cfg::W * blockIdx.x;
    const v2d *const wk = reinterpret_cast<const v2d *>(a.work) + (row * a.group + fr) * (long)N + (long)k1_0 * L;
    v2d *const out = reinterpret_cast<v2d *>(a.out) + row * a.out_stride + (frame0 + fr) * (long)N + k1_0 + c;
    const double cj = a.sign > 0 ? 1.0 : -1.0;
    // the 16 rows are one stretch of 16 N2 points: read as it lies, stored transposed
    for (int i = t; i < Cfg::W * L; i += Cfg::T) lds[17 * (i % L) + i / L] = wk[i];
    __syncthreads();
    auto lld = [&](int i) { return lds[17 * i + c]; };
    auto lst = [&](int i, v2d v) { lds[17 * i + c] = v; };
    auto gst = [&](int k2, v2d v) { out[(long)k2 * N1] = v2d{v.x, cj * v.y}; };
    {
        SkRegs64<RA, L, TPF> g;
        sk_load64<RA, 1, L, TPF, TWS>(tl, tw, g, lld);
        __syncthreads();
        sk_store64<RA, 1, L, TPF>(tl, g, lst);
    }
    __syncthreads();
    {
        SkRegs64<RB, L, TPF> g;
        sk_load64<RB, RA, L, TPF, TWS>(tl, tw, g, lld);
        sk_store64<RB, RA, L, TPF>(tl, g, gst);
    }
}

// ---------------------------------------------------------------- launchers
template <int LOG2N>
static hipError_t small64_launch(const PlainBatch64Args &a, hipStream_t s)
{
    using Cfg = Small64Cfg<LOG2N>;
    const hipError_t e = CSDR_MAX_LDS_ONCE((&fft_batch64_small_kernel<LOG2N>), Cfg::LDS_BYTES);
    if (e != hipSuccess) return e;
    const long total = (long)a.channels * a.nframes;
    hipLaunchKernelGGL(fft_batch64_small_kernel<LOG2N>, dim3((unsigned)((total + Cfg::FPW - 1) / Cfg::FPW)), dim3(Cfg::T),
                       Cfg::LDS_BYTES, s, a);
    return hipGetLastError();
}
// the work buffer holds a.group frames of every row: the call's frames go through it in groups, in stream order
template <int LOG2N>
static hipError_t four_step64_launch(const PlainBatch64Args &a, hipStream_t s)
{
    using Cfg = Four64Cfg<LOG2N>;
    if (!a.work || a.group < 1 || a.channels > 65535) return hipErrorInvalidValue;
    hipError_t e = CSDR_MAX_LDS_ONCE((&fft_batch64_cols_kernel<LOG2N>), Cfg::COLS_LDS);
    if (e == hipSuccess) e = CSDR_MAX_LDS_ONCE((&fft_batch64_rows_kernel<LOG2N>), Cfg::ROWS_LDS);
    if (e != hipSuccess) return e;
    for (int f0 = 0; f0 < a.nframes; f0 += a.group) {
        const int nf = a.nframes - f0 < a.group ? a.nframes - f0 : a.group;
        hipLaunchKernelGGL(fft_batch64_cols_kernel<LOG2N>, dim3(Cfg::N2 / Cfg::W, nf, a.channels), dim3(Cfg::T), Cfg::COLS_LDS, s, a, f0);
        hipLaunchKernelGGL(fft_batch64_rows_kernel<LOG2N>, dim3(Cfg::N1 / Cfg::W, nf, a.channels), dim3(Cfg::T), Cfg::ROWS_LDS, s, a, f0);
    }
    return hipGetLastError();
}

hipError_t fft_batch_plain64_launch(int log2n, const PlainBatch64Args &a, hipStream_t stream)
{
    if (!a.tw || a.channels < 1 || a.nframes < 1 || (long)a.channels * a.nframes > 0x7fffffffl) return hipErrorInvalidValue;
    switch (log2n) {
    case 9: return small64_launch<9>(a, stream);
    case 10: return small64_launch<10>(a, stream);
    case 11: return small64_launch<11>(a, stream);
    case 12: return small64_launch<12>(a, stream);
    case 13: return four_step64_launch<13>(a, stream);
    case 14: return four_step64_launch<14>(a, stream);
    case 15: return four_step64_launch<15>(a, stream);
    case 16: return four_step64_launch<16>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace csdr
