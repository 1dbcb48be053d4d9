// display_stream_kernels.hip -- the display path of CSdrInterface::ProcessIQData (reference
// interface/sdrinterface.cpp:889-907) in front of the display spectrum: the DC correction of m_DataBuf, the frame carry
// across calls, and the frames the skip counter and the screen gate select (display_plan.hpp).
//
// display_gather_kernel reads ONLY the selected frames -- from the carry, from fp32 rows or straight from the radio's
// datagrams (wire_format.hpp) -- and writes them DC-corrected, back to back, for the existing spectrum kernels
// (spectrum_kernels.hip, unchanged).  display_carry_kernel keeps the partial frame at the end of the call.  At the
// typical skip value (48 at 2 MS/s, 4096 points, 10 updates/s) a call reads about 1/48 of its input.
//
// BLK: the kernels behind a blanked chain call (StreamSrc::nb_mask): the sample comes from delay_n + 1 behind -- out of
// the blanker's history when that lies in front of the call -- and is zero under the mask.  Kernels of their own, chosen
// by the launchers: the plain ones keep their code.
#include "display_stream_kernels.h"

namespace csdr {

typedef float v2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2s stream_raw(const StreamSrc &a, int ch, long s)
{
    if (a.wire.pk) return wire_sample(a.wire.pk + (long)ch * a.wire.chan_stride, a.wire.pkt_len, s);
    return reinterpret_cast<const v2s *>(a.in)[(long)ch * a.in_stride + s];
}

template <bool BLK>
__device__ __forceinline__ v2s stream_sample(const StreamSrc &a, int ch, long s)
{
    if (s < 0) return reinterpret_cast<const v2s *>(a.carry)[(long)ch * a.carry_stride + a.pos + s];
    v2s v;
    if constexpr (BLK) {
        const NbChan *nb = a.nb_state + ch;
        const int on = nb->on;
        const long j = on ? s - nb->delay_n - 1 : s;
        if (on && ((a.nb_mask[(long)ch * a.nb_mask_stride + (s >> 5)] >> (s & 31)) & 1u)) v = v2s{0.f, 0.f};
        else if (j < 0) v = reinterpret_cast<const v2s *>(a.nb_hist)[(long)ch * NB_HIST + NB_HIST + j];   // j >= -NB_MAX_WIDTH / 2 - 1
        else v = stream_raw(a, ch, j);
    } else if (a.wire.pk) v = wire_sample(a.wire.pk + (long)ch * a.wire.chan_stride, a.wire.pkt_len, s);
    else v = reinterpret_cast<const v2s *>(a.in)[(long)ch * a.in_stride + s];
    if (a.dc)                                                          // sdrinterface.cpp:891-894, as unpack_kernel
        v = v2s{(float)((double)v.x - a.dc[2 * ch]), (float)((double)v.y - a.dc[2 * ch + 1])};
    return v;
}

template <bool BLK>
__global__ __launch_bounds__(256)
void display_gather_kernel(StreamSrc a, long start, long step, long total, int log2n, float *out)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;         // sample j of the channel's used frames
    const int ch = blockIdx.y;
    if (j >= total) return;
    const long k = j >> log2n, i = j & ((1l << log2n) - 1);
    reinterpret_cast<v2s *>(out)[(long)ch * total + j] = stream_sample<BLK>(a, ch, start + k * step + i);
}

// the row form: entry e of the table gathers ITS frames (start, step and count of its own) into out[row][...]; a row
// without a frame is in no table and its staging row is not touched
template <bool BLK>
__global__ __launch_bounds__(256)
void display_gather_rows_kernel(StreamSrc a, const SpecRow *rows, int log2n, float *out, long out_stride)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const SpecRow e = rows[blockIdx.y];
    if (j >= ((long)e.nframes << log2n)) return;
    const long k = j >> log2n, i = j & ((1l << log2n) - 1);
    reinterpret_cast<v2s *>(out)[(long)e.row * out_stride + j] = stream_sample<BLK>(a, e.row, (long)e.start + k * (long)e.step + i);
}

template <bool BLK>
__global__ __launch_bounds__(256)
void display_carry_kernel(StreamSrc a, float *carry, int dst, long src, int len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = blockIdx.y;
    if (i >= len) return;
    reinterpret_cast<v2s *>(carry)[(long)ch * a.carry_stride + dst + i] = stream_sample<BLK>(a, ch, src + i);
}

hipError_t display_gather_launch(const StreamSrc &a, long long start, long long step, int count, int N, float *out,
                                 hipStream_t stream)
{
    int l2 = 0;
    while ((1 << l2) < N) l2++;
    const long total = (long)count * N;
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned)((total + 255) / 256), a.channels);
    if (a.nb_mask)
        hipLaunchKernelGGL(display_gather_kernel<true>, grid, dim3(256), 0, stream, a, (long)start, (long)step, total, l2, out);
    else
        hipLaunchKernelGGL(display_gather_kernel<false>, grid, dim3(256), 0, stream, a, (long)start, (long)step, total, l2, out);
    return hipGetLastError();
}

hipError_t display_gather_rows_launch(const StreamSrc &a, const SpecRow *d_rows, int nrows, int max_count, int N, float *out,
                                      hipStream_t stream)
{
    int l2 = 0;
    while ((1 << l2) < N) l2++;
    const long total = (long)max_count * N;
    if (total == 0 || nrows == 0) return hipSuccess;
    const dim3 grid((unsigned)((total + 255) / 256), nrows);
    if (a.nb_mask)
        hipLaunchKernelGGL(display_gather_rows_kernel<true>, grid, dim3(256), 0, stream, a, d_rows, l2, out, total);
    else
        hipLaunchKernelGGL(display_gather_rows_kernel<false>, grid, dim3(256), 0, stream, a, d_rows, l2, out, total);
    return hipGetLastError();
}

hipError_t display_carry_launch(const StreamSrc &a, float *carry, int dst, long long src, int len, hipStream_t stream)
{
    if (len <= 0) return hipSuccess;
    const dim3 grid((unsigned)((len + 255) / 256), a.channels);
    if (a.nb_mask)
        hipLaunchKernelGGL(display_carry_kernel<true>, grid, dim3(256), 0, stream, a, carry, dst, (long)src, len);
    else
        hipLaunchKernelGGL(display_carry_kernel<false>, grid, dim3(256), 0, stream, a, carry, dst, (long)src, len);
    return hipGetLastError();
}

}  // namespace csdr
