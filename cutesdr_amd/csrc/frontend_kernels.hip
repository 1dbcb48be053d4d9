// frontend_kernels.hip -- the input-rate stages in front of the down-converter beside the noise blanker
// (noiseblank_kernels.hip): SURVEY 8(f) f2.
//
// unpack_kernel replaces the datagram conversion loops of CUdpThread::OnreadyRead
// (interface/netiobase.cpp:497-503, 521-526); spurcal_kernel the running I/Q means of
// CSdrInterface::NcoSpurCalibrate (interface/sdrinterface.cpp:829-848).
#include "frontend_kernels.h"

namespace csdr {

typedef float f2 __attribute__((ext_vector_type(2)));

// ---------------- wire format -> complex fp32 ----------------
// A thread converts two consecutive samples of a datagram with aligned 32-bit loads (datagram
// lengths, the 4-byte header and a sample pair -- 12 or 8 bytes -- are all multiples of 4) and one
// 16-byte store.
__global__ void unpack_kernel(const unsigned char *pk, long chan_stride, int npackets, int pkt_len, int per,
                              float *out, long out_stride, const double *dc)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;        // sample pair within the channel
    const int ch = blockIdx.y;
    const int half = per / 2;
    if (p >= (long)npackets * half) return;
    const long q = p / half;
    const int j = (int)(p - q * half);
    const unsigned *w = reinterpret_cast<const unsigned *>(pk + (long)ch * chan_stride + q * pkt_len + 4);
    const wf4 raw = pkt_len == 1444 ? wf4{__uint_as_float(w[3 * j]), __uint_as_float(w[3 * j + 1]), __uint_as_float(w[3 * j + 2]), 0.f}
                                    : wf4{__uint_as_float(w[2 * j]), __uint_as_float(w[2 * j + 1]), 0.f, 0.f};
    const wf4 x = wire_pair_decode(raw, pkt_len);
    float v[4] = {x.x, x.y, x.z, x.w};
    if (dc) {
        const double di = dc[2 * ch], dq = dc[2 * ch + 1];
        v[0] = (float)((double)v[0] - di); v[1] = (float)((double)v[1] - dq);
        v[2] = (float)((double)v[2] - di); v[3] = (float)((double)v[3] - dq);
    }
    float4 *o = reinterpret_cast<float4 *>(out + 2 * ((long)ch * out_stride + q * per + 2 * j));
    *o = make_float4(v[0], v[1], v[2], v[3]);
}

hipError_t unpack_launch(const unsigned char *pk, long chan_stride_bytes, int channels, int npackets, int pkt_len,
                         float *out, long out_stride, const double *dc, hipStream_t stream)
{
    const int per = pkt_len == 1444 ? 240 : 256;
    const long tot = (long)npackets * (per / 2);
    if (tot == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((tot + 255) / 256), channels), dim3(256), 0, stream,
                       pk, chan_stride_bytes, npackets, pkt_len, per, out, out_stride, dc);
    return hipGetLastError();
}

// ---------------- NCO spur (DC) estimate ----------------
// y_n = (1-a)^n y_0 + a * sum_k (1-a)^(n-1-k) x_k : a weighted reduction, one workgroup per channel.
// The sample source is a template input: fp32 rows (spurcal_kernel) or datagrams decoded in the load
// (spurcal_packets_kernel); a decoded value is exact in fp32, so both give the same doubles for the same samples.
template <class Load>
__device__ __forceinline__ void spurcal_body(Load x, int n, double *dc)
{
    __shared__ double red[2][256];
    const int ch = blockIdx.x, t = threadIdx.x;
    const double a = 1.0 / 100000.0, l1 = log1p(-a);
    double si = 0.0, sq = 0.0;
    for (long k = t; k < n; k += 256) {
        const double wgt = exp(l1 * (double)(n - 1 - k));
        const f2 v = x(k);
        si += wgt * (double)v.x; sq += wgt * (double)v.y;
    }
    red[0][t] = si; red[1][t] = sq;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { red[0][t] += red[0][t + s]; red[1][t] += red[1][t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        const double decay = exp(l1 * (double)n);
        dc[2 * ch] = decay * dc[2 * ch] + a * red[0][0];
        dc[2 * ch + 1] = decay * dc[2 * ch + 1] + a * red[1][0];
    }
}
__global__ __launch_bounds__(256)
void spurcal_kernel(const float *iq, long in_stride, int n, double *dc)
{
    const f2 *x = reinterpret_cast<const f2 *>(iq) + (long)blockIdx.x * in_stride;
    spurcal_body([&](long k) { return x[k]; }, n, dc);
}
__global__ __launch_bounds__(256)
void spurcal_packets_kernel(WireIn w, int n, double *dc)
{
    const unsigned char *chan = w.pk + (long)blockIdx.x * w.chan_stride;
    spurcal_body([&](long k) { const wf2 v = wire_sample(chan, w.pkt_len, k); return f2{v.x, v.y}; }, n, dc);
}

hipError_t spurcal_launch(const float *iq, long in_stride, int channels, int n, double *dc, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(spurcal_kernel, dim3(channels), dim3(256), 0, stream, iq, in_stride, n, dc);
    return hipGetLastError();
}
hipError_t spurcal_packets_launch(const unsigned char *pk, int channels, int npackets, int pkt_len, double *dc,
                                  hipStream_t stream)
{
    const int per = pkt_len == 1444 ? 240 : 256;
    const int n = npackets * per;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(spurcal_packets_kernel, dim3(channels), dim3(256), 0, stream,
                       WireIn{pk, (long)npackets * pkt_len, pkt_len, per}, n, dc);
    return hipGetLastError();
}

}  // namespace csdr
