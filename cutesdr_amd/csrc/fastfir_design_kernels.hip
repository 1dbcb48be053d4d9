// fastfir_design_kernels.hip -- CFastFIR::SetupParameters (dsp/fastfir.cpp:178-259) for many filters in one launch:
// one workgroup per job, everything in fp64.  The job carries the two normalised doubles the host derives from the edges
// (host_math.hpp: fastfir_design_job; the reference's sanity check stays there).  The workgroup
//   1. computes the N/2+1 taps -- windowed sinc times the pass-band shift, scaled by 1/N; the Blackman-Nuttall window
//      comes from a table (the host's fastfir_window), so three transcendentals per tap are the device library's --
//      and stores them zero padded in bit-reversed order,
//   2. transforms them with host_fft's own network (radix-2 decimation in time, sign +1) and a twiddle table of nearest
//      doubles (host_math.hpp: design_twiddles), every product and sum rounded on its own (no contraction into fused
//      multiply-adds: the response is then the same words whatever the compiler, and a plain fp64 model of the network
//      reproduces it),
//   3. writes the fp32 response in the generic and in the pipelined overlap-save kernel's register order (permutation
//      tables), its real gains Re(H[k] (-j)^k) in the 16384-point kernel's order, and the fp64 response in natural order
//      (the row get_response reads).
// N = 2048 / 4096 / 8192: the transform lives in LDS as complex fp64 (32 / 64 / 128 KB); N = 16384 would need 256 KB, so
// that size works in its fp64 response row in device memory (L2 resident, workgroup barriers between the stages).
// Control plane: one launch per process call at most.  Nothing here is tuned beyond keeping consecutive lanes on
// consecutive 16-byte elements from the stage of half = 64 on; the bit-reversed tap store and the first stages are bank
// conflicted in LDS (uncoalesced in device memory at N = 16384).  Measured times: HISTORY.md.
#include "fastfir_design_kernels.h"
#include "launch_once.hpp"

namespace csdr {

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v2f_d __attribute__((ext_vector_type(2)));

constexpr double kPiD = 3.14159265358979323846;      // K_2PI / 2, dsp/datatypes.h:44
constexpr double kTwoPiD = 2.0 * kPiD;

template <int LOG2N>
struct DesignCfg {
    static constexpr int N = 1 << LOG2N;
    static constexpr bool IN_LDS = LOG2N <= 13;
    static constexpr int T = N / 8 > 1024 ? 1024 : N / 8;          // 256, 512, 1024, 1024 threads
    static constexpr int LDS_BYTES = IN_LDS ? N * 16 : 0;
};

template <int LOG2N>
__global__ __launch_bounds__(DesignCfg<LOG2N>::T) void fastfir_design_kernel(DesignArgs a)
{
#pragma clang fp contract(off)
    using Cfg = DesignCfg<LOG2N>;
    constexpr int N = Cfg::N, T = Cfg::T, P = N / 2 + 1, CENTRE = N / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char design_smem[];
    const DesignJob job = a.jobs[blockIdx.x];
    const int tid = threadIdx.x;
    v2d *row = reinterpret_cast<v2d *>(a.resp) + (size_t)job.slot * N;
    v2d *w;
    if constexpr (Cfg::IN_LDS) w = reinterpret_cast<v2d *>(design_smem);
    else w = row;

    // ---- taps (fastfir.cpp:212-236), zero padded, into host_fft's bit-reversed start order
    for (int i = tid; i < N; i += T) {
        v2d v = {0.0, 0.0};
        if (i < P) {
            const double x = (double)(i - CENTRE);
            double z;
            if (i == CENTRE) z = 2.0 * job.nfc;
            else z = sin(kTwoPiD * x * job.nfc) / (kPiD * x) * a.win[i];
            v.x = z * cos(job.nfs * x) / (double)N;
            v.y = z * sin(job.nfs * x) / (double)N;
        }
        w[__brev((unsigned)i) >> (32 - LOG2N)] = v;
    }
    __syncthreads();

    // ---- host_fft(H, +1): stage s joins blocks of len = 2^s; butterfly q of a stage touches only its own two elements
#pragma unroll 1
    for (int s = 1; s <= LOG2N; s++) {
        const int half = 1 << (s - 1);
        for (int q = tid; q < N / 2; q += T) {
            const int k = q & (half - 1);
            const int b = ((q - k) << 1) + k;
            const int j = k << (LOG2N - s);
            const double wr = a.tw[2 * j], wi = a.tw[2 * j + 1];
            const v2d u = w[b], x = w[b + half];
            v2d v;
            v.x = x.x * wr - x.y * wi;
            v.y = x.x * wi + x.y * wr;
            w[b] = u + v;
            w[b + half] = u - v;
        }
        __syncthreads();
    }

    // ---- the three forms of the response
    v2f_d *h = reinterpret_cast<v2f_d *>(a.h) + (size_t)job.slot * N;
    v2f_d *h2 = reinterpret_cast<v2f_d *>(a.h2) + (size_t)job.slot * N;
    float *gain = a.gain + (size_t)job.slot * N;
    for (int i = tid; i < N; i += T) {
        const v2d p = w[a.perm[i]], p2 = w[a.perm2[i]];
        v2f_d f = {(float)p.x, (float)p.y}, f2 = {(float)p2.x, (float)p2.y};
        h[i] = f;
        h2[i] = f2;
        // the real gain of the linear-phase response, Re(H[k] (-j)^k): the component of H[k] that k mod 4 selects
        const int kg = a.permg[i];
        const v2d pg = w[kg];
        const double gr = (kg & 1) ? pg.y : pg.x;
        gain[i] = (float)((kg & 2) ? -gr : gr);
        if constexpr (Cfg::IN_LDS) row[i] = w[i];
    }
}

template <int LOG2N>
hipError_t launch_one(const DesignArgs &a, int njobs, hipStream_t stream)
{
    using Cfg = DesignCfg<LOG2N>;
    if (Cfg::LDS_BYTES > 0) {      // once per device (launch_once.hpp)
        hipError_t e = CSDR_MAX_LDS_ONCE((&fastfir_design_kernel<LOG2N>), Cfg::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((fastfir_design_kernel<LOG2N>), dim3(njobs), dim3(Cfg::T), Cfg::LDS_BYTES, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t fastfir_design_launch(int log2n, const DesignArgs &a, int njobs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    switch (log2n) {
    case 11: return launch_one<11>(a, njobs, stream);
    case 12: return launch_one<12>(a, njobs, stream);
    case 13: return launch_one<13>(a, njobs, stream);
    case 14: return launch_one<14>(a, njobs, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace csdr
