// spurcal_host.hpp -- the NCO-spur bookkeeping of CSdrInterface (reference interface/sdrinterface.cpp:791-824
// ManageNCOSpurOffsets, :829-848 NcoSpurCalibrate, :886-887 its caller) as functions for host and device, so that the
// rule exists once: K13 (spurcal_kernels.hip) and the hooks the CPU tests call (capi_hosttest.hip) evaluate the same text.
//
// Per receiver the state is {m_NCOSpurOffsetI, m_NCOSpurOffsetQ} (two doubles, the [channels][2] layout every d_dc
// argument of the library has) and {m_NcoSpurCalCount, m_NcoSpurCalActive} (Rec).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace csdr {
namespace spur {

constexpr int kMaxSamples = 300000;      // SPUR_CAL_MAXSAMPLES, sdrinterface.cpp:47
constexpr double kAlpha = 1.0 / 100000.0;                  // :837, :839
constexpr double kKeep = 1.0 - 1.0 / 100000.0;

struct Rec {
    int count;                           // m_NcoSpurCalCount
    int active;                          // m_NcoSpurCalActive
};

enum { CMD_SET = 0, CMD_STARTCAL = 1, CMD_READ = 2 };      // eNCOSPURCMD, sdrinterface.h:45-49

// ManageNCOSpurOffsets (:791-824) on one receiver; a READ's values are what off[] holds afterwards
__host__ __device__ inline void spurcal_command(int cmd, double vi, double vq, double *off, Rec *r)
{
    r->active = 0;                                         // :793, whatever the command
    if (cmd == CMD_SET) { off[0] = vi; off[1] = vq; }      // :799-800
    else if (cmd == CMD_STARTCAL) {
        if (off[0] > 10.0 || off[0] < -10.0) off[0] = 0.0; // :805-806
        if (off[1] > 10.0 || off[1] < -10.0) off[1] = 0.0; // :807-808
        r->count = 0;                                      // :809
        r->active = 1;                                     // :810
    }
}

// What n complex samples do that arrive as reference calls of call_len samples each (one datagram: 240 or 256), the
// last one possibly short.  A call does nothing on an inactive receiver (:886); on an active one with count >=
// kMaxSamples it clears `active` and nothing else (:843-847); otherwise the recurrence runs over all of it and count
// grows by Length / 4 with Length = 2 * samples (:831-841).
struct Put {
    int calls;                           // the first `calls` calls run the recurrence ...
    int samples;                         // ... which are the first `samples` samples
    int count, active;                   // the record afterwards
};
__host__ __device__ inline Put spurcal_put(int count, int active, int n, int call_len)
{
    Put p{0, 0, count, active};
    if (!active || n <= 0) return p;
    if (count >= kMaxSamples) { p.active = 0; return p; }
    const int ncalls = (n - 1) / call_len + 1;
    const int q = call_len / 2;                            // (2 * call_len) / 4 without the product
    const int room = kMaxSamples - count;
    const int u = q > 0 && (room + q - 1) / q < ncalls ? (room + q - 1) / q : ncalls;
    p.calls = u;
    if (u < ncalls) {                                      // call u meets count >= kMaxSamples
        p.samples = u * call_len; p.count = count + u * q; p.active = 0;
    } else {                                               // ends with the put: active stays until the next call
        const int r = n - (ncalls - 1) * call_len;
        p.samples = n; p.count = count + (ncalls - 1) * q + r / 2;
    }
    return p;
}

// (1 - a)^len, what a stretch of len samples leaves of the value in front of it: one exp per stretch length
__host__ __device__ inline double spurcal_pow(long long len) { return exp((double)len * log1p(-kAlpha)); }

}  // namespace spur
}  // namespace csdr
