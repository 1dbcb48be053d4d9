// seqcheck_kernels.hip -- K12: the datagram sequence check.  C independent copies of CUdpThread::OnreadyRead's
// bookkeeping (reference interface/netiobase.cpp:484-496 / :509-521; the rule itself is seq_host.hpp's seq_step), one
// workgroup per receiver, one launch per put.
//
// The rule is no recurrence: after any datagram m_LastSeqNum is the successor of its number, so datagram p is judged
// against seq_after(seq[p - 1]) -- datagram 0 against the carried state -- and what it adds to the missed count, its event
// bit and its index as a candidate for first_gap depend on two header words only.  A receiver's lanes stride over its
// datagrams; a lane reads the aligned header word of datagram p (the number is its high half) and takes datagram
// p - 1's from the lane below, the first lane of a wave from memory (the word the wave below has just read).  Sum, count
// and minimum go down the wave by shuffles and across the waves through LDS; thread 0 writes the receiver's record
// with ordinary stores.  No atomics, no scratch in global memory; offsets are 32 bit as in wire_format.hpp.
#include "seqcheck_kernels.h"
#include <climits>

// waves per receiver.  4: measured against 1 on 256 receivers x 2185 datagrams (HISTORY.md, "Datagram sequence check")
#ifndef SEQ_WAVES
#define SEQ_WAVES 4
#endif

namespace csdr {
namespace seq {

namespace {
constexpr int kWaves = SEQ_WAVES;
constexpr int kThreads = 64 * kWaves;

__device__ __forceinline__ unsigned header_seq(const unsigned char *chan, unsigned p, unsigned pkt_len)
{
    return seq_of_word(*reinterpret_cast<const unsigned *>(chan + p * pkt_len));
}
}  // namespace

__global__ __launch_bounds__(kThreads)
void seqcheck_put_kernel(const unsigned char *pk, unsigned chan_stride, int npackets, unsigned pkt_len, State *state)
{
    __shared__ long long red_missed[kWaves];
    __shared__ int red_events[kWaves], red_first[kWaves];
    const unsigned char *chan = pk + (size_t)blockIdx.x * chan_stride;
    State *st = state + blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long missed = 0;
    int events = 0, first = INT_MAX;
    for (int base = 0; base < npackets; base += kThreads) {      // uniform: every lane of a wave reaches the shuffle
        const int p = base + t;
        const bool mine = p < npackets;
        const unsigned s = mine ? header_seq(chan, (unsigned)p, pkt_len) : 0u;
        unsigned before = (unsigned)__shfl_up((int)s, 1);
        if (lane == 0 && mine && p > 0) before = header_seq(chan, (unsigned)p - 1u, pkt_len);
        if (mine) {
            const unsigned expected = p == 0 ? (unsigned)st->last : seq_after(before);
            int delta, event;
            seq_step(s, expected, &delta, &event);
            missed += delta; events += event;
            if (event && p < first) first = p;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        missed += __shfl_down(missed, o);
        events += __shfl_down(events, o);
        first = min(first, __shfl_down(first, o));
    }
    if (kWaves > 1) {
        if (lane == 0) { red_missed[wave] = missed; red_events[wave] = events; red_first[wave] = first; }
        __syncthreads();
    }
    if (t == 0) {
        for (int w = 1; w < kWaves; w++) { missed += red_missed[w]; events += red_events[w]; first = min(first, red_first[w]); }
        st->missed += missed;
        st->events += events;
        st->last = (int)seq_after(header_seq(chan, (unsigned)npackets - 1u, pkt_len));
        st->first_gap = first == INT_MAX ? -1 : first;
    }
}

__global__ __launch_bounds__(64)
void seqcheck_control_kernel(State *state, int lo, int hi, int reset)
{
    const int c = lo + (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= hi) return;
    state[c].missed = 0; state[c].events = 0;
    if (reset) state[c].last = 0;
}

__global__ __launch_bounds__(64)
void seqcheck_gather_kernel(const State *state, int channels, long long *missed, long long *events, int *first_gap)
{
    const int c = (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= channels) return;
    if (missed) missed[c] = state[c].missed;
    if (events) events[c] = state[c].events;
    if (first_gap) first_gap[c] = state[c].first_gap;
}

hipError_t seqcheck_put_launch(const unsigned char *pk, int channels, int npackets, int pkt_len, State *state, hipStream_t stream)
{
    if (npackets <= 0 || channels <= 0) return hipSuccess;
    hipLaunchKernelGGL(seqcheck_put_kernel, dim3(channels), dim3(kThreads), 0, stream, pk, (unsigned)npackets * (unsigned)pkt_len,
                       npackets, (unsigned)pkt_len, state);
    return hipGetLastError();
}
hipError_t seqcheck_control_launch(State *state, int lo, int hi, int reset, hipStream_t stream)
{
    if (hi <= lo) return hipSuccess;
    hipLaunchKernelGGL(seqcheck_control_kernel, dim3((hi - lo + 63) / 64), dim3(64), 0, stream, state, lo, hi, reset);
    return hipGetLastError();
}
hipError_t seqcheck_gather_launch(const State *state, int channels, long long *missed, long long *events, int *first_gap,
                                  hipStream_t stream)
{
    hipLaunchKernelGGL(seqcheck_gather_kernel, dim3((channels + 63) / 64), dim3(64), 0, stream, state, channels, missed, events,
                       first_gap);
    return hipGetLastError();
}
int seqcheck_waves() { return kWaves; }

}  // namespace seq
}  // namespace csdr
