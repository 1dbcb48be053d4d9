// seq_host.hpp -- the datagram sequence bookkeeping of CUdpThread::OnreadyRead (reference interface/netiobase.cpp:484-496
// for 24 bit, :509-521 for 16 bit: the same text) as one function for host and device, so that the rule exists once:
// the kernel (seqcheck_kernels.hip) and the sequential walk (seq_walk below, exported for the tests) both call seq_step.
//
// A datagram's sequence number is bytes 2-3 of its four header bytes, little endian: the high half of the aligned
// 32-bit word the datagram starts with (seq_of_word).  Per receiver the state is m_LastSeqNum, a quint16 that starts at
// 0 (:433), and CNetIOBase::m_MissedPackets, the reference's int, held here in 64 bits.
#pragma once
#include <hip/hip_runtime.h>

namespace csdr {
namespace seq {

// what one receiver carries from call to call, and what a get reads
struct State {
    long long missed;                    // m_MissedPackets: the signed sum of the differences
    long long events;                    // datagrams whose number was not the expected one
    int last;                            // m_LastSeqNum
    int first_gap;                       // the last put's first such datagram, or -1
};

__host__ __device__ inline unsigned seq_of_word(unsigned header_word) { return header_word >> 16; }

// One datagram with number `seq` while m_LastSeqNum is `last`: returns m_LastSeqNum afterwards, *delta = what the
// datagram adds to m_MissedPackets ((qint16)seq - (qint16)last: one datagram lost across 0x7fff/0x8000 gives -65535,
// a duplicate -1), *event = whether it was out of sequence.
__host__ __device__ inline unsigned seq_step(unsigned seq, unsigned last, int *delta, int *event)
{
    if (seq == 0) last = 0;                              // :486-487 "is first packet after started"
    *event = seq != last;
    *delta = 0;
    if (seq != last) {                                   // :488-493
        *delta = (int)(short)(unsigned short)seq - (int)(short)(unsigned short)last;
        last = seq;
    }
    last = (last + 1) & 0xffffu;                         // :494 on a quint16
    if (last == 0) last = 1;                             // :495-496
    return last;
}

// m_LastSeqNum after a datagram with number `seq`, whatever it was before: the rule is no recurrence (after the
// datagram m_LastSeqNum is the successor of seq whether or not it matched), so datagram p is judged against
// seq_after(seq[p - 1]) and a receiver's call is a reduction
__host__ __device__ inline unsigned seq_after(unsigned seq)
{
    int delta, event;
    return seq_step(seq, seq, &delta, &event);
}

// the sequential form: npackets datagrams of pkt_len bytes one after the other, as OnreadyRead meets them; first_gap is
// this walk's alone
inline void seq_walk(const unsigned char *packets, int npackets, int pkt_len, State *s)
{
    s->first_gap = -1;
    for (int p = 0; p < npackets; p++) {
        const unsigned char *b = packets + (size_t)p * (size_t)pkt_len;
        int delta, event;
        s->last = (int)seq_step((unsigned)b[2] | ((unsigned)b[3] << 8), (unsigned)s->last, &delta, &event);
        s->missed += delta;
        s->events += event;
        if (event && s->first_gap < 0) s->first_gap = p;
    }
}

}  // namespace seq
}  // namespace csdr
