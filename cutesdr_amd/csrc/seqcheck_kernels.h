// seqcheck_kernels.h -- launch interface of K12, the datagram sequence check (seqcheck_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include "seq_host.hpp"

namespace csdr {
namespace seq {

// state[ch] advanced over the npackets datagrams of pk [channels][npackets][pkt_len] (4-byte aligned, pkt_len a multiple
// of 4, npackets * pkt_len < 2 GiB: the caller checks); state[ch].first_gap is this call's
hipError_t seqcheck_put_launch(const unsigned char *pk, int channels, int npackets, int pkt_len, State *state, hipStream_t stream);
// channels lo .. hi - 1: missed, events <- 0; reset: last <- 0 too
hipError_t seqcheck_control_launch(State *state, int lo, int hi, int reset, hipStream_t stream);
// the records' fields into [channels] arrays of the caller's (any may be null)
hipError_t seqcheck_gather_launch(const State *state, int channels, long long *missed, long long *events, int *first_gap,
                                  hipStream_t stream);
int seqcheck_waves();                    // waves per receiver of this build

}  // namespace seq
}  // namespace csdr
