// nb_host.hpp -- the noise blanker's host-side logic (capi_frontend.hip): the tile geometry the kernels
// (noiseblank_kernels.hip) are written for, the rule that cuts a call into segments and the choice among the kernel's
// forms, as pure functions (csdr__host_nb_* in capi_hosttest.hip hands them to the CPU tests).
#pragma once
#include "frontend_kernels.h"

namespace csdr {

// 512 threads and two rounds of workgroups: 2.60 ms against 2.79 with 256 threads and one round (256 receivers x 2^21;
// 1024 threads 3.2 ms) -- fewer streams in flight per L2 at a time, for the sample leaving the moving-sum window
constexpr int NB_THREADS = 512;
// Samples per thread and tile: four, and EIGHT in the mask form with the ring.  Round 4, C4 share from 24-bit
// datagrams, per launch: two streams x 4 per thread 1.40 ms (74 registers, three workgroups per CU; bound by the
// fabric: 6.6 GB at 4.8 TB/s); two streams x 8: 18 % fewer vector instructions and the same 1.40 ms (123 registers, two
// workgroups per CU); ring x 4: 1.27 ms, now bound by the vector unit (84 % busy, 305 instructions per wave and
// 256 samples -- most of them per tile and thread: datagram addresses, the two scans, the workgroup sums, the mask
// word); ring x 8: 1.07 ms (92 registers, 64 KB of ring, two workgroups per CU, one round of 512 workgroups).
constexpr int NB_PER_THREAD = 4, NB_PER_THREAD_RING = 8;
constexpr int nb_per_thread(bool mask, bool ring) { return mask && ring ? NB_PER_THREAD_RING : NB_PER_THREAD; }
constexpr int nb_tile(bool mask, bool ring) { return NB_THREADS * nb_per_thread(mask, ring); }
// the magnitudes of a workgroup's last NB_RING samples stay in LDS (ring forms): 16384, four of the largest tile
constexpr int NB_RING = 4 * nb_tile(true, true);
// a segment is whole tiles of whichever form runs; the host cuts segments by the mask form's larger tile
constexpr int nb_seg_tile(bool mask) { return mask ? nb_tile(true, true) : nb_tile(false, false); }
constexpr int NB_MIN_SEG_TILES = 32;    // a segment that is not the whole call is at least this many tiles long
// The ring form runs when every channel with the blanker on has nb_ring_min <= mag_n + 1 <= nb_ring_max: the window
// is at least a tile behind (no barrier between a tile's ring writes and its own ring reads) and a tile short of the ring
constexpr int nb_ring_min(bool mask) { return nb_tile(mask, true); }
constexpr int nb_ring_max(bool mask) { return NB_RING - nb_ring_min(mask); }

// what the kernels rely on, where the constants meet
constexpr int nb_warmup(int width, int tile) { return (width + tile - 1) / tile * tile; }   // the tiles in front of a later segment
static_assert(4 * nb_warmup(NB_MAX_WIDTH, nb_tile(false, false)) <= NB_MIN_SEG_TILES * nb_seg_tile(false) &&
              4 * nb_warmup(NB_MAX_WIDTH, nb_tile(true, false)) <= NB_MIN_SEG_TILES * nb_seg_tile(true),
              "a later segment's warm-up starts inside the call: a segment is at least four warm-ups long");
static_assert(nb_seg_tile(true) % nb_tile(true, true) == 0 && nb_seg_tile(true) % nb_tile(true, false) == 0 &&
              nb_seg_tile(false) % nb_tile(false, true) == 0 && nb_seg_tile(false) % nb_tile(false, false) == 0,
              "segments are whole tiles of either form");
static_assert(NB_RING % nb_tile(true, true) == 0 && NB_RING % nb_tile(false, true) == 0, "tiles divide the ring");
static_assert(240 % NB_PER_THREAD_RING == 0 && 256 % NB_PER_THREAD_RING == 0 && nb_seg_tile(true) % NB_PER_THREAD_RING == 0,
              "integer form: a thread's eight samples lie in one datagram, and a segment ends on a multiple of eight");
static_assert(NB_MAX_WIDTH + 1 <= NB_HIST && NB_RING <= NB_HIST, "the history reaches as far back as a window or a delay");

// ---- segments ----------------------------------------------------------------------------------------------
// Each channel's call of n samples is cut into nseg segments of seg_len samples, one workgroup each: enough
// workgroups to fill the chip, each at least 32 tiles long (the longest blank width is 4 tiles, the moving-sum
// reduction at a segment start another ~10-32 tiles' worth of reads).
// (mask mode: 74 registers, three 512-thread workgroups per CU: 3072 workgroups = four rounds measured best,
// 3.28 ms for the C4 share's datagram-fed chain against 3.36 with 2048 and 3.49 with 4096)
// (with the ring: two workgroups per CU -- 64 KB of ring each -- and ONE round of them: mask form 1.07 ms against
// 1.11 with two rounds, 1.18 with six; sample form 2.20 against 2.24 and 2.29 with four)
constexpr long nb_want_workgroups(bool mask, bool ring) { return ring ? 512 : (mask ? 3072 : 2048); }
struct NbSegments { int nseg, seg_len; };
inline NbSegments nb_segments(long n, int channels, bool mask, bool ring)
{
    const long tile = nb_seg_tile(mask), min_seg = NB_MIN_SEG_TILES * tile;
    long nseg = (nb_want_workgroups(mask, ring) + channels - 1) / channels;
    if (nseg > n / min_seg) nseg = n / min_seg;
    if (nseg < 1) nseg = 1;
    const long seg_len = ((n + nseg - 1) / nseg + tile - 1) / tile * tile;
    return {(int)((n + seg_len - 1) / seg_len), (int)seg_len};
}

// ---- the kernel's forms ---------------------------------------------------------------------------------------
enum NbForm {
    NB_SAMPLES, NB_SAMPLES_RING,        // noiseblank_kernel<false, RING>: blanked, delayed samples out
    NB_MASK, NB_MASK_RING,              // noiseblank_kernel<true, RING>: one bit per sample out
    NB_MASK_INT24, NB_MASK_INT16        // noiseblank_mask_int_kernel<1444 / 1028>: the mask from datagrams, in integers
};
constexpr bool nb_form_ring(NbForm f) { return f != NB_SAMPLES && f != NB_MASK; }

struct NbHost {                          // one channel's SetupBlanker comparands (noiseproc.cpp:80-86)
    bool configured = false, on = false;
    double thresh = 0, width = 0, fs = 0;
    int mag_n = 0;                       // as on the device (a rate-only change does not reconfigure: not derivable from fs)
    bool integral = true;                // every sample since the last set-up (which clears sum and buffers) came from datagrams:
                                         // the moving sum and the history are whole multiples of 2^-8 (noiseblank_kernels.hip)
};
// mask: one bit per sample out (else samples); pkt_len: 0 for float rows, else the datagram length; the switches:
// CSDR_NB_RING and csdr__noiseproc_set_int.  A channel with the blanker off constrains nothing.
inline NbForm nb_choose_form(bool mask, int pkt_len, const NbHost *h, int channels, bool ring_switch, bool int_switch)
{
    bool ring = ring_switch, integral = int_switch && pkt_len != 0;
    for (int c = 0; c < channels; c++) {
        if (!h[c].on) continue;
        if (h[c].mag_n + 1 < nb_ring_min(mask) || h[c].mag_n + 1 > nb_ring_max(mask)) ring = false;
        if (!h[c].integral) integral = false;
    }
    if (mask && ring && integral) return pkt_len == 1444 ? NB_MASK_INT24 : NB_MASK_INT16;
    if (mask) return ring ? NB_MASK_RING : NB_MASK;
    return ring ? NB_SAMPLES_RING : NB_SAMPLES;
}

}  // namespace csdr
