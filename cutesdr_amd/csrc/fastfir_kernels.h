// fastfir_kernels.h -- launch interface of the batched overlap-save kernel (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "wg_trace.hpp"

namespace csdr {

typedef float v2f_h __attribute__((ext_vector_type(2)));
typedef float v4f_h __attribute__((ext_vector_type(4)));

struct FastFirArgs {
    const v2f_h *in;      // [channels][in_stride] complex fp32, this call's new samples
    const v2f_h *hist;    // [channels][N/2]: last N/2 samples of the previous call (zeros at start)
    v2f_h *hist_next;     // [channels][N/2]: receives this call's tail (other ping-pong half)
    v2f_h *out;           // [channels][out_stride]
    const v4f_h *h;       // frequency response in pass-F3 register order, [16][N/32] float4 per filter
    const v4f_h *gain;    // N = 16384, pipelined kernel, responses of the library's own design only (else null): the real
                          // gains P[k] = Re(H[k] (-j)^k) in that kernel's order, [8][N/32] float4 per filter (fastfir2_gain_bin_of)
    const v2f_h *tw1;     // W_N^{n}, n = 0..1023
    const v2f_h *tw2;     // W_1024^{n*k}, [k][n], 32x32
    long in_stride;       // complex samples between channels
    long out_stride;
    long h_stride;        // float4 between channel filters (0 = one shared filter)
    int channels;
    int nblocks;          // hops of N/2 samples per channel in this call
    int blocks_per_run;   // consecutive blocks walked by one workgroup
    int runs;             // ceil(nblocks / blocks_per_run)
    int dbg_stage;        // 0 in production; >0 selects the diagnostic twin kernel
    v2f_h *dbg;           // [N] LDS image dump of the diagnostic twin
#ifdef CSDR_WG_TRACE
    WgTraceArg trace;
#endif
};

hipError_t fastfir_launch(int log2n, const FastFirArgs &a, hipStream_t stream);
int fastfir_bin_of(int log2n, int t, int r);

// software-pipelined build, N = 2048 ... 16384 (fastfir2_kernels.hip): same LDS image as fastfir_launch, its
// own H order
// *kernel, where given, receives which kernel the launch took (FastFirKernel): the test hook
// csdr__fastfir_last_kernel reports it, so the answer comes from the code that chooses
enum FastFirKernel { FASTFIR_KERNEL_NONE = -1, FASTFIR_KERNEL_GENERIC = 0, FASTFIR_KERNEL_PIPELINED_H = 1, FASTFIR_KERNEL_PIPELINED_GAIN = 2 };
hipError_t fastfir2_launch(int log2n, const FastFirArgs &a, hipStream_t stream, int *kernel = nullptr);
// the K1_TWREG that unit was compiled with
int fastfir2_twreg();
// 1 where that unit's real-gain kernel runs its tail groups in the radix-4 form (K1_RADIX4; fft_core.hpp: dit_tail_r4)
int fastfir2_radix4();
// 1 where that unit's real-gain kernel keeps the outer-pass twiddle powers in registers for the whole run (K1_PWRES)
int fastfir2_pwres();
// how that unit's 16384-point kernels talk to HBM: bit 0 K1_RUNEND (no fetch behind a run's last block, the history tail
// stored inside the call's last block), bit 1 K1_PROLOGUE (one round trip in front of the block loop), bit 2 the real-gain
// kernel keeps no twiddle table in LDS (K1_TW2LDS, at K1_TWREG = 16), bit 3 K1_LDSPREAD (a block's loads in four pairs);
// and the dynamic LDS the real-gain kernel is launched with
int fastfir2_hbm_knobs();
int fastfir2_gain_lds_bytes();
// natural-order spectrum bin of H slot (float4 index j*(N/32) + t, half e) of that kernel
int fastfir2_bin_of(int log2n, int t, int j, int e);
// natural-order spectrum bin of gain slot (float4 index i*(N/32) + t, component c): the same per-thread order, four
// gains per tail group i
int fastfir2_gain_bin_of(int log2n, int t, int i, int c);
// The shared twiddles of the 16384-point kernels (rows k1 and 32 - k1 of the radix-32 passes on one twiddle, rows k0 and
// 16 - k0 of the outer pass on one power; fastfir2_twshare() is 2, the builds 0 and 1 are retired): by how many bins the
// outputs of thread t's row of F3 (*inner) and of its whole 1024-point sub-transform (*outer) are rotated, and the two
// orders above composed with that rotation -- the bin whose multiplier a slot has to hold.  What the uploads use.
int fastfir2_twshare();
void fastfir2_twshare_shift(int log2n, int t, int *inner, int *outer);
int fastfir2_slot_bin(int log2n, int t, int j, int e);
int fastfir2_gain_slot_bin(int log2n, int t, int i, int c);

}  // namespace csdr
