// fastfir2_kernels.hip -- batched overlap-save FFT FIR for gfx950, software-pipelined build (K1): N = 16384 (the
// headline configuration), and since round 5 N = 8192, 4096 and 2048 -- the same passes with an outer pass of radix 8 / 4 /
// 2 over four / eight / sixteen columns per thread (the instruction stream of the 16384-point instantiation is unchanged,
// checked in the ISA), 4096 points as two and 2048 points as four blocks side by side per workgroup (K1Cfg below).
//
// Same algorithm, LDS image, spectrum order and HBM traffic as fastfir_os_kernel
// (fastfir_kernels.hip; reference dsp/fastfir.cpp:268-321, dsp/fft.cpp:416-426): passes
// F1 (radix-R0 from HBM) | F2 (radix-32) | F3 + H + I1 (registers) | I2 (radix-32) | I3 (radix-R0,
// store the valid half).  What differs is the ORDER of the instruction stream.  The first build
// left the compiler a free hand and got, per pass, "all LDS reads | all butterflies | all LDS
// writes": with two waves per SIMD running in lockstep between the workgroup barriers, the LDS
// pipe and the VALU took turns (13.8k VALU + 9.2k LDS cycles per block against 24.8k measured).
// Here every pass is cut into groups of four points (fft_core.hpp: head / tail4 / head4 / tail):
//   * the points of a group are fetched in the order the first two stages need them, so the
//     butterflies start after four reads instead of thirty-two;
//   * a group's results are written while the next group's butterflies issue (one group behind);
//   * the 8-byte LDS accesses are relaxed atomics: hipcc neither merges them into ds_read2_b64 /
//     ds_write2_b64 (half the LDS rate of ds_read_b64) nor reorders them, and still counts them
//     in its s_waitcnt bookkeeping;
//   * sched_barrier(0) between groups pins that order against the machine scheduler.
// The outer-pass twiddle powers: in the real-gain kernel computed once, in front of the block loop, and resident for the
// whole run (K1_PWRES); in every other kernel computed once per block (pass I3) and reused by pass F1 of the next block.
#define CSDR_FMA_BFLY 1          // FMA-form decimation-in-time butterflies (fft_core.hpp)
#define CSDR_PLAIN_CONST_FMA 1   // ... written without asm where the twiddle is a compile-time constant
#include "launch_once.hpp"
#include "fastfir_dev.hpp"
#include "fastfir_kernels.h"

namespace csdr {

// Round-3 knobs (each A/B'd with tools/ab_many.sh).  The kernel runs at the chip's POWER limit
// (1.87-1.91 GHz in-kernel against 2.4 nominal, tools/k1_cycles.py): what shortens a launch is less energy per
// block -- fewer instructions, fewer bytes moved -- not fewer stall cycles.
#ifndef K1_LDAUX
#define K1_LDAUX 2          // cache policy of the input loads: nt (every sample is read once)
#endif
#ifndef K1_STAUX
#define K1_STAUX 2          // ... and of the output stores (written once)
#endif
#ifndef K1_HREG
#define K1_HREG 8           // float4 of this thread's share of H that stay in registers for the whole run (0..8 fit)
#endif
#ifndef K1_TWREG
#define K1_TWREG 16         // real-gain kernel: pass twiddles k1 = 1 ... of F2 / I2 that stay in registers.  All sixteen the
                            // passes use fit (254 VGPRs beside the resident outer powers, no scratch) and none is read from LDS (HISTORY.md; 3 is the build
                            // tests/test_fastfir_twreg_gpu.py runs beside it)
#endif
#ifndef K1_HREG4K
#define K1_HREG4K 4         // ... at N = 4096, whose outer pass (eight columns of four points) keeps more values live
#endif
#ifndef K1_W1_FETCH_MAX_R0
#define K1_W1_FETCH_MAX_R0 2 // outer radix up to which the base twiddles are fetched per block instead of held (2: N = 2048 only;
                             // at N = 4096 the fetch removes the kernel's 40 bytes of scratch and measures 1.5 % SLOWER)
#endif
#ifndef K1_HREG2K
#define K1_HREG2K 8         // ... at N = 2048 (the sixteen base twiddles are fetched where they are used: 0 / 4 / 8 resident measured 0.710 / 0.697 / 0.689 ms)
#endif
#ifndef K1_RADIX4
#define K1_RADIX4 1         // real-gain kernel: the last two stages of every register network as radix-4 groups on shared
                            // products (fft_core.hpp: dit_tail_r4), eleven packed instructions a group instead of twelve
#endif
#ifndef K1_PWRES
#define K1_PWRES 1          // real-gain kernel: the outer-pass twiddle powers are built once in front of the block loop and stay
                            // in registers for the whole run (0: rebuilt at the top of every I3, as in every other kernel)
#endif
// How the 16384-point kernels talk to HBM over a block and over a run (HISTORY.md, "A block's HBM traffic spread
// out"; every one at 0 gives the instruction stream before them, line for line).  Kernel time of bench.py's C3, parent 0.5739 ms:
#ifndef K1_RUNEND
#define K1_RUNEND 1         // the prefetch behind the last block of a run asks an EMPTY buffer range (zeros, no fetch), and the
                            // history tail is stored from inside the call's last block instead of behind the block loop (alone
                            // +0.2 %, within the visit's spread; beside K1_LDSPREAD -0.15 %; kept for the bytes it no longer moves)
#endif
#ifndef K1_PROLOGUE
#define K1_PROLOGUE 0       // in front of the block loop every load is issued before the first wait: one round trip, not two
                            // (alone 0.6 % SLOWER, beside K1_LDSPREAD -0.25 %, on top of K1_RUNEND and K1_LDSPREAD nothing: off)
#endif
#ifndef K1_TW2LDS
#define K1_TW2LDS 0         // 1: the real-gain kernel with all sixteen pass twiddles in registers neither copies the table into
                            // LDS nor reserves its 8 KiB (alone 0.8 % SLOWER, beside K1_LDSPREAD -0.3 %, on top of the two nothing: off)
#endif
#ifndef K1_LDSPREAD
#define K1_LDSPREAD 1       // real-gain kernel: the next new half's eight loads as four pairs in front of F2, F3, I2 and I3 instead
                            // of one burst in F1 (-1.1 % alone, -1.25 % with K1_RUNEND: every run under every parent run of two visits)
#endif
static_assert(K1_TWREG >= 0 && K1_TWREG <= 16, "K1_TWREG");

#define CSDR_SB() __builtin_amdgcn_sched_barrier(0)

// Priority ladder.  The two waves of a SIMD (w and w+4) run the same code between two workgroup barriers, and
// the SIMD issues by priority, then age: left alone, the older wave takes every slot it can use, reaches the
// barrier thousands of cycles early and waits while the younger one runs alone at a single wave's issue
// rate (in-kernel stamps: 8.3k of 21.7k cycles per block spent waiting).  Lowering the priority step by step
// through the interval (3, 2, 1, 0) makes whichever wave is behind the preferred one: the pair stays within
// one segment of each other and the waits fall to 2k cycles.
#define CSDR_PRIO(p) __builtin_amdgcn_s_setprio(p)

// Diagnostic build only (-DCSDR_K1_STAMPS, tools/k1_stamps.py): cycle shares of the passes of one block,
// summed per wave in scalar registers and written to a.dbg after the loop.  No stamp executes otherwise.
#ifdef CSDR_K1_STAMPS
#define CSDR_STAMP(i)                                                                         \
    do {                                                                                      \
        CSDR_SB();                                                                            \
        unsigned long long now_;                                                              \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");         \
        CSDR_SB();                                                                            \
        acc_[i] += now_ - last_;                                                              \
        last_ = now_;                                                                         \
    } while (0)
#define CSDR_STAMP_PARAMS , unsigned long long (&acc_)[16], unsigned long long &last_       // (for F2, which stamps inside itself)
#define CSDR_STAMP_ARGS , acc_, last_
#else
#define CSDR_STAMP(i) do { } while (0)
#define CSDR_STAMP_PARAMS
#define CSDR_STAMP_ARGS
#endif

template <int I> using int_c = std::integral_constant<int, I>;

// "Compute group i, write group i - 1": a pass's NG groups of results go to LDS or HBM one group behind the butterflies,
// as one fenced group of wide stores each (fastfir_dev.hpp) ...
template <int NG, class Compute, class Store> __device__ __forceinline__ void one_group_behind(Compute &&compute, Store &&store)
{
    static_for<0, NG + 1>([&](auto I) {
        constexpr int i = I.value;
        if constexpr (i < NG) compute(I);
        if constexpr (i > 0) {
            CSDR_STORE_GROUP_BEGIN();
            store(int_c<i - 1>{});
            CSDR_STORE_GROUP_END();
        } else {
            CSDR_SB();
        }
    });
}
// ... and the same for 8-byte LDS stores (lds_st8), which are not subject to the wide-store hazard
template <int NG, class Compute, class Store> __device__ __forceinline__ void one_group_behind_st8(Compute &&compute, Store &&store)
{
    static_for<0, NG + 1>([&](auto I) {
        constexpr int i = I.value;
        if constexpr (i < NG) compute(I);
        if constexpr (i > 0) store(int_c<i - 1>{});
        CSDR_SB();
    });
}

// The twiddle sets of the 16384-point kernels.  The table entry of row k1 and column sn is W_1024^(sn k1), and
// W_1024^(sn (32 - k1)) = W_32^sn conj(W_1024^(sn k1)):
// rows 17 ... 31 of F2 take conj(twiddle 32 - k1) and are then W_32^(-sn) off, which F3 -- a transform over sn -- turns into a
// circular shift of its 32 outputs by one bin (index j of such a row holds bin j - 1).  No instruction looks at what bin a
// register holds; only the upload order of H / the gains does (fastfir2_slot_bin).  I1 returns such a row times
// conj(W_32^sn), which with twiddle 32 - k1 UNconjugated is the conjugate twiddle I2 needs.  Tail group i of F2 and head
// group bitrev3(i) of I2 hold the rows k1 = i + 8 {0, 1, 2, 3}: groups i and 8 - i run on the same four twiddles.  The groups
// are walked in the order 0, 4, (1, 7), (2, 6), (3, 5) -- step s is group tws_group(s) -- on twiddle SETS: set 0 = rows {8, 16},
// set 1 = {4, 12}, set 1 + m = {m, m + 8, 8 - m, 16 - m} for the pair (m, 8 - m).
constexpr int tws_group(int step) { return step < 2 ? 4 * step : ((step & 1) ? 8 - step / 2 : step / 2); }
constexpr int tws_set(int step) { return step < 2 ? step : 1 + step / 2; }
constexpr bool tws_opens(int step) { return step < 2 || (step & 1) == 0; }          // the step is the first of its set
constexpr int tws_row(int set, int slot)                                             // table row in `slot` of `set` (0: none)
{
    if (set < 2) return slot < 2 ? 8 - 4 * set + 8 * slot : 0;
    const int m = set - 1;
    return slot == 0 ? m : (slot == 1 ? m + 8 : (slot == 2 ? 8 - m : 16 - m));
}
constexpr int tws_row_of(int k1) { return k1 <= 16 ? k1 : 32 - k1; }                 // the table row that serves row k1
constexpr int tws_set_of(int k1)
{
    const int r = tws_row_of(k1) & 7;
    return r == 0 ? 0 : (r == 4 ? 1 : 1 + (r < 4 ? r : 8 - r));
}
constexpr int tws_slot_of(int k1)
{
    for (int slot = 0; slot < 4; slot++)
        if (tws_row(tws_set_of(k1), slot) == tws_row_of(k1)) return slot;
    return -1;
}
static_assert(tws_group(2) == 1 && tws_group(3) == 7 && tws_group(7) == 5 && tws_set(7) == 4 && tws_set_of(31) == 2 &&
              tws_slot_of(24) == 0 && tws_slot_of(16) == 1 && tws_slot_of(20) == 1 && tws_slot_of(25) == 2 && tws_slot_of(23) == 1,
              "twiddle sets of the 16384-point kernels");

// (N = 2048 likewise: FOUR blocks of one wave each, and a block's barriers are wave barriers.)
// N = 4096 runs TWO blocks side by side in one workgroup: a block of 4096 points is 128 threads and 43 KB of LDS, three
// workgroups -- six waves -- per CU, against the eight (two per SIMD) the schedule below is made for.  Two "virtual
// workgroups" of 128 threads, each with its own LDS image and its own run of blocks, sharing the twiddle table and the
// (then merely coincident) barriers: 256 threads, 78 KB, two per CU, eight waves -- the shape of the 8192-point launch.
//
// RG ("real gains", N = 16384 only): the responses are the library's own design, H[k] = P[k] j^k with P real
// (host_math.hpp: fastfir_gain).  The multiply between the transforms is then a real scale by P that rides in I1's first
// butterflies, all 32 gains of a thread stay in registers for the whole run and nothing of H is fetched inside the block
// loop; the factor j^k is a circular shift of the block by N/4 samples -- four rows of the outer pass -- that I3 takes by
// finishing rows 4 ... 11 instead of 8 ... 15.  The registers the in-flight half of H used hold pass twiddles of F2 / I2.
template <int LOG2N, bool RG = false>
struct K1Cfg {
    using Base = FastFirCfg<LOG2N>;
    static_assert(!RG || LOG2N == 14, "the quarter-block shift is whole rows of the outer pass at N = 16384 only");
    static constexpr int VW = LOG2N == 12 ? 2 : (LOG2N == 11 ? 4 : 1);      // virtual workgroups per workgroup
    static constexpr int TV = Base::T;                                      // threads of one block
    static constexpr int T = VW * TV;

    static constexpr int N = Base::N, R0 = Base::R0, G = Base::G, L = N / 2, HALF = R0 / 2;
    static_assert(R0 == 16 || R0 == 8 || R0 == 4 || R0 == 2, "the grouped outer pass is written for N = 2048 ... 16384");
    // A thread's G columns of the outer pass are G / 2 PAIRS, pair pp = columns PSTEP pp + 2t, + 1 (PSTEP = 2 TV: every
    // load, store and 16-byte LDS access of a wave covers 64 adjacent pairs -- with G adjacent columns per thread the
    // four 16-byte accesses of the 4096-point kernel each touched a quarter of every line: 1.8 ms instead of 0.8)
    static constexpr int PSTEP = 2 * TV, PSTEP_LDS = PSTEP + 2 * (PSTEP / 32), PSTEP_B = PSTEP * 8;
    static constexpr int OUTER_ROW = 1024 + 2 * (1024 / 32);       // padded elements between rows of the outer pass
    // The 16384-point kernels only: rows k1 and 32 - k1 of F2 / I2 share one pass twiddle (tws_* above), and rows k0 and
    // 16 - k0 of the outer pass one power: W_N^(n2 (16 - k0)) = W_1024^n2 conj(W_N^(n2 k0)) -- rows 9 ... 15 of F1 take
    // conj(power 16 - k0), which leaves the whole 1024-point sub-transform one bin on, I3 takes the same power
    // unconjugated: powers 1 ... 8 only.  The smaller sizes keep a twiddle per row and with it their former words: with the
    // inner step at N = 2048 (whose filter words then differ in the last bits; its error stays 1.1e-7 of max|x|) a SAM
    // receiver restarted inside tests/test_batch_control_combinations_gpu.py::test_seeded_control_sequence_on_datagrams_with_
    // the_blanker came out 1.0e-2 / 7.8e-3 of full scale off in its first two bursts, bound 1e-3 (HISTORY.md, "Shared twiddles")
    static constexpr bool TWS = LOG2N == 14;
    static constexpr int PWN = R0 == 16 ? R0 / 2 + 1 : R0;
    static constexpr bool W1_RESIDENT = R0 > K1_W1_FETCH_MAX_R0;    // the base twiddles stay in registers for the whole run
    static constexpr int HREG = RG ? 0 : (LOG2N == 12 ? K1_HREG4K : (LOG2N == 11 ? K1_HREG2K : K1_HREG));   // resident float4 of H
    static constexpr int TWREG = RG ? K1_TWREG : 0;      // pass twiddles k1 = 1 ... TWREG of F2 / I2 that stay in registers
    static constexpr bool R4 = RG && K1_RADIX4 != 0;     // tail groups in the radix-4 form (other rounding order: this kernel only)
    static constexpr bool PW_RESIDENT = RG && K1_PWRES != 0;   // the outer-pass powers are built once per run, not once per block
    static constexpr bool TW2_LDS = !(RG && TWREG == 16 && K1_TW2LDS != 0);      // some pass reads a twiddle from the table in LDS
    static constexpr int LDS_BYTES = (VW * Base::LDS_DATA + (TW2_LDS ? 1024 : 0)) * 8;
    static constexpr bool RUNEND = LOG2N == 14 && K1_RUNEND != 0;                // (the 16384-point kernels, real gains and complex H)
    static constexpr bool PROLOGUE = LOG2N == 14 && K1_PROLOGUE != 0;
    static constexpr bool LDSPREAD = RG && K1_LDSPREAD != 0;       // (on complex H the pairs would move the waits of H's fetches)

    // the register arrays a thread carries through the block loop
    using Y = v2f[G][R0];                   // F1 / I3: the R0 points of this thread's G columns
    using W1 = v2f[R0 > 2 ? G : 1];         // base twiddles W_N^n2 of those columns
    using Pw = v2f[G][PWN];                 // ... and their powers, pw[e][k0]
    using Hv = v4f[RG ? 1 : 16];            // H: float4 j (fastfir2_bin_of) multiplies in F3's tail group j / 2
    using Pv = v4f[RG ? 8 : 1];             // RG: float4 i (fastfir2_gain_bin_of), the gains of the four bins tail group i of F3 finishes
    using Twr = v2f[TWREG > 0 ? TWREG : 1];
};

// Half a block's input: v[e * HALF + n1] = column PSTEP (e / 2) + 2t + (e & 1), row n1.  A struct around the array: a bare
// v2f[16] that is live across the block loop is made one 32-float vector by the compiler's alloca promotion before it is
// split into registers, and leaves 35 moves at the loop exit.
struct K1Half { v2f v[16]; };

// What a thread computes once and every pass of every block reads
struct K1Thread {
    int t, voff;                    // thread of the block, and its byte offset among a row's column pairs
    v2f *col;                       // F2 / I2: point n1 of sub-transform sb, column sn at col[34 * n1]
    const v2f *twc;                 // ... and twiddle k1 at twc[32 * k1]
    v2f *rowp;                      // F3: this thread's 32 consecutive points
    v2f *outer;                     // F1 / I3: row k0, pair pp at outer[OUTER_ROW k0 + PSTEP_LDS pp]
    const v2f_h *tw1;               // FastFirArgs: the base twiddles, the block count, and the buffers of this channel
    int nblocks;
    rsrc_t r_in, r_h, r_out;
    const void *in;                 // K1_RUNEND: this channel's input and its bytes (k1_next_half builds the range per block), the end
    unsigned in_bytes;              // of this workgroup's run, and the history half the call's last block writes
    int run_end;
    rsrc_t r_hn;
#ifdef K1_ABLATE
    v4f habl;
    v2f twabl;
#endif
};

// Timing ablations (tools/altlib.py NAME -DK1_ABLATE -DABL_...; the results are garbage, never shipped): H from a
// constant instead of L2 (ABL_H, k1_fetch_h), pass twiddles from a constant instead of LDS (ABL_TW, k1_pass_tw), no
// workgroup barriers (ABL_BAR, k1_block_barrier), no output stores (ABL_GST, k1_store_out).
#ifdef K1_ABLATE
__device__ __forceinline__ void keep_alive(v4f v) { asm volatile("" ::"v"(v)); }
#endif

// a block of 2048 points is ONE wave: its two "workgroup" barriers are wave barriers (the four blocks of a workgroup
// then run free of each other)
template <int LOG2N> __device__ __forceinline__ void k1_block_barrier()
{
#ifdef ABL_BAR
    wave_sync();
#else
    if constexpr (LOG2N == 11) wave_sync();
    else __syncthreads();
#endif
}

// twiddle K1 of F2 / I2: the first TWREG from registers (read once, from the table in device memory), the rest from LDS
template <int LOG2N, bool RG, int K1> __device__ __forceinline__ v2f k1_pass_tw(const K1Thread &c, const typename K1Cfg<LOG2N, RG>::Twr &twr)
{
#ifdef ABL_TW
    return c.twabl;
#else
    if constexpr (K1 <= K1Cfg<LOG2N, RG>::TWREG) return twr[K1 - 1];
    else return lds_ld8(c.twc + 32 * K1);
#endif
}

// float4 J of this thread's share of H, where it is not resident (K1_HREG): from L2, in flight from F2's tail group J / 2
// to the multiply in F3
template <int LOG2N, int J> __device__ __forceinline__ void k1_fetch_h(const K1Thread &c, typename K1Cfg<LOG2N>::Hv &hv)
{
#ifdef ABL_H
    hv[J] = c.habl;
#else
    if constexpr (J >= K1Cfg<LOG2N>::HREG) hv[J] = buf_load16(c.r_h, c.t * 16, J * (K1Cfg<LOG2N>::TV * 16));
#endif
}

// one float4 of the output (the ablation is written for the 16384-point kernels only)
template <int LOG2N> __device__ __forceinline__ void k1_store_out(const K1Thread &c, int voff, int soff, v4f v)
{
#ifdef ABL_GST
    if constexpr (LOG2N == 14) { keep_alive(v); return; }
#endif
    buf_store16_aux<K1_STAUX>(c.r_out, voff, soff, v);
}

// one hop-half of samples: rows n1 = 0..HALF-1 of 1024 samples, this thread's G / 2 column pairs
// (K1_LDSPREAD: rows N1A ... N1B - 1 of it)
template <int LOG2N, int N1A = 0, int N1B = K1Cfg<LOG2N>::HALF>
__device__ __forceinline__ void k1_load_half(rsrc_t r, int voff, int soff, v2f (&dst)[16])
{
    using Cfg = K1Cfg<LOG2N>;
#pragma unroll
    for (int n1 = N1A; n1 < N1B; n1++)
#pragma unroll
        for (int pp = 0; pp < Cfg::G / 2; pp++) {
            v4f v = buf_load16_aux<K1_LDAUX>(r, voff + pp * Cfg::PSTEP_B, soff + n1 * 8192);
            dst[(2 * pp) * Cfg::HALF + n1] = v2f{v.x, v.y};
            dst[(2 * pp + 1) * Cfg::HALF + n1] = v2f{v.z, v.w};
        }
}
// Where block b's prefetch -- the new half of block b + 1 -- is asked for.  The block is one straight line of code, so the
// loads are issued behind every block.  K1_RUNEND: behind the last block of a run they ask a buffer range of NO bytes, which
// the range check answers with zeros and without a fetch (the offset stays one inside the input all the same); before,
// they fetched block b + 1 where the input has one -- a run that ends inside the call -- and the last block again
// where it has not, and nobody used the samples
struct K1Next { rsrc_t r; int soff; };
template <int LOG2N> __device__ __forceinline__ K1Next k1_next_half(const K1Thread &c, int b)
{
    using Cfg = K1Cfg<LOG2N>;
    if constexpr (Cfg::RUNEND) {
        const bool more = b + 1 < c.run_end;
        return K1Next{make_rsrc(c.in, more ? c.in_bytes : 0u), (more ? b + 1 : b) * (Cfg::L * 8)};
    } else {
        return K1Next{c.r_in, (b + 1 < c.nblocks ? b + 1 : c.nblocks - 1) * (Cfg::L * 8)};
    }
}
// The tail of this call's input is the overlap of the next call (fastfir.cpp:280-300): the new half of the call's last
// block, written to the other half of the ping-pong history so no workgroup can still be reading it
template <int LOG2N> __device__ __forceinline__ void k1_store_hist(rsrc_t r_hn, int voff, const K1Half &h)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int G = Cfg::G, HALF = Cfg::HALF;
    v4f sv[8];
#pragma unroll
    for (int n1 = 0; n1 < HALF; n1++)
#pragma unroll
        for (int pp = 0; pp < G / 2; pp++)
            sv[n1 * (G / 2) + pp] = store_operand(h.v[(2 * pp) * HALF + n1], h.v[(2 * pp + 1) * HALF + n1]);
    CSDR_STORE_GROUP_BEGIN();
#pragma unroll
    for (int n1 = 0; n1 < HALF; n1++)
#pragma unroll
        for (int pp = 0; pp < G / 2; pp++) buf_store16(r_hn, voff + pp * Cfg::PSTEP_B, n1 * 8192, sv[n1 * (G / 2) + pp]);
    CSDR_STORE_GROUP_END();
}

// outer-pass twiddles W_N^{n2 k0}, n2 = 2t+e: pw[e][k0], k0 = 1 ... PWN - 1.  On complex H (and at the smaller sizes) rebuilt
// at the top of every I3 and kept for F1 of the next block only: live across the whole loop they would not fit beside H.
// The real-gain kernel holds no H and eight powers per column instead of fifteen: there the set fastfir_os2_body builds
// in front of the block loop stays for the whole run (K1Cfg::PW_RESIDENT) -- the same products on the same inputs, once
// (N = 2048: sixteen base twiddles and no powers -- they are fetched where the outer passes use them, 8 KB of table
// that stays in the vector cache, instead of thirty-two registers held for the whole run)
template <int LOG2N> __device__ __forceinline__ v4f k1_w_pair(const K1Thread &c, int pp)
{
    return *reinterpret_cast<const v4f *>(c.tw1 + K1Cfg<LOG2N>::PSTEP * pp + 2 * c.t);
}
template <int LOG2N> __device__ __forceinline__ void k1_load_w1(const K1Thread &c, typename K1Cfg<LOG2N>::W1 &w1)
{
    if constexpr (K1Cfg<LOG2N>::R0 > 2) {
#pragma unroll
        for (int pp = 0; pp < K1Cfg<LOG2N>::G / 2; pp++) { const v4f v = k1_w_pair<LOG2N>(c, pp); w1[2 * pp] = v2f{v.x, v.y}; w1[2 * pp + 1] = v2f{v.z, v.w}; }
    }
}

// ================= F1: radix-R0 forward transform of [oldh | newh], twiddle, scatter to LDS =================
// (a decimation-in-time network like every transform of this kernel -- FMA butterflies; its
// bit-reversed input order costs nothing, the samples sit in registers: position bitrev(n1) <- row n1)
//
// The last stage, the twiddles and the stores, four float4 per group, stored one group behind.
// N = 16384: tail group i finishes rows k0 = i, i+4, i+8, i+12; rows above 8 take conj(power 16 - k0) (K1Cfg::TWS)
template <int LOG2N, bool RG> __device__ __forceinline__ void k1_f1_rows16(const K1Thread &c, typename K1Cfg<LOG2N>::Y &y, typename K1Cfg<LOG2N>::Pw &pw)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int R0 = Cfg::R0;
    v4f wv[16];                                    // row k0 at [k0]
    one_group_behind<R0 / 4>([&](auto Ii) {
        constexpr int i = Ii.value;
        dit_tail_sel<K1Cfg<LOG2N, RG>::R4, i, R0, +1>(y[0]);
        dit_tail_sel<K1Cfg<LOG2N, RG>::R4, i, R0, +1>(y[1]);
        static_for<0, 4>([&](auto P) {
            constexpr int k0 = i + 4 * P.value;
            if constexpr (k0 > R0 / 2) {
                y[0][k0] = cmul_conj(y[0][k0], pw[0][R0 - k0]);
                y[1][k0] = cmul_conj(y[1][k0], pw[1][R0 - k0]);
            } else if constexpr (k0 != 0) {
                y[0][k0] = cmul(y[0][k0], pw[0][k0]);
                y[1][k0] = cmul(y[1][k0], pw[1][k0]);
            }
            wv[k0] = store_operand(y[0][k0], y[1][k0]);
        });
    }, [&](auto Ii) {                              // rows of the previous group: written while this one computes
        static_for<0, 4>([&](auto P) {
            constexpr int k0 = Ii.value + 4 * P.value;
            *reinterpret_cast<v4f *>(c.outer + Cfg::OUTER_ROW * k0) = wv[k0];
        });
    });
}
// N = 2048: the one butterfly of the head was the whole outer transform; group i = rows 0, 1 of the pairs 2i, 2i + 1
template <int LOG2N> __device__ __forceinline__ void k1_f1_rows2(const K1Thread &c, typename K1Cfg<LOG2N>::Y &y)
{
    using Cfg = K1Cfg<LOG2N>;
    v4f wv[16], wq[8];
    static_for<0, 8>([&](auto PP) { wq[PP.value] = k1_w_pair<LOG2N>(c, PP.value); });
    one_group_behind<4>([&](auto Ii) {
        static_for<0, 2>([&](auto Q) {
            constexpr int pp = 2 * Ii.value + Q.value;
            y[2 * pp][1] = cmul(y[2 * pp][1], v2f{wq[pp].x, wq[pp].y});
            y[2 * pp + 1][1] = cmul(y[2 * pp + 1][1], v2f{wq[pp].z, wq[pp].w});
            wv[pp] = store_operand(y[2 * pp][0], y[2 * pp + 1][0]);
            wv[8 + pp] = store_operand(y[2 * pp][1], y[2 * pp + 1][1]);
        });
    }, [&](auto Ii) {
        static_for<0, 2>([&](auto Q) {
            constexpr int pp = 2 * Ii.value + Q.value;
            *reinterpret_cast<v4f *>(c.outer + Cfg::PSTEP_LDS * pp) = wv[pp];
            *reinterpret_cast<v4f *>(c.outer + Cfg::OUTER_ROW + Cfg::PSTEP_LDS * pp) = wv[8 + pp];
        });
    });
}
// N = 8192: the last stage (8) in four groups, group i finishes rows k0 = i, i + 4 of the G = 4 columns;
// N = 4096: the head group was the whole radix-4 transform, group i is row k0 = i of the G = 8 columns.
template <int LOG2N> __device__ __forceinline__ void k1_f1_rows84(const K1Thread &c, typename K1Cfg<LOG2N>::Y &y, typename K1Cfg<LOG2N>::Pw &pw)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int R0 = Cfg::R0, G = Cfg::G, NG = 4, RPG = R0 / NG;           // rows per group
    v4f wv[16];                                    // (R0 rows) x (G / 2 column pairs): row k0, pair pp at [k0 * (G / 2) + pp]
    one_group_behind<NG>([&](auto Ii) {
        constexpr int i = Ii.value;
        if constexpr (R0 == 8)
            static_for<0, G>([&](auto E) { bfly_dit<4 * i, +1>(y[E.value][i], y[E.value][i + 4]); });
        static_for<0, RPG>([&](auto P) {
            constexpr int k0 = i + NG * P.value;
            static_for<0, G>([&](auto E) {
                if constexpr (k0 != 0) y[E.value][k0] = cmul(y[E.value][k0], pw[E.value][k0]);
            });
            static_for<0, G / 2>([&](auto PP) {
                wv[k0 * (G / 2) + PP.value] = store_operand(y[2 * PP.value][k0], y[2 * PP.value + 1][k0]);
            });
        });
    }, [&](auto Ii) {
        static_for<0, RPG>([&](auto P) {
            constexpr int k0 = Ii.value + NG * P.value;
            static_for<0, G / 2>([&](auto PP) {
                *reinterpret_cast<v4f *>(c.outer + Cfg::OUTER_ROW * k0 + Cfg::PSTEP_LDS * PP.value) = wv[k0 * (G / 2) + PP.value];
            });
        });
    });
}
template <int LOG2N, bool RG> __device__ __forceinline__ void k1_pass_f1(const K1Thread &c, int b, K1Half &oldh, K1Half &newh, typename K1Cfg<LOG2N>::Pw &pw)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int R0 = Cfg::R0, G = Cfg::G, HALF = Cfg::HALF;
    typename Cfg::Y y;
    static_for<0, HALF>([&](auto N1) {
        static_for<0, G>([&](auto E) {
            constexpr int e = E.value, n1 = N1.value, po = bitrev<R0>(n1), pn = bitrev<R0>(HALF + n1);
            y[e][po] = oldh.v[e * HALF + n1]; y[e][pn] = newh.v[e * HALF + n1];
        });
    });
    if constexpr (R0 == 2) {
        static_for<0, G>([&](auto E) { bfly_dit<0, +1>(y[E.value][0], y[E.value][1]); });
    } else {
        static_for<0, (R0 >= 8 ? R0 / 4 : 1)>([&](auto Gg) {
            static_for<0, G>([&](auto E) { dit_head4<Gg.value, R0, +1>(y[E.value]); });
        });
    }
    CSDR_SB();
    // block b+1's new half: into the registers of the old half, which the butterflies above have read
    // (unconditional, so that the block stays one straight line of code: k1_next_half).  K1_RUNEND: the call's last block
    // first stores its new half -- the next call's history, whole in registers here -- while the CUs still have a block of
    // arithmetic in front of them: a uniform branch that one block of the call's last run takes
    if constexpr (Cfg::RUNEND) {
        if (b + 1 == c.nblocks) k1_store_hist<LOG2N>(c.r_hn, c.voff, newh);
        CSDR_SB();
    }
    if constexpr (!K1Cfg<LOG2N, RG>::LDSPREAD) {
        const K1Next nx = k1_next_half<LOG2N>(c, b);
        k1_load_half<LOG2N>(nx.r, c.voff, nx.soff, oldh.v);
    }
    CSDR_SB();
    CSDR_PRIO(0);
    if constexpr (R0 == 16) k1_f1_rows16<LOG2N, RG>(c, y, pw);
    else if constexpr (R0 == 2) k1_f1_rows2<LOG2N>(c, y);
    else k1_f1_rows84<LOG2N>(c, y, pw);
}

// ================= F2: radix-32 forward inside sub-transform sb, column sn =================
// Tail group i finishes k1 = i, i+8, i+16, i+24: twiddle, store (one group behind).  H[k] comes from
// L2 (what is not resident: K1_HREG), at most two loads per tail group (a burst of sixteen held the wave for
// ~500 cycles of issue alone), in flight from here to the multiply in F3.
// N = 16384: the groups in the order tws_group, a twiddle set read one step ahead of the first group it serves;
// the H fetches keep their order, two per step
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_f2_tail_shared(const K1Thread &c, v2f (&x)[32], typename K1Cfg<LOG2N, RG>::Hv &hv,
                                                  const typename K1Cfg<LOG2N, RG>::Twr &twr CSDR_STAMP_PARAMS)
{
    v2f tw[5][4];
    auto load_set = [&](auto S) {
        static_for<0, 4>([&](auto Q) {
            constexpr int row = tws_row(S.value, Q.value);
            if constexpr (row != 0) tw[S.value][Q.value] = k1_pass_tw<LOG2N, RG, row>(c, twr);
        });
    };
    load_set(int_c<0>{});
    CSDR_SB();
    CSDR_STAMP(8);                             // F2 middle stage
    one_group_behind_st8<8>([&](auto St) {
        constexpr int s = St.value, i = tws_group(s);
        if constexpr (s < 7 && tws_opens(s + 1)) load_set(int_c<tws_set(s + 1)>{});
        if constexpr (!RG) { k1_fetch_h<LOG2N, 2 * s>(c, hv); k1_fetch_h<LOG2N, 2 * s + 1>(c, hv); }
        dit_tail_sel<K1Cfg<LOG2N, RG>::R4, i, 32, +1>(x);
        static_for<0, 4>([&](auto P) {
            constexpr int k1 = i + 8 * P.value;
            if constexpr (k1 != 0 && k1 <= 16) x[k1] = cmul(x[k1], tw[tws_set_of(k1)][tws_slot_of(k1)]);
            if constexpr (k1 > 16) x[k1] = cmul_conj(x[k1], tw[tws_set_of(k1)][tws_slot_of(k1)]);
        });
    }, [&](auto St) {
        static_for<0, 4>([&](auto P) {
            constexpr int k1 = tws_group(St.value) + 8 * P.value;
            lds_st8(c.col + 34 * k1, x[k1]);
        });
    });
}
// below: the groups in their own order, the four twiddles of a group read one group ahead
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_f2_tail_plain(const K1Thread &c, v2f (&x)[32], typename K1Cfg<LOG2N, RG>::Hv &hv,
                                                 const typename K1Cfg<LOG2N, RG>::Twr &twr CSDR_STAMP_PARAMS)
{
    v2f tw[2][4];
    static_for<1, 4>([&](auto P) { tw[0][P.value] = k1_pass_tw<LOG2N, RG, 8 * P.value>(c, twr); });
    CSDR_SB();
    CSDR_STAMP(8);                             // F2 middle stage
    one_group_behind_st8<8>([&](auto Ii) {
        constexpr int i = Ii.value;
        if constexpr (i < 7)                       // twiddles of the next group
            static_for<0, 4>([&](auto P) { tw[(i + 1) & 1][P.value] = k1_pass_tw<LOG2N, RG, i + 1 + 8 * P.value>(c, twr); });
        if constexpr (!RG) { k1_fetch_h<LOG2N, 2 * i>(c, hv); k1_fetch_h<LOG2N, 2 * i + 1>(c, hv); }
        dit_tail<i, 32, +1>(x);
        static_for<0, 4>([&](auto P) {
            constexpr int k1 = i + 8 * P.value;
            if constexpr (k1 != 0) x[k1] = cmul(x[k1], tw[i & 1][P.value]);
        });
    }, [&](auto Ii) {
        static_for<0, 4>([&](auto P) {
            constexpr int k1 = Ii.value + 8 * P.value;
            lds_st8(c.col + 34 * k1, x[k1]);
        });
    });
}
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_pass_f2(const K1Thread &c, v2f (&x)[32], typename K1Cfg<LOG2N, RG>::Hv &hv,
                                           const typename K1Cfg<LOG2N, RG>::Twr &twr CSDR_STAMP_PARAMS)
{
    // the four points of head group g (network positions 4g..4g+3 <- rows bitrev(4g+q)); three groups
    // ahead of the butterflies (lgkmcnt counts to 15)
    auto fetch = [&](auto Gg) {
        static_for<0, 4>([&](auto Q) {
            constexpr int p = 4 * Gg.value + Q.value;
            x[p] = lds_ld8(c.col + 34 * bitrev<32>(p));
        });
    };
    static_for<0, 3>(fetch);
    CSDR_SB();
    static_for<0, 8>([&](auto Gg) {
        if constexpr (Gg.value + 3 < 8) fetch(int_c<Gg.value + 3>{});
        dit_head4<Gg.value, 32, +1>(x);
        if constexpr ((Gg.value & 1) == 1) CSDR_SB();
    });
    CSDR_STAMP(7);                             // F2 heads
    dit_single<8, 32, +1>(x);
    CSDR_SB();
    if constexpr (K1Cfg<LOG2N>::TWS) k1_f2_tail_shared<LOG2N, RG>(c, x, hv, twr CSDR_STAMP_ARGS);
    else k1_f2_tail_plain<LOG2N, RG>(c, x, hv, twr CSDR_STAMP_ARGS);
}

// ================= F3 + H + I1: points 32t..32t+31, registers only =================
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_pass_f3(const K1Thread &c, v2f (&x)[32], typename K1Cfg<LOG2N, RG>::Hv &hv, typename K1Cfg<LOG2N, RG>::Pv &pv)
{
    // forward: network position p <- point m2 = bitrev(p).  Rows q, q+4, q+8, q+12 of 16-byte pairs hold
    // the points {2q, 2q+1} + 8 {0,1,2,3}: exactly the inputs of head groups bitrev3(2q) and bitrev3(2q+1)
    v2f y[32];
    static_for<0, 4>([&](auto Q) {
        static_for<0, 4>([&](auto P) {
            constexpr int j = Q.value + 4 * P.value;
            const v4f v = *reinterpret_cast<const v4f *>(c.rowp + 2 * j);
            x[bitrev<32>(2 * j)] = v2f{v.x, v.y};
            x[bitrev<32>(2 * j + 1)] = v2f{v.z, v.w};
        });
    });
    CSDR_SB();
    static_for<0, 4>([&](auto Q) {
        dit_head4<bitrev<8>(2 * Q.value), 32, +1>(x);
        dit_head4<bitrev<8>(2 * Q.value + 1), 32, +1>(x);
        CSDR_SB();
    });
    dit_single<8, 32, +1>(x);
    CSDR_SB();
    // tail group i finishes the bins k2 = i, i+8, i+16, i+24 -- the four inputs (network positions
    // 4g..4g+3, g = bitrev3(i), position 4g + 2 q1 + q0 <- k2 = i + 8 q1 + 16 q0) of the inverse's head
    // group g: multiply by H (folded into that group's first butterflies) and go straight on
    static_for<0, 8>([&](auto Ii) {
        constexpr int i = Ii.value, g = bitrev<8>(i);
        dit_tail_sel<K1Cfg<LOG2N, RG>::R4, i, 32, +1>(x);
        // times H: the products of the odd inputs ride in the FMA butterflies of the inverse's first stage
        y[4 * g] = x[i]; y[4 * g + 1] = x[i + 16]; y[4 * g + 2] = x[i + 8]; y[4 * g + 3] = x[i + 24];
        if constexpr (RG)
            dit_head4_gain<g, 32, -1>(y, v2f{pv[i].x, pv[i].y}, v2f{pv[i].z, pv[i].w});
        else
            dit_head4_tw<g, 32, -1>(y, v2f{hv[2 * i].x, hv[2 * i].y}, v2f{hv[2 * i].z, hv[2 * i].w},
                                    v2f{hv[2 * i + 1].x, hv[2 * i + 1].y}, v2f{hv[2 * i + 1].z, hv[2 * i + 1].w});
        if constexpr ((i & 1) == 1) CSDR_SB();
    });
#pragma unroll
    for (int i = 0; i < 32; i++) x[i] = y[i];
    CSDR_PRIO(1);
    dit_single<8, 32, -1>(x);
    CSDR_SB();
    v4f wv[16];
    one_group_behind<4>([&](auto Q) {
        constexpr int q = Q.value;
        dit_tail_sel<K1Cfg<LOG2N, RG>::R4, 2 * q, 32, -1>(x);
        dit_tail_sel<K1Cfg<LOG2N, RG>::R4, 2 * q + 1, 32, -1>(x);
        static_for<0, 4>([&](auto P) {
            constexpr int j = q + 4 * P.value;
            wv[j] = store_operand(x[2 * j], x[2 * j + 1]);
        });
    }, [&](auto Q) {
        static_for<0, 4>([&](auto P) {
            constexpr int j = Q.value + 4 * P.value;
            *reinterpret_cast<v4f *>(c.rowp + 2 * j) = wv[j];
        });
    });
}

// ================= I2: conj twiddle, radix-32 DIT inverse =================
// N = 16384: points of the head group of step s (g = bitrev3(tws_group(s)): rows k1 = i, i + 16, i + 8, i + 24 at positions
// 4g ... 4g + 3) and the twiddle set the step opens, two steps ahead of the butterflies; rows up to 16 take the
// conjugate twiddle, rows from 17 twiddle 32 - k1 as it is
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_i2_head_shared(const K1Thread &c, v2f (&x)[32], const typename K1Cfg<LOG2N, RG>::Twr &twr)
{
    v2f tw[5][4];
    auto fetch = [&](auto St) {
        constexpr int s = St.value, g = bitrev<8>(tws_group(s));
        static_for<0, 4>([&](auto Q) {
            constexpr int r = 4 * g + Q.value;
            x[r] = lds_ld8(c.col + 34 * bitrev<32>(r));
        });
        if constexpr (tws_opens(s))
            static_for<0, 4>([&](auto Q) {
                constexpr int row = tws_row(tws_set(s), Q.value);
                if constexpr (row != 0) tw[tws_set(s)][Q.value] = k1_pass_tw<LOG2N, RG, row>(c, twr);
            });
    };
    static_for<0, 2>(fetch);
    CSDR_SB();
    static_for<0, 8>([&](auto St) {
        constexpr int s = St.value, i = tws_group(s), g = bitrev<8>(i);
        if constexpr (s + 2 < 8) fetch(int_c<s + 2>{});
        constexpr int ka = i == 0 ? 8 : i, kb = i + 16, kc = i + 8, kd = i + 24;      // (group 0: position 0 is plain)
        dit_head4_seltw<g, 32, -1, i == 0, (ka <= 16), (kb <= 16), (kc <= 16), (kd <= 16)>(
            x, tw[tws_set_of(ka)][tws_slot_of(ka)], tw[tws_set_of(kb)][tws_slot_of(kb)],
            tw[tws_set_of(kc)][tws_slot_of(kc)], tw[tws_set_of(kd)][tws_slot_of(kd)]);
        if constexpr ((s & 1) == 1) CSDR_SB();
    });
}
// below: points and twiddles of head group g, two groups ahead of the butterflies
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_i2_head_plain(const K1Thread &c, v2f (&x)[32], const typename K1Cfg<LOG2N, RG>::Twr &twr)
{
    v2f tw[32];
    auto fetch = [&](auto Gg) {
        static_for<0, 4>([&](auto Q) {
            constexpr int r = 4 * Gg.value + Q.value;
            x[r] = lds_ld8(c.col + 34 * bitrev<32>(r));
        });
        static_for<0, 4>([&](auto Q) {
            constexpr int r = 4 * Gg.value + Q.value;
            if constexpr (r != 0) tw[r] = k1_pass_tw<LOG2N, RG, bitrev<32>(r)>(c, twr);
        });
    };
    static_for<0, 2>(fetch);
    CSDR_SB();
    static_for<0, 8>([&](auto Gg) {
        constexpr int g = Gg.value;
        if constexpr (g + 2 < 8) fetch(int_c<g + 2>{});
        dit_head4_conjtw<g, 32, -1, g == 0>(x, tw[4 * g], tw[4 * g + 1], tw[4 * g + 2], tw[4 * g + 3]);
        if constexpr ((g & 1) == 1) CSDR_SB();
    });
}
template <int LOG2N, bool RG> __device__ __forceinline__ void k1_pass_i2(const K1Thread &c, v2f (&x)[32], const typename K1Cfg<LOG2N, RG>::Twr &twr)
{
    if constexpr (K1Cfg<LOG2N>::TWS) k1_i2_head_shared<LOG2N, RG>(c, x, twr);
    else k1_i2_head_plain<LOG2N, RG>(c, x, twr);
    dit_single<8, 32, -1>(x);
    CSDR_SB();
    one_group_behind_st8<8>([&](auto I) { dit_tail_sel<K1Cfg<LOG2N, RG>::R4, I.value, 32, -1>(x); }, [&](auto I) {
        static_for<0, 4>([&](auto P) {
            constexpr int n1 = I.value + 8 * P.value;
            lds_st8(c.col + 34 * n1, x[n1]);
        });
    });
}

// ================= I3: conj twiddle, radix-R0 DIT inverse, store the valid half =================
// sample 1024*n1 + column, n1 >= HALF  ->  output offset 1024*(n1-HALF) + column
// N = 16384
template <int LOG2N, bool RG> __device__ __forceinline__ void k1_i3_rows16(const K1Thread &c, int b, typename K1Cfg<LOG2N>::Y &y)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int R0 = Cfg::R0, L = Cfg::L;
    v4f sv[8];
    one_group_behind<R0 / 4>([&](auto I) {
        constexpr int i = I.value;
        if constexpr (RG) {
            // the scale by P left out the response's delay of N/4 samples: output row n1 is row n1 + 4
            dit_tail_middle_sel<K1Cfg<LOG2N, RG>::R4, i, R0, -1>(y[0]);     // only rows 4..11 of the inverse transform are kept
            dit_tail_middle_sel<K1Cfg<LOG2N, RG>::R4, i, R0, -1>(y[1]);
            sv[2 * i] = store_operand(y[0][i + 4], y[1][i + 4]);
            sv[2 * i + 1] = store_operand(y[0][i + 8], y[1][i + 8]);
        } else {
            dit_tail_upper<i, R0, -1>(y[0]);      // only rows 8..15 of the inverse transform are kept
            dit_tail_upper<i, R0, -1>(y[1]);
            sv[2 * i] = store_operand(y[0][i + 8], y[1][i + 8]);
            sv[2 * i + 1] = store_operand(y[0][i + 12], y[1][i + 12]);
        }
    }, [&](auto I) {
        constexpr int i = I.value;
        k1_store_out<LOG2N>(c, c.voff, b * (L * 8) + i * 8192, sv[2 * i]);
        k1_store_out<LOG2N>(c, c.voff, b * (L * 8) + (i + 4) * 8192, sv[2 * i + 1]);
    });
}
// N = 2048: the kept half is the butterfly's difference output, row 1 = y0 - conj(w) y1; group i = pairs 2i, 2i + 1
template <int LOG2N> __device__ __forceinline__ void k1_i3_rows2(const K1Thread &c, int b, typename K1Cfg<LOG2N>::Y &y)
{
    using Cfg = K1Cfg<LOG2N>;
    v4f sv[8], wq[8];
    static_for<0, 8>([&](auto PP) { wq[PP.value] = k1_w_pair<LOG2N>(c, PP.value); });
    one_group_behind<4>([&](auto I) {
        static_for<0, 2>([&](auto Q) {
            constexpr int pp = 2 * I.value + Q.value;
            const v2f d0 = y[2 * pp][0] - cmul_conj(y[2 * pp][1], v2f{wq[pp].x, wq[pp].y});
            const v2f d1 = y[2 * pp + 1][0] - cmul_conj(y[2 * pp + 1][1], v2f{wq[pp].z, wq[pp].w});
            sv[pp] = store_operand(d0, d1);
        });
    }, [&](auto I) {
        static_for<0, 2>([&](auto Q) {
            constexpr int pp = 2 * I.value + Q.value;
            k1_store_out<LOG2N>(c, c.voff + pp * Cfg::PSTEP_B, b * (Cfg::L * 8), sv[pp]);
        });
    });
}
// only the upper half of the inverse transform is kept (fastfir.cpp:291-300).  N = 8192: the last stage's
// difference outputs, rows 4..7, group i = row 4 + i; N = 4096: rows 2, 3 of the head group's radix-4
// transform, group i = row 2 + i
template <int LOG2N> __device__ __forceinline__ void k1_i3_rows84(const K1Thread &c, int b, typename K1Cfg<LOG2N>::Y &y)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int R0 = Cfg::R0, G = Cfg::G, HALF = Cfg::HALF, NG = HALF;
    v4f sv[8];                                     // (HALF rows) x (G / 2 column pairs)
    one_group_behind<NG>([&](auto I) {
        constexpr int i = I.value;
        if constexpr (R0 == 8)
            static_for<0, G>([&](auto E) { bfly_dit_lower<4 * i, -1>(y[E.value][i], y[E.value][i + 4]); });
        static_for<0, G / 2>([&](auto PP) {
            sv[i * (G / 2) + PP.value] = store_operand(y[2 * PP.value][HALF + i], y[2 * PP.value + 1][HALF + i]);
        });
    }, [&](auto I) {
        static_for<0, G / 2>([&](auto PP) {
            k1_store_out<LOG2N>(c, c.voff + PP.value * Cfg::PSTEP_B, b * (Cfg::L * 8) + I.value * 8192, sv[I.value * (G / 2) + PP.value]);
        });
    });
}
template <int LOG2N, bool RG>
__device__ __forceinline__ void k1_pass_i3(const K1Thread &c, int b, typename K1Cfg<LOG2N>::W1 &w1, typename K1Cfg<LOG2N>::Pw &pw)
{
    using Cfg = K1Cfg<LOG2N>;
    constexpr int R0 = Cfg::R0, G = Cfg::G;
    typename Cfg::Y y;
    static_for<0, R0>([&](auto Rr) {
        constexpr int r = Rr.value, k0 = bitrev<R0>(r);
        static_for<0, G / 2>([&](auto PP) {
            const v4f v = *reinterpret_cast<const v4f *>(c.outer + Cfg::OUTER_ROW * k0 + Cfg::PSTEP_LDS * PP.value);
            y[2 * PP.value][r] = v2f{v.x, v.y};
            y[2 * PP.value + 1][r] = v2f{v.z, v.w};
        });
    });
    if constexpr (R0 > 2) {
        if constexpr (!Cfg::W1_RESIDENT) k1_load_w1<LOG2N>(c, w1);
        if constexpr (!K1Cfg<LOG2N, RG>::PW_RESIDENT) {
#pragma unroll
            for (int e = 0; e < G; e++) twiddle_powers<Cfg::PWN>(opaque(w1[e]), pw[e]);     // while the reads are in flight
        }
        CSDR_SB();
        static_for<0, (R0 >= 8 ? R0 / 4 : 1)>([&](auto Gg) {
            constexpr int g = Gg.value;
            static_for<0, G>([&](auto E) {
                constexpr int e = E.value;
                if constexpr (R0 == 16) {
                    // position 4g + q holds row k0 = bitrev(4g + q): rows above R0 / 2 take power R0 - k0 as it is
                    constexpr int ka = bitrev<R0>(4 * g), kb = bitrev<R0>(4 * g + 1), kc = bitrev<R0>(4 * g + 2), kd = bitrev<R0>(4 * g + 3);
                    constexpr int H0 = R0 / 2;
                    dit_head4_seltw<g, R0, -1, g == 0, (ka <= H0), (kb <= H0), (kc <= H0), (kd <= H0)>(
                        y[e], pw[e][ka <= H0 ? ka : R0 - ka], pw[e][kb <= H0 ? kb : R0 - kb],
                        pw[e][kc <= H0 ? kc : R0 - kc], pw[e][kd <= H0 ? kd : R0 - kd]);
                } else
                    dit_head4_conjtw<g, R0, -1, g == 0>(y[e], pw[e][bitrev<R0>(4 * g)], pw[e][bitrev<R0>(4 * g + 1)],
                                                        pw[e][bitrev<R0>(4 * g + 2)], pw[e][bitrev<R0>(4 * g + 3)]);
            });
            if constexpr ((g & 1) == 1) CSDR_SB();
        });
    }
    CSDR_PRIO(2);
    if constexpr (R0 == 16) k1_i3_rows16<LOG2N, RG>(c, b, y);
    else if constexpr (R0 == 2) k1_i3_rows2<LOG2N>(c, b, y);
    else k1_i3_rows84<LOG2N>(c, b, y);
}

template <int LOG2N, bool RG> __device__ __forceinline__ void fastfir_os2_body(const FastFirArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_FF);
    using Cfg = K1Cfg<LOG2N, RG>;
    constexpr int N = Cfg::N, T = Cfg::TV, G = Cfg::G, L = Cfg::L, HALF = Cfg::HALF, VW = Cfg::VW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int t = VW == 1 ? (int)threadIdx.x : (int)threadIdx.x % T, vw = VW == 1 ? 0 : (int)threadIdx.x / T;
    v2f *lds = reinterpret_cast<v2f *>(smem_raw) + vw * Cfg::Base::LDS_DATA;
    v2f *tw2 = reinterpret_cast<v2f *>(smem_raw) + VW * Cfg::Base::LDS_DATA;     // tw2[k1*32 + n2] = W_1024^{n2*k1}
    if constexpr (VW > 1) {                   // (a virtual workgroup that has nothing to do leaves below: the table is whole first)
        for (int i = threadIdx.x; i < 1024; i += VW * T) tw2[i] = a.tw2[i];
        __syncthreads();
    }

    int wg = blockIdx.x * VW + vw, ch, run;
    if ((a.channels & 7) == 0) {
        int xcd = wg & 7, slot = wg >> 3;
        ch = (slot / a.runs) * 8 + xcd;
        run = slot % a.runs;
    } else {
        ch = wg / a.runs;
        run = wg % a.runs;
    }
    const int b0 = run * a.blocks_per_run;
    int b1 = b0 + a.blocks_per_run;
    if (b1 > a.nblocks) b1 = a.nblocks;
    // VW == 2 (N = 4096): the two virtual workgroups of a real one share its s_barrier, and one of them may END here -- or
    // walk one block fewer in the last run -- while the other keeps arriving at barriers.  That is defined on this target:
    // the gfx9 barrier counts the waves of the workgroup that have not terminated (an s_endpgm wave leaves the count), so
    // the survivor's barriers complete with its own waves.  The HIP model does not promise it, the build pins the target:
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "fastfir_os2_kernel<12> relies on gfx950's s_barrier ignoring terminated waves (two virtual workgroups per workgroup)"
#endif
    if (ch >= a.channels || b0 >= b1) return;          // uniform per (virtual) workgroup

    // K1_PROLOGUE: the table's words are fetched with everything else and written behind the powers (tw2_words)
    if constexpr (VW == 1 && Cfg::TW2_LDS && !Cfg::PROLOGUE)
        for (int i = t; i < 1024; i += T) tw2[i] = a.tw2[i];

    K1Thread c;
    c.t = t; c.tw1 = a.tw1; c.nblocks = a.nblocks;
    c.r_in = make_rsrc(a.in + (long)ch * a.in_stride, (unsigned)a.nblocks * L * 8u);
    const rsrc_t r_hist = make_rsrc(a.hist + (long)ch * L, L * 8u);
    c.r_out = make_rsrc(a.out + (long)ch * a.out_stride, (unsigned)a.nblocks * L * 8u);
    c.r_h = make_rsrc(a.h + (long)ch * a.h_stride, N * 8u);
    const rsrc_t r_g = make_rsrc(a.gain + (long)ch * (a.h_stride / 2), N * 4u);      // (RG; half of H's bytes per filter)
    c.voff = t * 16;
    if constexpr (Cfg::RUNEND) {
        c.in = a.in + (long)ch * a.in_stride; c.in_bytes = (unsigned)a.nblocks * L * 8u; c.run_end = b1;
        c.r_hn = make_rsrc(a.hist_next + (long)ch * L, L * 8u);
    }

    typename Cfg::W1 w1;
    k1_load_w1<LOG2N>(c, w1);
    typename Cfg::Pw pw;
    // K1_PROLOGUE: the powers are built behind the LAST load of this prologue, not here.  Everything the run needs is then
    // asked for before the first wait, the base twiddles first: the vector-memory counter retires loads in the order of
    // issue, so the powers wait for these alone and are built while the samples are in flight.  Before: base twiddles,
    // wait, powers, and only then the rest -- two round trips at the one moment every workgroup of the launch asks at once
    v2f tw2_words[1024 / T];
    if constexpr (Cfg::PROLOGUE) {
        if constexpr (Cfg::TW2_LDS) {
#pragma unroll
            for (int i = 0; i < 1024 / T; i++) tw2_words[i] = a.tw2[t + i * T];
        }
        CSDR_SB();
    }
    if constexpr (Cfg::R0 > 2 && !Cfg::PROLOGUE) {
#pragma unroll
        for (int e = 0; e < G; e++) twiddle_powers<Cfg::PWN>(opaque(w1[e]), pw[e]);
    }

    // H: the first K1_HREG of this thread's sixteen float4 stay in registers for the whole run -- all the registers the
    // kernel has to spare: a 1 KB fetch from L2 costs about as much energy as four packed instructions -- the rest is
    // fetched from L2 for every block (k1_fetch_h).  RG: all eight float4 of gains stay
    typename Cfg::Hv hv;
#pragma unroll
    for (int j = 0; j < Cfg::HREG; j++) hv[j] = buf_load16(c.r_h, t * 16, j * (T * 16));
    typename Cfg::Pv pv;
    if constexpr (RG) {
#pragma unroll
        for (int i = 0; i < 8; i++) pv[i] = buf_load16(r_g, t * 16, i * (T * 16));
    }
#ifdef K1_ABLATE
    c.habl = v4f{1.0f, 0.0f, 1.0f, 0.0f};
    asm volatile("" : "+v"(c.habl));
    c.twabl = v2f{0.8f, 0.6f};
    asm volatile("" : "+v"(c.twabl));
#endif
    v2f x[32];           // passes F2 ... I2: the 32 points of this thread
    // The two halves of a block's input.  The new half of one block is the old half of the next: the block loop is
    // unrolled by two and the buffers swap roles, so nothing is copied; the samples after next are fetched into the old
    // half's registers as soon as the first butterfly stage has read them.
    K1Half hp, hq;
    if (b0 == 0) k1_load_half<LOG2N>(r_hist, c.voff, 0, hp.v);
    else k1_load_half<LOG2N>(c.r_in, c.voff, (b0 - 1) * (L * 8), hp.v);
    k1_load_half<LOG2N>(c.r_in, c.voff, b0 * (L * 8), hq.v);

    const int sb = t >> 5, sn = t & 31;       // sub-transform and column of passes F2 / I2
    c.col = lds + lds_pad(1024 * sb) + sn;
    c.twc = tw2 + sn;
    typename Cfg::Twr twr;
#pragma unroll
    for (int k1 = 1; k1 <= Cfg::TWREG; k1++) twr[k1 - 1] = a.tw2[32 * k1 + sn];
    if constexpr (Cfg::PROLOGUE) {
        CSDR_SB();
#pragma unroll
        for (int e = 0; e < G; e++) twiddle_powers<Cfg::PWN>(opaque(w1[e]), pw[e]);
        if constexpr (Cfg::TW2_LDS) {
#pragma unroll
            for (int i = 0; i < 1024 / T; i++) tw2[t + i * T] = tw2_words[i];
        }
    }
    c.rowp = lds + 34 * t;
    c.outer = lds + lds_pad(2 * t);

#ifdef K1_CYC          // diagnostic build (tools/k1_cycles.py): shader cycles and real time of the whole block loop
    const unsigned long long cyc0_ = __builtin_amdgcn_s_memtime(), rt0_ = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef CSDR_K1_STAMPS
    unsigned long long acc_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(last_)::"memory");
#endif
    // one block: [oldh | newh] in, the valid half out; block b+1's new half is left in oldh
    auto one_block = [&](const int b, K1Half &oldh, K1Half &newh) {
        CSDR_SB();
        CSDR_PRIO(1);
        // K1_LDSPREAD: quarter Q of the next new half, asked for at the head of a later pass (into registers F1 has read)
        auto spread = [&](auto Q) {
            if constexpr (Cfg::LDSPREAD) {
                const K1Next nx = k1_next_half<LOG2N>(c, b);
                k1_load_half<LOG2N, Q.value * (HALF / 4), (Q.value + 1) * (HALF / 4)>(nx.r, c.voff, nx.soff, oldh.v);
                CSDR_SB();
            }
        };
        k1_pass_f1<LOG2N, RG>(c, b, oldh, newh, pw);
        CSDR_STAMP(0);                             // F1 (and the loop-carried moves)
        k1_block_barrier<LOG2N>();
        CSDR_STAMP(1);                             // barrier after F1
        CSDR_PRIO(3);
        spread(int_c<0>{});
        k1_pass_f2<LOG2N, RG>(c, x, hv, twr CSDR_STAMP_ARGS);
        CSDR_STAMP(2);                             // F2
        wave_sync();                                   // F2 -> F3 stays inside the half-wave that owns sub-transform sb
        CSDR_PRIO(2);
        spread(int_c<1>{});
        k1_pass_f3<LOG2N, RG>(c, x, hv, pv);
        CSDR_STAMP(3);                             // F3 + H + I1
        wave_sync();
        CSDR_PRIO(0);
        spread(int_c<2>{});
        k1_pass_i2<LOG2N, RG>(c, x, twr);
        CSDR_STAMP(4);                             // I2
        k1_block_barrier<LOG2N>();
        CSDR_STAMP(5);                             // barrier after I2
        CSDR_PRIO(3);
        spread(int_c<3>{});
        k1_pass_i3<LOG2N, RG>(c, b, w1, pw);
        CSDR_STAMP(6);                             // I3
    };
    // Everything fetched so far (both input halves, the resident part of H) is waited for HERE, once: left to the
    // compiler the wait sits at the loop header ("vmcnt(7) ... vmcnt(0)" in front of F1's first butterflies), where
    // on the back edge the eight youngest vector-memory operations are the output stores of the block just finished.
    __builtin_amdgcn_s_waitcnt(0x0f70);          // vmcnt(0); lgkmcnt / expcnt left alone (gfx9 encoding)
    int b = b0;
    for (; b + 1 < b1; b += 2) {
        one_block(b, hp, hq);
        one_block(b + 1, hq, hp);
    }
    const bool odd_tail = b < b1;                // uniform per workgroup: a run with an odd number of blocks
    if (odd_tail) one_block(b, hp, hq);

#ifdef K1_CYC
    if (a.dbg && t == 0) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(a.dbg) + (long)blockIdx.x * 2;
        o[0] = __builtin_amdgcn_s_memtime() - cyc0_;
        o[1] = __builtin_amdgcn_s_memrealtime() - rt0_;
    }
#endif
#ifdef CSDR_K1_STAMPS
    if (a.dbg && (c.t & 63) == 0) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(a.dbg) + ((long)blockIdx.x * (T / 64) + (c.t >> 6)) * 16;
        for (int i = 0; i < 16; i++) o[i] = acc_[i];
    }
#endif
    // the tail of this call's input is the overlap of the next call (fastfir.cpp:280-300);
    // written to the other half of the ping-pong history so no workgroup can still be reading it
    // (K1_RUNEND: the call's last block has stored it, k1_pass_f1)
    if constexpr (!Cfg::RUNEND) if (b1 == a.nblocks) {
        const rsrc_t r_hn = make_rsrc(a.hist_next + (long)ch * L, L * 8u);
        v4f sv[8];
#pragma unroll
        for (int n1 = 0; n1 < HALF; n1++)      // the last new half: in hp after a pair of blocks, in hq after a single one
#pragma unroll
            for (int pp = 0; pp < G / 2; pp++)
                sv[n1 * (G / 2) + pp] = odd_tail ? store_operand(hq.v[(2 * pp) * HALF + n1], hq.v[(2 * pp + 1) * HALF + n1])
                                                 : store_operand(hp.v[(2 * pp) * HALF + n1], hp.v[(2 * pp + 1) * HALF + n1]);
        CSDR_STORE_GROUP_BEGIN();
#pragma unroll
        for (int n1 = 0; n1 < HALF; n1++)
#pragma unroll
            for (int pp = 0; pp < G / 2; pp++) buf_store16(r_hn, c.voff + pp * Cfg::PSTEP_B, n1 * 8192, sv[n1 * (G / 2) + pp]);
        CSDR_STORE_GROUP_END();
    }
}


// fastfir_os2_kernel<14> runs on real gains (a.gain); fastfir_os2h_kernel is the same size on complex H, for responses
// that are not the library's own design (a.gain null)
template <int LOG2N>
__global__ __launch_bounds__(K1Cfg<LOG2N>::T) __attribute__((amdgpu_waves_per_eu(2, 2)))
void fastfir_os2_kernel(FastFirArgs a)
{
    fastfir_os2_body<LOG2N, LOG2N == 14>(a);
}
__global__ __launch_bounds__(K1Cfg<14>::T) __attribute__((amdgpu_waves_per_eu(2, 2)))
void fastfir_os2h_kernel(FastFirArgs a)
{
    fastfir_os2_body<14, false>(a);
}

template <int LOG2N>
static hipError_t launch2_one(const FastFirArgs &a, hipStream_t stream, int *which)
{
    using Cfg = K1Cfg<LOG2N>;
    void (*kernel)(FastFirArgs) = &fastfir_os2_kernel<LOG2N>;
    if (LOG2N == 14 && !a.gain) kernel = &fastfir_os2h_kernel;
    // (the one instantiation whose body runs on real gains: fastfir_os2_kernel<14>)
    if (which) *which = (LOG2N == 14 && kernel != &fastfir_os2h_kernel) ? FASTFIR_KERNEL_PIPELINED_GAIN : FASTFIR_KERNEL_PIPELINED_H;
    // once per device and kernel (the attribute belongs to the device, and a process may drive several): the per-launch
    // call cost the per-datagram host form microseconds
    // (the real-gain kernel reserves no twiddle table where it reads none: K1Cfg::TW2_LDS)
    const int lds_bytes = kernel == &fastfir_os2h_kernel ? Cfg::LDS_BYTES : K1Cfg<LOG2N, LOG2N == 14>::LDS_BYTES;
    hipError_t e = kernel == &fastfir_os2h_kernel ? CSDR_MAX_LDS_ONCE(&fastfir_os2h_kernel, Cfg::LDS_BYTES)
                                                  : CSDR_MAX_LDS_ONCE(&fastfir_os2_kernel<LOG2N>, (K1Cfg<LOG2N, LOG2N == 14>::LDS_BYTES));
    if (e != hipSuccess) return e;
#ifdef CSDR_WG_TRACE
    FastFirArgs b = a;
    b.trace = wgtrace_next();
    hipLaunchKernelGGL(kernel, dim3((a.channels * a.runs + Cfg::VW - 1) / Cfg::VW), dim3(Cfg::T), lds_bytes, stream, b);
    return hipGetLastError();
#endif
    hipLaunchKernelGGL(kernel, dim3((a.channels * a.runs + Cfg::VW - 1) / Cfg::VW), dim3(Cfg::T), lds_bytes, stream, a);
    return hipGetLastError();
}

hipError_t fastfir2_launch(int log2n, const FastFirArgs &a, hipStream_t stream, int *kernel)
{
    switch (log2n) {
    case 11: return launch2_one<11>(a, stream, kernel);
    case 12: return launch2_one<12>(a, stream, kernel);
    case 13: return launch2_one<13>(a, stream, kernel);
    case 14: return launch2_one<14>(a, stream, kernel);
    default: return hipErrorInvalidValue;
    }
}

int fastfir2_twreg() { return K1_TWREG; }
int fastfir2_radix4() { return K1Cfg<14, true>::R4 ? 1 : 0; }
int fastfir2_pwres() { return K1Cfg<14, true>::PW_RESIDENT ? 1 : 0; }
// bit 0: K1_RUNEND, 1: K1_PROLOGUE, 2: the real-gain kernel keeps no twiddle table in LDS (K1_TW2LDS and K1_TWREG = 16), 3: K1_LDSPREAD
int fastfir2_hbm_knobs()
{
    using Cfg = K1Cfg<14, true>;
    return (Cfg::RUNEND ? 1 : 0) | (Cfg::PROLOGUE ? 2 : 0) | (Cfg::TW2_LDS ? 0 : 4) | (Cfg::LDSPREAD ? 8 : 0);
}
int fastfir2_gain_lds_bytes() { return K1Cfg<14, true>::LDS_BYTES; }

// Host mirror of the kernel's index algebra: thread t of pass F3 owns k0 = t >> 5 (sub-transform) and k1 = t & 31
// (its row), and consumes H in the order its tail groups finish bins: float4 j = 2 i + h of thread t, half e,
// multiplies k2 = i + 8 h + 16 e; natural bin k = k0 + R0 (k1 + 32 k2), R0 = N / 1024 sub-transforms.
int fastfir2_bin_of(int log2n, int t, int j, int e)
{
    const int R0 = (1 << log2n) / 1024;
    const int i = j >> 1, h = j & 1;
    const int k2 = i + 8 * h + 16 * e;
    return (t >> 5) + R0 * ((t & 31) + 32 * k2);
}
// ... and of the real gains: float4 i of thread t holds, in the order I1's head group takes them, the gains of the bins
// k2 = i, i + 16, i + 8, i + 24 -- the halves of H's float4 2 i and 2 i + 1
int fastfir2_gain_bin_of(int log2n, int t, int i, int c)
{
    return fastfir2_bin_of(log2n, t, 2 * i + (c >> 1), c & 1);
}

// The shared twiddles of the 16384-point kernels (2: rows k1 and 32 - k1 of F2 / I2 and rows k0 and 16 - k0 of the outer pass;
// the builds 0 and 1 are retired, HISTORY.md).  The two orders above say where a bin's multiplier sits when every row runs
// on its own twiddle.  A row of F3 that ran on a shared one (k1 = t & 31 from 17 up, N = 16384) has its 32 outputs one bin
// on: index k2 holds bin k2 - *inner (mod 32).  *outer is the same shift of a whole 1024-point sub-transform by the outer
// pass: sub-transforms k0 = t >> 5 from 9 up at N = 16384 hold sub-bin k1 + 32 (k2 - *inner) - *outer (mod 1024).  Both are 0
// at the smaller sizes.
int fastfir2_twshare() { return 2; }
void fastfir2_twshare_shift(int log2n, int t, int *inner, int *outer)
{
    *inner = (log2n == 14 && (t & 31) >= 17) ? 1 : 0;
    *outer = (log2n == 14 && (t >> 5) > 8) ? 1 : 0;
}
// ... and composed with them: the natural bin whose multiplier belongs in H slot (t, j, e) / gain slot (t, i, c) -- what
// the uploads (capi_fastfir.hip: perm2 / permg, host and device design alike) are built from
int fastfir2_slot_bin(int log2n, int t, int j, int e)
{
    const int R0 = (1 << log2n) / 1024;
    int inner, outer;
    fastfir2_twshare_shift(log2n, t, &inner, &outer);
    const int k2 = ((j >> 1) + 8 * (j & 1) + 16 * e - inner) & 31;
    const int sub = ((t & 31) + 32 * k2 - outer) & 1023;           // bin of the 1024-point sub-transform t >> 5
    return (t >> 5) + R0 * sub;
}
int fastfir2_gain_slot_bin(int log2n, int t, int i, int c)
{
    return fastfir2_slot_bin(log2n, t, 2 * i + (c >> 1), c & 1);
}

}  // namespace csdr

