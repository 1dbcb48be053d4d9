// downconv_kernel.hpp -- NCO mixer + decimate-by-2^n cascade for gfx950 (K2 in DESIGN.md).
//
// Replaces CDownConvert::ProcessData (reference dsp/downconvert.cpp:186-263): the gain-stabilised
// rotating-phasor NCO (:210-216) and the chain of CIC-3 (:444-460), fixed 11-tap (:348-423) and
// generic 15..51-tap (:286-320) half-band decimators picked by SetDataRate (:114-173), batched
// over many channels and fused into ONE pass over HBM: 8 B read per input sample, 8 B written
// per output sample, every intermediate rate lives in LDS.
//
// Every stage is the FIR  y[j] = sum_k h[k] xe[2j+k],  xe = [stage history | stage input]
// (SURVEY App. A.3), so the cascade is a pure feed-forward function of the mixed input stream
// and can be cut anywhere: a workgroup owns one segment of one channel, rebuilds the stage
// histories by running the W >= sum_s (L_s-1) 2^s samples in front of its segment through the
// cascade (outputs discarded), then walks its segment tile by tile with the histories carried
// in LDS.  Segment 0 warms up from the W mixed samples the previous call left behind.
//
// NCO: the reference phasor is e^{j(phi0+(n+1)delta)} times the amplitude a_n of the recurrence
// a_{n+1} = a_n (1.95 - a_n^2), a_0 = 1 (-> sqrt(0.95)).  Here the phase is a 64-bit fixed-point
// accumulator (exact per-sample phase, no drift), re-anchored with an accurate sincospi every
// 16 rows and advanced by one complex multiply per row in between; a_n comes from a 512-entry
// table for a channel's first samples and is constant afterwards.
//
// The file reads top down: the plan and its LDS image, the stage arithmetic, the state a tile's steps share
// (DcWave, DcNco, DcTileIn), one function per step of a tile, the two kinds of tile, the kernel, the launch.
#pragma once
#include "fft_core.hpp"
#include "launch_once.hpp"
#include "downconv_kernels.h"
#include "../../include/csdr_hb_taps.h"

namespace csdr {

constexpr int DC_T = 64;                  // threads per workgroup
constexpr int DC_ROW = 2 * DC_T;           // samples per row (16 B per lane)
constexpr int DC_TILE = 512;              // input samples per tile
constexpr int DC_NR = DC_TILE / DC_ROW;    // rows per tile
constexpr int DC_ANCHOR_ROWS = 16;
typedef float f4a8 __attribute__((ext_vector_type(4), aligned(8)));   // a 16-byte load from an 8-byte aligned address

// ---- the cascade as a compile-time plan ----------------------------------------------------------------
// SetDataRate's stage sequences are few in practice (CIC-3s, then 11-tap half bands, then one to three longer
// ones: tools/list_dc_plans.py), and a kernel that knows its sequence needs no stage dispatch, no layout words
// in registers, no lane predicates in the passes of a complete tile.  DcPlanT<kinds...> instantiates the kernel
// for one sequence (cutesdr_amd/_build.py compiles downconv_plan.hip once per listed plan); DcPlanDyn is the
// same kernel with everything taken at run time, for every other sequence (the pure mixer among them): for
// compile-time purposes it has no stages.
template <int... K> struct DcPlanT {
    static_assert(sizeof...(K) > 0, "the pure mixer runs on the run-time plan");
    static constexpr bool FIX = true;
    static constexpr int NS = sizeof...(K);
    static constexpr int KIND[sizeof...(K) + 1] = {K..., 0};
};
struct DcPlanDyn {
    static constexpr bool FIX = false;
    static constexpr int NS = 0;
    static constexpr int KIND[1] = {0};
};
constexpr int dc_hist_of(int kind) { return kind == 3 ? 2 : kind - 1; }
// pair coefficient q and centre coefficient of a stage kind, as dc_host.hpp's dc_make_plan stores them (fp32)
constexpr float dc_pair_coef(int kind, int q) { return kind == 3 ? (q == 0 ? 0.125f : 0.375f) : (float)csdr_hb_even[(kind - 11) / 4][q]; }
constexpr float dc_centre_coef(int kind) { return kind == 3 ? 0.f : 0.5f; }

// LDS image: region s = [even half | odd half] of xe_s = [history | stage-s input], region ns = tile outputs
struct DcLayout {
    int roff[DC_MAX_STAGES + 2];
    int ooff[DC_MAX_STAGES + 1];
    int slots;
};
constexpr DcLayout dc_layout_of(const int *kind, int ns)
{
    DcLayout l{};
    int o = 0;
    for (int s = 0; s <= ns; s++) {
        l.roff[s] = o;
        if (s < ns) {
            const int half = (dc_hist_of(kind[s]) / 2 + (DC_TILE >> (s + 1)) + 2) & ~1;    // + slack for the CIC's O[j+1]
            l.ooff[s] = half;
            o += 2 * half;
        } else {
            l.ooff[s] = 0;
            o += ((DC_TILE >> s) + 1) & ~1;
        }
    }
    l.slots = o;
    return l;
}

// The workgroup is ONE wave and the LDS unit executes a wave's instructions in issue order: a ds_read issued after a
// ds_write of the same wave sees the written data, whichever lane wrote it.  The hand-over between the steps of a
// tile therefore needs neither an s_waitcnt (it would make every step wait out the LDS write latency) nor an
// s_barrier; only the compiler must keep the program order of the LDS accesses.  (A wavefront-scope fence would
// do that too, but it also orders -- and so drains -- the global loads prefetched for the next tile.)
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}
static_assert(DC_T == 64, "lds_barrier() relies on a single-wave workgroup");

// the raw samples are read once: non-temporal loads keep them from displacing what the chip re-reads (K1 measured
// -1.2 % for the same change; here A/B'd with tools/bench_k2_plans.py)
__device__ __forceinline__ v4f dc_stream_load(const v4f *p) { return __builtin_nontemporal_load(p); }

// e^{j * 2*pi * phase/2^64}
__device__ __forceinline__ v2f phasor_of(unsigned long long phase)
{
    const float halfturns = (float)((int)(phase >> 32)) * 4.6566128730773926e-10f;   // 2^-31
    float s, c;
    sincospif(halfturns, &s, &c);
    return v2f{c, s};
}

// Per-stage parameters of the run-time plan and of short tiles, staged in LDS once per workgroup: the tap values
// are read from there (wide uniform reads), the layout words sit packed in two registers with stage s in lane s
// (v_readlane).
enum { DP_KIND = 0, DP_HIST2, DP_ROFF, DP_OOFF, DP_CC, DP_C0 = 8, DP_WORDS = 24 };   // rows of 96 B, taps 16-B aligned
typedef int DcParamRow[DP_WORDS];

// The arithmetic of one output, the same in every form of the stage (run-time plan, compiled plan, one or several
// outputs per lane): first product rounded on its own, then acc + (a + b) * c as one fused multiply-add per tap pair.
// Left to the compiler, "o * cc + (a + b) * c0" contracts into a fused multiply-add around EITHER product, depending on
// the code around it -- one-ulp differences between the forms; dc_first() keeps the first product out of that choice.
__device__ __forceinline__ v2f dc_first(v2f x, float c)
{
    v2f p = x * c;
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ v2f dc_mac(v2f acc, v2f a, v2f b, float c) { return acc + (a + b) * c; }
__device__ __forceinline__ v2f dc_cic(v2f e0, v2f o0, v2f e1, v2f o1, float c0, float c1)    // downconvert.cpp:453-454
{
    return dc_mac(dc_first(o0 + e1, c1), e0, o1, c0);
}

// One decimate-by-2 stage with the tap geometry fixed at compile time: L = 3 is the CIC-3
// (downconvert.cpp:444-460), otherwise an L-tap half band whose non-zero taps are the even ones
// (symmetric pairs 2q / L-1-2q) and the centre (downconvert.cpp:286-320, 348-423).  The pair
// coefficients are wave-uniform and stay in scalar registers.
//
// The stage input xe = [history | input] is kept split by sample parity, E[m] = xe[2m] and
// O[m] = xe[2m+1], so that output j reads E[j+q] / O[j+q]: consecutive lanes touch consecutive
// LDS words (the interleaved layout made every tap read a 16-byte-stride access).  Outputs go to
// the next stage's halves (its history is even, so output j has parity j&1) or, after the last
// stage, to the linear tile-output region.  One output per lane and pass.
template <int L>
__device__ __forceinline__ void dc_stage(const v2f *E, const v2f *O, v2f *yE, v2f *yO, v2f *ylin, int nout,
                                         const int *prm, int t)
{
    constexpr int NP = (L == 3) ? 2 : (L + 1) / 4;
    constexpr int H = (L - 1) / 2;              // centre tap (odd index for every L = 4k+3)
    float c[NP];
#pragma unroll
    for (int q = 0; q < NP; q += 4) {
        const v4f v = *reinterpret_cast<const v4f *>(prm + DP_C0 + q);
        c[q] = v.x;
        if (q + 1 < NP) c[q + 1] = v.y;
        if (q + 2 < NP) c[q + 2] = v.z;
        if (q + 3 < NP) c[q + 3] = v.w;
    }
    const float cc = __int_as_float(prm[DP_CC]);
    for (int j = t; j < nout; j += DC_T) {
        v2f acc;
        if (L == 3) {
            acc = dc_cic(E[j], O[j], E[j + 1], O[j + 1], c[0], c[1]);
        } else {
            acc = dc_first(O[j + (H - 1) / 2], cc);
#pragma unroll
            for (int q = 0; q < NP; q++) acc = dc_mac(acc, E[j + q], E[j + H - q], c[q]);
        }
        if (ylin) ylin[j] = acc;
        else if (j & 1) yO[j >> 1] = acc;
        else yE[j >> 1] = acc;
    }
}

// The same stage for a complete tile of a compile-time plan: the output count is a constant, whole passes carry
// no lane predicate and every LDS offset is an immediate.
// A lane computes G ADJACENT outputs from one register window (round 3): outputs j .. j+G-1 read E[j .. j+H+G-1]
// and G consecutive odd-half samples, as 16-byte LDS reads -- (H+G)/2 + G/2 wide reads instead of (H+2)*G narrow
// ones.  The down-converter keeps the LDS pipe busy three quarters of its time (SQ_LDS_IDX_ACTIVE 74 %, DESIGN K2),
// and the first two stages are two thirds of that traffic: 56 -> 40 B per output of an 11-tap stage at G = 2.  The
// arithmetic per output -- centre product, then the pairs in tap order -- is what dc_stage does, so the words are too.
// (Four outputs per lane measured no better than two -- more registers -- and are gone.)
constexpr int DC_G2_MAXL = 19;            // two outputs per lane up to this many taps
template <int L, int NOUT>
__device__ __forceinline__ void dc_stage_full(const v2f *E, const v2f *O, v2f *yE, v2f *yO, bool last, int t)
{
    constexpr int NP = (L == 3) ? 2 : (L + 1) / 4;
    constexpr int H = (L - 1) / 2;
    float c[NP];                                 // the taps are literals here: no table read, no registers
#pragma unroll
    for (int q = 0; q < NP; q++) c[q] = dc_pair_coef(L, q);
    constexpr float cc = dc_centre_coef(L);
    // (long half bands sit at the end of a cascade, a few outputs per tile: their window would cost more registers --
    // spills at 128 -- than the LDS bytes it saves)
    constexpr int G = (NOUT >= 2 && L <= DC_G2_MAXL) ? 2 : 1;
    if constexpr (G == 1) {
        constexpr int PASSES = NOUT >= DC_T ? NOUT / DC_T : 1;
        v2f r[PASSES];
        if (NOUT >= DC_T || t < NOUT) {
#pragma unroll
            for (int k = 0; k < PASSES; k++) {
                const v2f *e = E + t + k * DC_T, *o = O + t + k * DC_T;
                if (L == 3) r[k] = dc_cic(e[0], o[0], e[1], o[1], c[0], c[1]);
                else {
                    v2f acc = dc_first(o[(H - 1) / 2], cc);
#pragma unroll
                    for (int q = 0; q < NP; q++) acc = dc_mac(acc, e[q], e[H - q], c[q]);
                    r[k] = acc;
                }
            }
            v2f *y = last ? yE + t : ((t & 1) ? yO : yE) + (t >> 1);
#pragma unroll
            for (int k = 0; k < PASSES; k++) y[k * (last ? DC_T : DC_T / 2)] = r[k];
        }
    } else {
        constexpr int PASSES = NOUT >= G * DC_T ? NOUT / (G * DC_T) : 1;
        constexpr int NWIN = (L == 3 ? 1 : H) + G;                    // E[j .. j+NWIN-1]
        constexpr int NB = (NWIN + 1) / 2;
        constexpr int C0 = (L == 3) ? 0 : (H - 1) / 2;                // first odd-half sample: O[j + C0]
        constexpr int OB0 = C0 & ~1, NOB = (C0 - OB0 + (L == 3 ? G + 1 : G) + 1) / 2;
        // Alignment and extent of the 16-byte window reads.  A region starts at an even slot (dc_layout_of rounds every
        // half to an even length), j is a multiple of G and OB0 is even: E + j + 2i and O + j + OB0 + 2i are 16-byte
        // aligned whatever the history's parity (only the OUTPUT halves, which start behind hist/2 slots, are 8-byte
        // aligned: they are stored as v2f unless `last`).  An odd window is read one sample long; that sample and the
        // whole last window lie inside the half, whose length is (hist/2 + NOUT + 2) & ~1:
        constexpr int HALF = (dc_hist_of(L) / 2 + NOUT + 2) & ~1;
        static_assert((NOUT >= G ? NOUT - G : 0) + 2 * NB <= HALF, "even-half window reads stay inside the stage's LDS half");
        static_assert((NOUT >= G ? NOUT - G : 0) + OB0 + 2 * NOB <= HALF, "odd-half window reads stay inside the stage's LDS half");
        v2f r[PASSES][G];
        if (NOUT >= G * DC_T || G * t < NOUT) {
#pragma unroll
            for (int k = 0; k < PASSES; k++) {
                const int j = G * t + G * DC_T * k;
                v2f w[2 * NB], o[2 * NOB];
#pragma unroll
                for (int i = 0; i < NB; i++) {
                    const v4f v = *reinterpret_cast<const v4f *>(E + j + 2 * i);
                    w[2 * i] = v2f{v.x, v.y}; w[2 * i + 1] = v2f{v.z, v.w};
                }
#pragma unroll
                for (int i = 0; i < NOB; i++) {
                    const v4f v = *reinterpret_cast<const v4f *>(O + j + OB0 + 2 * i);
                    o[2 * i] = v2f{v.x, v.y}; o[2 * i + 1] = v2f{v.z, v.w};
                }
#pragma unroll
                for (int u = 0; u < G; u++) {
                    if (L == 3) {
                        r[k][u] = dc_cic(w[u], o[u], w[u + 1], o[u + 1], c[0], c[1]);
                    } else {
                        v2f acc = dc_first(o[C0 - OB0 + u], cc);
#pragma unroll
                        for (int q = 0; q < NP; q++) acc = dc_mac(acc, w[u + q], w[u + H - q], c[q]);
                        r[k][u] = acc;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PASSES; k++) {
                const int j = G * t + G * DC_T * k;
                if (last) {
                    *reinterpret_cast<v4f *>(yE + j) = v4f{r[k][0].x, r[k][0].y, r[k][1].x, r[k][1].y};
                } else {                                              // (the halves start behind an odd history: 8-byte aligned)
                    yE[j >> 1] = r[k][0];
                    yO[j >> 1] = r[k][1];
                }
            }
        }
    }
}

// ---- what the steps of a tile share ------------------------------------------------------------------
// What is fixed for the workgroup: its lane, its channel and segment, the channel's rows, the blanker in front.
struct DcWave {
    int t, ch, seg;
    v2f *lds;
    const DcParamRow *ptab;
    long seg_start, seg_end;
    long steady_end;                         // complete tiles in front of it have nothing to save for the next call
    DcChan cs;
    const v2f *in;                           // input row: float samples ...
    const unsigned char *pk;  int pkt_len;   // ... or datagrams (pk != nullptr)
    v2f *out;
    const v2f *hist;  v2f *hist_next;
    // BLK: delay D1 = delay_n + 1 (0 when the row's blanker is off: its mask is all zero), mask row, raw history
    int D1;
    const unsigned *mrow;
    const v2f *bhist;
};

// The lane's two phasors of the current row (samples 2t and 2t + 1), carrying the settled amplitude a_inf.
struct DcNco {
    v2f p0, p1, step1, rowstep;              // step1 / rowstep: one sample / one row of rotation
    float a_inf, inv_a_inf;
    int anchor_rows;                         // rows until the phasors are re-anchored
    // Re-anchoring the phasors (exact phase from the 64-bit accumulator, then one complex multiply per row) on an
    // ABSOLUTE grid -- every DC_ANCHOR_ROWS rows counted from the channel's first sample, not from wherever this
    // workgroup's segment or this call happens to start: a tile that starts between two grid points anchors at the
    // grid point behind it and walks the rows in between with the same multiplies a continuous run would have made.
    // The mixed samples, hence the output WORDS, then do not depend on how the stream is cut into calls and segments
    // (for calls that are whole tiles: a short tile breaks the row cadence and anchors where it stands, as before).
    __device__ __forceinline__ void anchor(const DcChan &cs, long at, bool full_tile, int t)
    {
        int back = 0;                                    // whole tiles between the grid point and `at`
        if (full_tile) {
            const unsigned long long ab = cs.age + (unsigned long long)at;
            if ((ab & (unsigned long long)(DC_TILE - 1)) == 0) back = (int)((ab / DC_TILE) & (unsigned long long)(DC_ANCHOR_ROWS / DC_NR - 1));
        }
        p0 = phasor_of(cs.phase + cs.inc * (unsigned long long)(at - (long)back * DC_TILE + 2 * t + 1)) * a_inf;
        p1 = cmul(p0, step1);
        for (int r = 0; r < back * DC_NR; r++) advance();
        anchor_rows = full_tile ? DC_ANCHOR_ROWS - back * DC_NR : 0;
    }
    __device__ __forceinline__ void advance() { p0 = cmul(p0, rowstep); p1 = cmul(p1, rowstep); }
};

// The raw input of a tile is fetched into registers one tile ahead, while the previous tile goes through the
// cascade: nothing waits on HBM latency except the very first tile.  Datagram words are decoded where they are
// consumed.  BLK: the tile's mask words (lane l & 15 holds word l & 15 of the sixteen; a lane's two samples of a row
// share one) and, for datagram input behind an ODD delay, the raw words of the one sample behind the tile's last pair.
struct DcTileIn {
    v4f raw[DC_NR];
    unsigned mkw;
    unsigned xw[3];
};

// the input format as a constant: 0 float rows, otherwise the datagram length (the decode then carries no format
// test and the sample-index division is a multiply)
template <class F>
__device__ __forceinline__ void dc_with_format(const DcWave &w, F &&f)
{
    if (!w.pk) f(std::integral_constant<int, 0>{});
    else if (w.pkt_len == 1444) f(std::integral_constant<int, 1444>{});
    else f(std::integral_constant<int, 1028>{});
}

__device__ __forceinline__ int dc_tile_len(const DcWave &w, long p)
{
    const long lim = ((p < w.seg_start) ? w.seg_start : w.seg_end) - p;
    return (int)(lim < DC_TILE ? lim : DC_TILE);
}

// ---- fetch ---------------------------------------------------------------------------------------------
// A COMPLETE tile at p: all rows, no bounds.  BLK: the blanker hands over raw[i - D1] for sample i, all of them in
// this call's input (the caller's condition), with the tile's mask words; datagrams are fetched as ALIGNED pairs, so
// behind an odd delay the pairs start one sample early and the sample behind the tile's last pair comes along.
template <int FMT, bool BLK>
__device__ __forceinline__ void dc_fetch_full(const DcWave &w, DcTileIn &ti, long p)
{
    const bool odd = BLK && (w.D1 & 1);
    if constexpr (BLK) ti.mkw = w.mrow[(p >> 5) + (w.t & 15)];
#pragma unroll
    for (int r = 0; r < DC_NR; r++) {
        const long i = p + r * DC_ROW + 2 * w.t;
        if constexpr (FMT != 0) {
            const wf4 v = wire_pair_fetch(w.pk, FMT, BLK ? i - w.D1 - (odd ? 1 : 0) : i);
            // 24-bit: three words into three lanes, the fourth stays 0 (written whole, the tuple is put together from
            // the load and a zero behind a wait on the first row's load, in front of the cascade)
            if constexpr (FMT == 1444) { ti.raw[r].x = v.x; ti.raw[r].y = v.y; ti.raw[r].z = v.z; }
            else ti.raw[r] = v4f{v.x, v.y, v.z, v.w};
        } else if constexpr (BLK) {
            ti.raw[r] = *reinterpret_cast<const f4a8 *>(w.in + i - w.D1);                   // 8-byte aligned, 16 bytes
        } else {
            ti.raw[r] = dc_stream_load(reinterpret_cast<const v4f *>(w.in + i));
        }
    }
    if constexpr (BLK && FMT != 0)
        if (odd) wire_sample_fetch(w.pk, FMT, p + DC_TILE - 1 - w.D1, ti.xw);
    // All of the tile's loads are issued HERE (a compiler fence, no instruction): left free, the compiler merges the
    // last row's load with the bounded fetch's on the other side of the caller's branch and sinks it behind the join,
    // where it is issued only after the first three rows have arrived (24-bit datagrams: +4 % per launch).
    asm volatile("" ::: "memory");
}
// BLK: only a complete tile whose delayed samples all lie in this call's input is prefetched (the steady tile's
// condition); other tiles are read where they are consumed (dc_blanked_pair)
template <int FMT>
__device__ __forceinline__ void dc_fetch_blanked(const DcWave &w, DcTileIn &ti, long p)
{
    if (p - w.D1 - 1 >= 0 && p + DC_TILE <= w.seg_end) dc_fetch_full<FMT, true>(w, ti, p);
}
// any tile at p, bounded by its length (nothing past the end, nothing for the history-fed warm-up)
template <bool BLK>
__device__ __forceinline__ void dc_fetch(const DcWave &w, DcTileIn &ti, long p)
{
    if (p >= w.seg_end || (p < w.seg_start && w.seg == 0)) return;
    if constexpr (BLK) {
        dc_with_format(w, [&](auto FMT) { dc_fetch_blanked<decltype(FMT)::value>(w, ti, p); });
    } else {
        const int m = dc_tile_len(w, p);
#pragma unroll
        for (int r = 0; r < DC_NR; r++) {
            const int i = r * DC_ROW + 2 * w.t;
            if (i < m) {
                if (w.pk) {
                    const wf4 v = wire_pair_fetch(w.pk, w.pkt_len, p + i);                  // raw words; p + i is even
                    ti.raw[r] = v4f{v.x, v.y, v.z, v.w};
                } else {
                    ti.raw[r] = dc_stream_load(reinterpret_cast<const v4f *>(w.in + p + i));
                }
            }
        }
    }
}

// ---- decode --------------------------------------------------------------------------------------------
// value of lane + 1 (lane 63: lane 0's): the DPP wavefront rotate, no LDS
__device__ __forceinline__ float dc_rotl1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x134, 0xf, 0xf, false));   // wave_rol:1
}
// The samples of a tile fetched by dc_fetch_full.  BLK, datagrams behind an ODD delay: the lane fetched the aligned
// pair (e, e+1) and wants (e+1, e+2); e+2 is the first sample of the next lane's pair (lane 63: of the next row's
// lane 0, and behind the tile's last pair the one sample fetched into xw) -- a wavefront rotate, no LDS.
template <int FMT, bool BLK>
__device__ __forceinline__ void dc_decode(const DcWave &w, const DcTileIn &ti, v4f dv[DC_NR])
{
#pragma unroll
    for (int row = 0; row < DC_NR; row++) {
        dv[row] = ti.raw[row];
        if constexpr (FMT != 0) {
            const wf4 d = wire_pair_decode(wf4{dv[row].x, dv[row].y, dv[row].z, dv[row].w}, FMT);
            dv[row] = v4f{d.x, d.y, d.z, d.w};
        }
    }
    if constexpr (BLK && FMT != 0) {
        if (w.D1 & 1) {
            const wf2 xs = wire_sample_decode(ti.xw, FMT);
            const bool lastlane = w.t == DC_T - 1;
            v4f rot[DC_NR];
#pragma unroll
            for (int row = 0; row < DC_NR; row++) {
                const float ax = dc_rotl1(dv[row].x), ay = dc_rotl1(dv[row].y);
                const float bx = row + 1 < DC_NR ? dc_rotl1(dv[row + 1 < DC_NR ? row + 1 : row].x) : xs.x;
                const float by = row + 1 < DC_NR ? dc_rotl1(dv[row + 1 < DC_NR ? row + 1 : row].y) : xs.y;
                rot[row] = v4f{dv[row].z, dv[row].w, lastlane ? bx : ax, lastlane ? by : ay};
            }
#pragma unroll
            for (int row = 0; row < DC_NR; row++) dv[row] = rot[row];
        }
    }
}
// zero under the blanker's mask: word 4 row + (t >> 4) of the tile's sixteen; tiles start at multiples of 512, so
// sample i's bit (i & 31) is 2t & 31
__device__ __forceinline__ v4f dc_masked(v4f v, unsigned mkw, int row, int t)
{
    const unsigned m = (unsigned)__shfl((int)mkw, 4 * row + (t >> 4)) >> ((2 * t) & 31);
    if (m & 1u) { v.x = 0.f; v.y = 0.f; }
    if (m & 2u) { v.z = 0.f; v.w = 0.f; }
    return v;
}
// Tiles that were not prefetched whole.  One raw input sample of the stream the blanker saw: this call's, or the
// history's for j < 0 ...
__device__ __forceinline__ v2f dc_raw_at(const DcWave &w, long j)
{
    if (j < 0) return w.bhist[NB_HIST + j];
    if (w.pk) { const wf2 s = wire_sample(w.pk, w.pkt_len, j); return v2f{s.x, s.y}; }
    return w.in[j];
}
// ... samples idx, idx + 1 (idx even) as the blanker hands them over: delayed by D1, zero under the mask ...
__device__ __forceinline__ v4f dc_blanked_pair(const DcWave &w, long idx)
{
    v2f s0 = dc_raw_at(w, idx - w.D1), s1 = dc_raw_at(w, idx + 1 - w.D1);
    const unsigned m = w.mrow[idx >> 5] >> (idx & 31);
    if (m & 1u) s0 = v2f{0.f, 0.f};
    if (m & 2u) s1 = v2f{0.f, 0.f};
    return v4f{s0.x, s0.y, s1.x, s1.y};
}
// ... and the lane's pair of row `row` of the tile at pos: read in place (BLK) or decoded from the bounded prefetch
template <bool BLK>
__device__ __forceinline__ v4f dc_pair_of_row(const DcWave &w, const DcTileIn &ti, long pos, int row)
{
    if constexpr (BLK) {
        return dc_blanked_pair(w, pos + row * DC_ROW + 2 * w.t);
    } else {
        if (!w.pk) return ti.raw[row];
        const wf4 d = wire_pair_decode(wf4{ti.raw[row].x, ti.raw[row].y, ti.raw[row].z, ti.raw[row].w}, w.pkt_len);
        return v4f{d.x, d.y, d.z, d.w};
    }
}

// ---- mix: stage 0's input, parity halves behind their histories ---------------------------------------------
// a complete tile, amplitude settled, no history to save; pair(row) gives the lane's two samples of a row
template <class F>
__device__ __forceinline__ void dc_mix_full(v2f *e, v2f *o, DcNco &nco, F &&pair)
{
#pragma unroll
    for (int row = 0; row < DC_NR; row++) {
        const v4f v = pair(row);
        e[row * DC_T] = cmul(v2f{v.x, v.y}, nco.p0);
        o[row * DC_T] = cmul(v2f{v.z, v.w}, nco.p1);
        nco.advance();
    }
}
// any other tile: n samples, the start-up envelope, the last W mixed samples of the call kept as the next call's
// warm-up; without stages the mixed samples go to the linear output region
template <bool BLK>
__device__ __forceinline__ void dc_mix_ragged(const DcArgs &a, const DcWave &w, DcNco &nco, const DcTileIn &ti, v2f *r0,
                                              v2f *r0o, long pos, int n, bool warm, int ns)
{
#pragma unroll
    for (int row = 0; row < DC_NR; row++) {
        const int i = row * DC_ROW + 2 * w.t;
        const long gi = pos + i;                       // sample index within the call
        if (i < n) {
            const v4f v = dc_pair_of_row<BLK>(w, ti, pos, row);
            v2f x0 = cmul(v2f{v.x, v.y}, nco.p0), x1 = cmul(v2f{v.z, v.w}, nco.p1);
            const unsigned long long age = w.cs.age + (unsigned long long)gi;
            if (age + 1 < DC_AMP_N) {                   // start-up envelope (the phasors carry a_inf)
                x0 *= a.amp[age] * nco.inv_a_inf; x1 *= a.amp[age + 1] * nco.inv_a_inf;
            }
            if (ns == 0) {
                *reinterpret_cast<v4f *>(&r0[i]) = v4f{x0.x, x0.y, x1.x, x1.y};
            } else {
                r0[i >> 1] = x0; r0o[i >> 1] = x1;
            }
            const long hj = gi - (a.n_in - a.W);
            if (!warm && hj >= 0 && a.W > 0)
                *reinterpret_cast<v4f *>(&w.hist_next[hj]) = v4f{x0.x, x0.y, x1.x, x1.y};
        }
        nco.advance();
    }
}
// segment 0's warm-up: the mixed samples the previous call left behind
__device__ __forceinline__ void dc_take_history(const v2f *h, v2f *r0, v2f *r0o, int n, int ns, int t)
{
    for (int i = t; i < n; i += DC_T) {
        const v2f v = h[i];
        if (ns == 0) r0[i] = v;
        else if (i & 1) r0o[i >> 1] = v;
        else r0[i >> 1] = v;
    }
}

// ---- cascade, history slide and tile store of a compile-time plan --------------------------------------
// LDS -> LDS, n input samples: whole passes for a complete tile (the steady tile passes the constant)
template <class P>
__device__ __forceinline__ void dc_cascade(const DcWave &w, int n)
{
    constexpr DcLayout LY = dc_layout_of(P::KIND, P::NS);
    static_for<0, P::NS>([&](auto S) {
        constexpr int s = S.value, L = P::KIND[s];
        constexpr bool last = s + 1 == P::NS;
        const v2f *E = w.lds + LY.roff[s], *O = E + LY.ooff[s];
        v2f *yE = w.lds + LY.roff[s + 1] + (last ? 0 : dc_hist_of(P::KIND[s + 1]) / 2), *yO = yE + LY.ooff[s + 1];
        if (n == DC_TILE) dc_stage_full<L, ((DC_TILE / 2) >> s)>(E, O, yE, yO, last, w.t);
        else dc_stage<L>(E, O, yE, yO, last ? yE : nullptr, n >> (s + 1), w.ptab[s], w.t);
        lds_barrier();
    });
}
// Slide every stage's history: the last hist_s inputs of stage s (hist_s/2 per parity half) move to the front of
// its region (lanes 0-31 the even half, 32-63 the odd one); all reads, a barrier, then the writes, because a short
// tile overlaps source and target.
template <class P>
__device__ __forceinline__ void dc_slide(v2f *lds, int n, int t)
{
    constexpr DcLayout LY = dc_layout_of(P::KIND, P::NS);
    v2f keep[P::NS];
    const int i = t & 31, odd = t >> 5;
    static_for<0, P::NS>([&](auto S) {
        constexpr int sg = S.value;
        if (__builtin_expect(i < dc_hist_of(P::KIND[sg]) / 2, 1)) keep[sg] = lds[LY.roff[sg] + (odd ? LY.ooff[sg] : 0) + i + (n >> (sg + 1))];
    });
    lds_barrier();
    static_for<0, P::NS>([&](auto S) {
        constexpr int sg = S.value;
        if (__builtin_expect(i < dc_hist_of(P::KIND[sg]) / 2, 1)) lds[LY.roff[sg] + (odd ? LY.ooff[sg] : 0) + i] = keep[sg];
    });
}
// tile outputs -> HBM
template <class P>
__device__ __forceinline__ void dc_store_tile(const DcWave &w, long pos, int n)
{
    constexpr int LEN = DC_TILE >> P::NS;
    const v2f *y = w.lds + dc_layout_of(P::KIND, P::NS).roff[P::NS];
    v2f *o = w.out + (pos >> P::NS);
    if (n == DC_TILE) {
#pragma unroll
        for (int j = 0; j < (LEN + DC_T - 1) / DC_T; j++)
            if (LEN >= DC_T || w.t < LEN) o[j * DC_T + w.t] = y[j * DC_T + w.t];
    } else {
        for (int j = w.t; j < (n >> P::NS); j += DC_T) o[j] = y[j];
    }
}

// ---- the same three steps of the run-time plan -----------------------------------------------------------
// pv0 / pv1, lane s: kind | hist/2 << 8 | odd-half offset << 16, and the region offset, of stage s
__device__ __forceinline__ void dc_stage_any(int kind, const v2f *E, const v2f *O, v2f *yE, v2f *yO, v2f *ylin, int nout,
                                             const int *prm, int t)
{
#define DC_CASE(LL) case LL: dc_stage<LL>(E, O, yE, yO, ylin, nout, prm, t); break;
    switch (kind) {
    DC_CASE(3) DC_CASE(11) DC_CASE(15) DC_CASE(19) DC_CASE(23) DC_CASE(27) DC_CASE(31)
    DC_CASE(35) DC_CASE(39) DC_CASE(43) DC_CASE(47)
    default: dc_stage<51>(E, O, yE, yO, ylin, nout, prm, t); break;
    }
#undef DC_CASE
}
__device__ __forceinline__ int dc_cascade_dyn(const DcWave &w, int ns, int pv0, int pv1, int n)
{
    int len = n;
    for (int s = 0; s < ns; s++) {
        const int d0 = __builtin_amdgcn_readlane(pv0, s), dn = __builtin_amdgcn_readlane(pv0, s + 1);
        const v2f *E = w.lds + __builtin_amdgcn_readlane(pv1, s), *O = E + (d0 >> 16);
        const int hn2 = (dn >> 8) & 0xff;                   // 0 behind the last stage
        v2f *yE = w.lds + __builtin_amdgcn_readlane(pv1, s + 1) + hn2;
        v2f *yO = yE + (dn >> 16);
        len >>= 1;
        dc_stage_any(d0 & 0xff, E, O, yE, yO, s + 1 == ns ? yE : nullptr, len, w.ptab[s], w.t);
        lds_barrier();
    }
    return len;
}
__device__ __forceinline__ void dc_slide_dyn(v2f *lds, int ns, int pv0, int pv1, int n, int t)
{
    constexpr int R = (DC_MAX_STAGES * 64 + DC_T - 1) / DC_T;
    v2f keep[R];
    int dst[R];
    static_for<0, R>([&](auto RR) {
        constexpr int r = RR.value;
        const int u = t + r * DC_T, odd = (u >> 5) & 1, i = u & 31;
        const int sg = __builtin_amdgcn_readfirstlane(u >> 6);
        dst[r] = -1;
        if (sg < ns) {
            const int d = __builtin_amdgcn_readlane(pv0, sg);
            if (i < ((d >> 8) & 0xff)) {
                dst[r] = __builtin_amdgcn_readlane(pv1, sg) + (odd ? (d >> 16) : 0) + i;
                keep[r] = lds[dst[r] + (n >> (sg + 1))];
            }
        }
    });
    lds_barrier();
    static_for<0, R>([&](auto RR) { if (dst[RR.value] >= 0) lds[dst[RR.value]] = keep[RR.value]; });
}

// ---- the two kinds of tile ----------------------------------------------------------------------------
// Steady state of a compile-time plan: a complete tile mixed from this call's input, the NCO amplitude settled,
// nothing to save for the next call (BLK: and no delayed sample reaching into the blanker's history).  No tile
// length, no path selection, no lane predicate; every other tile (history-fed warm-up, the last W samples, a
// segment's odd end) is a general tile, which keeps the same one-tile-ahead prefetch protocol.
template <bool BLK>
__device__ __forceinline__ bool dc_steady_ok(const DcWave &w, long pos)
{
    const long lim = pos < w.seg_start ? w.seg_start : w.steady_end;
    if (!(pos + DC_TILE <= lim && (w.seg > 0 || pos >= 0) && w.cs.age + (unsigned long long)pos >= DC_AMP_N)) return false;
    if constexpr (BLK) { if (pos - w.D1 - 1 < 0) return false; }
    return true;
}
template <class P, bool BLK, int FMT>
__device__ __forceinline__ void dc_steady_tile(const DcWave &w, DcNco &nco, DcTileIn &ti, long pos)
{
    constexpr DcLayout LY = dc_layout_of(P::KIND, P::NS);
    const bool warm = pos < w.seg_start;
    if (nco.anchor_rows <= 0) nco.anchor(w.cs, pos, true, w.t);
    nco.anchor_rows -= DC_NR;
    bool any_blank = false;                                // (rare: a tile with an impulse in it)
    if constexpr (BLK) any_blank = __any(ti.mkw != 0u);
    v4f dv[DC_NR];
    dc_decode<FMT, BLK>(w, ti, dv);
    v2f *e = w.lds + LY.roff[0] + dc_hist_of(P::KIND[0]) / 2 + w.t;
    dc_mix_full(e, e + LY.ooff[0], nco, [&](int row) {
        v4f v = dv[row];
        if (any_blank) v = dc_masked(v, ti.mkw, row, w.t);
        return v;
    });
    lds_barrier();
    if constexpr (BLK) dc_fetch_blanked<FMT>(w, ti, pos + DC_TILE);
    else if (pos + 2 * DC_TILE <= (warm ? w.seg_start : w.steady_end)) dc_fetch_full<FMT, false>(w, ti, pos + DC_TILE);
    else dc_fetch<false>(w, ti, pos + DC_TILE);
    dc_cascade<P>(w, DC_TILE);
    dc_slide<P>(w.lds, DC_TILE, w.t);
    if (!warm) dc_store_tile<P>(w, pos, DC_TILE);
    lds_barrier();
}
// Any tile; returns its length.
template <class P, bool BLK>
__device__ __forceinline__ int dc_general_tile(const DcArgs &a, const DcWave &w, DcNco &nco, DcTileIn &ti, int pv0, int pv1,
                                               long pos)
{
    constexpr DcLayout LY = dc_layout_of(P::KIND, P::NS);
    const int ns = P::FIX ? P::NS : a.nstages;
    const int *roff = P::FIX ? LY.roff : a.roff;
    const bool warm = pos < w.seg_start;
    const int n = dc_tile_len(w, pos);
    // stage-0 input: parity halves behind their histories (no decimation: the linear output region)
    const int h0 = ns > 0 ? (P::FIX ? dc_hist_of(P::KIND[0]) : a.st[0].hist) / 2 : 0;
    v2f *r0 = w.lds + roff[0] + h0, *r0o = r0 + (ns > 0 ? (P::FIX ? LY.ooff[0] : a.ooff[0]) : 0);
    if (warm && w.seg == 0) {
        dc_take_history(w.hist + pos + a.W, r0, r0o, n, ns, w.t);
    } else {
        // the phasors run on from tile to tile and are re-anchored every DC_ANCHOR_ROWS rows (and after a short
        // tile, which breaks the row cadence)
        if (nco.anchor_rows <= 0 || n != DC_TILE) nco.anchor(w.cs, pos, n == DC_TILE, w.t);
        nco.anchor_rows -= DC_NR;
        // Full tile, amplitude settled, no history to save: the lean mix.  A compiled plain plan never gets here with
        // such a tile: lean implies n == DC_TILE (pos + DC_TILE <= seg_start when warm, <= seg_end otherwise), a
        // settled amplitude, seg > 0 or pos >= 0 (the history-fed warm-up took the other branch) and, when not warm,
        // pos + DC_TILE <= n_in - W or W == 0 -- together dc_steady_ok(pos), which has just said no.  (Blanked plans
        // do: a complete tile whose delayed samples reach into the blanker's history.)
        const bool lean = (!P::FIX || BLK) && ns > 0 && n == DC_TILE && w.cs.age + (unsigned long long)pos >= DC_AMP_N &&
                          (warm || a.W == 0 || pos + n <= a.n_in - a.W);
        if (lean) dc_mix_full(r0 + w.t, r0o + w.t, nco, [&](int row) { return dc_pair_of_row<BLK>(w, ti, pos, row); });
        else dc_mix_ragged<BLK>(a, w, nco, ti, r0, r0o, pos, n, warm, ns);
    }
    lds_barrier();
    dc_fetch<BLK>(w, ti, pos + n);                        // next tile's input, in flight during the cascade
    if constexpr (P::FIX) {
        dc_cascade<P>(w, n);
        dc_slide<P>(w.lds, n, w.t);
        if (!warm) dc_store_tile<P>(w, pos, n);
    } else {
        const int len = dc_cascade_dyn(w, ns, pv0, pv1, n);
        dc_slide_dyn(w.lds, ns, pv0, pv1, n, w.t);
        if (!warm) for (int j = w.t; j < len; j += DC_T) w.out[(pos >> ns) + j] = w.lds[roff[ns] + j];
    }
    lds_barrier();
    return n;
}

// ---- set-up --------------------------------------------------------------------------------------------
// the stage parameter rows (run-time plan, short tiles) and zeroed stage histories
__device__ __forceinline__ void dc_stage_rows(const DcArgs &a, DcParamRow *ptab, v2f *lds, const int *roff, int ns, int t)
{
    for (int i = t; i < (ns + 1) * DP_WORDS; i += DC_T) {
        const int s = i / DP_WORDS, k = i % DP_WORDS;
        int v = 0;
        if (k == DP_ROFF) v = roff[s];
        else if (k == DP_OOFF) v = a.ooff[s];
        else if (s < ns) {
            if (k == DP_KIND) v = a.kind[s];
            else if (k == DP_HIST2) v = a.st[s].hist / 2;
            else if (k == DP_CC) v = __float_as_int(a.st[s].ccoef);
            else if (k >= DP_C0 && k - DP_C0 < DC_MAX_PAIRS) v = __float_as_int(a.st[s].c[k - DP_C0]);
        }
        ptab[s][k] = v;
    }
    for (int s = 0; s < ns; s++)
        for (int i = t; i < a.st[s].hist; i += DC_T)
            lds[roff[s] + ((i & 1) ? a.ooff[s] : 0) + (i >> 1)] = v2f{0.f, 0.f};
    lds_barrier();
}
template <bool BLK>
__device__ __forceinline__ DcWave dc_wave_of(const DcArgs &a, v2f *lds, const DcParamRow *ptab, int t, int ch, int seg)
{
    DcWave w{};
    w.t = t; w.ch = ch; w.seg = seg; w.lds = lds; w.ptab = ptab;
    w.cs = a.chan[ch];
    const long in_row = a.in_rows ? a.in_rows[ch] : ch;
    w.in = a.in + in_row * a.in_stride;
    w.pk = a.wire.pk ? a.wire.pk + in_row * a.wire.chan_stride : nullptr;
    w.pkt_len = a.wire.pkt_len;
    if constexpr (BLK) {
        const NbChan nb = a.nb_state[in_row];
        w.D1 = nb.on ? nb.delay_n + 1 : 0;
        w.mrow = a.nb_mask + in_row * a.nb_mask_stride;
        w.bhist = a.nb_hist + in_row * NB_HIST;
    }
    w.out = a.out + (long)ch * a.out_stride;
    w.hist = a.hist + (long)ch * a.hist_stride;
    w.hist_next = a.hist_next + (long)ch * a.hist_stride;
    w.seg_start = (long)seg * a.seg_len;
    w.seg_end = w.seg_start + a.seg_len;
    if (w.seg_end > a.n_in) w.seg_end = a.n_in;
    w.steady_end = a.W ? (w.seg_end < (long)a.n_in - a.W ? w.seg_end : (long)a.n_in - a.W) : w.seg_end;
    return w;
}

// ---- the kernel ----------------------------------------------------------------------------------------
// BLK: the noise blanker's decision applied in this kernel's loads (DcArgs::nb_mask; a kernel of its own so that the
// plain kernel keeps its registers: the blanked form carries the mask words and one more sample per tile)
constexpr int DC_WAVES_PER_SIMD = 4;      // 128 registers a lane (three waves, 168 registers, were tried and measured slower)
template <class P, bool BLK = false>
__global__ __launch_bounds__(DC_T) __attribute__((amdgpu_waves_per_eu(DC_WAVES_PER_SIMD, DC_WAVES_PER_SIMD)))
void downconv_kernel(DcArgs a)
{
    constexpr DcLayout LY = dc_layout_of(P::KIND, P::NS);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2f *lds = reinterpret_cast<v2f *>(smem_raw);
    const int t = threadIdx.x;
    const int ns = P::FIX ? P::NS : a.nstages;
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_DC);
    const int wg = blockIdx.x;
    const int ci = wg / a.nseg, seg = wg % a.nseg;
    if (ci >= a.nchan) return;
    // LDS regions R_s = [hist_s | stage-s input] at roff[s] (the plan's own layout; host computed for a run-time
    // plan), R_ns = tile outputs
    const int *roff = P::FIX ? LY.roff : a.roff;
    __shared__ __attribute__((aligned(16))) int ptab[DC_MAX_STAGES + 1][DP_WORDS];
    dc_stage_rows(a, ptab, lds, roff, ns, t);
    int pv0, pv1;                                        // run-time plan: stage s's layout words in lane s
    {
        const int *row = ptab[(t & 63) <= ns ? (t & 63) : ns];
        pv0 = row[DP_KIND] | (row[DP_HIST2] << 8) | (row[DP_OOFF] << 16);
        pv1 = row[DP_ROFF];
    }
    const DcWave w = dc_wave_of<BLK>(a, lds, ptab, t, a.chan_list ? a.chan_list[ci] : ci, seg);
    DcNco nco;
    nco.step1 = phasor_of(w.cs.inc);
    nco.rowstep = phasor_of(w.cs.inc * (unsigned long long)DC_ROW);
    nco.a_inf = a.amp[DC_AMP_N - 1]; nco.inv_a_inf = 1.0f / nco.a_inf;
    nco.p0 = nco.p1 = v2f{1.f, 0.f};
    nco.anchor_rows = 0;
    DcTileIn ti;
    ti.mkw = ti.xw[0] = ti.xw[1] = ti.xw[2] = 0u;
    for (int r = 0; r < DC_NR; r++) ti.raw[r] = v4f{0.f, 0.f, 0.f, 0.f};

    // pos: index of the tile's first sample in this call's input (negative inside the warm-up)
    long pos = w.seg_start - a.W;
    dc_fetch<BLK>(w, ti, pos);
    while (pos < w.seg_end) {
        if constexpr (P::FIX) {
            // one copy of the steady loop per input format (float rows, 16-bit and 24-bit datagrams)
            dc_with_format(w, [&](auto FMT) {
                for (; dc_steady_ok<BLK>(w, pos); pos += DC_TILE) dc_steady_tile<P, BLK, decltype(FMT)::value>(w, nco, ti, pos);
            });
            if (pos >= w.seg_end) break;
        }
        pos += dc_general_tile<P, BLK>(a, w, nco, ti, pv0, pv1, pos);
    }

    // the NCO runs on: phase and age after this call's n_in samples (the host keeps the same arithmetic in its
    // mirror, so a retune uploads a consistent state)
    if (seg == 0 && t == 0) {
        DcChan nx;
        nx.phase = w.cs.phase + w.cs.inc * (unsigned long long)a.n_in;
        nx.inc = w.cs.inc;
        nx.age = w.cs.age + (unsigned long long)a.n_in;
        a.chan_next[w.ch] = nx;
    }
    // calls shorter than the warm-up length keep the tail of the old history in front
    if (seg == a.nseg - 1 && a.n_in < a.W)
        for (int j = t; j < a.W - a.n_in; j += DC_T) w.hist_next[j] = w.hist[j + a.n_in];
}

// ---- launch --------------------------------------------------------------------------------------------
// the plain or the blanked kernel of plan P (DcArgs::nb_mask: the blanker's mask applied in the kernel's own loads);
// lds = dynamic LDS bytes, raised above 64 KB once per device (launch_once.hpp; never needed in practice -- a
// cascade is ~10 KB)
template <class P, bool BLK>
inline hipError_t dc_launch_form(DcArgs &a, int lds, hipStream_t stream)
{
    if (lds > 64 * 1024) {
        const hipError_t e = CSDR_MAX_LDS_ONCE((&downconv_kernel<P, BLK>), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((downconv_kernel<P, BLK>), dim3(a.nchan * a.nseg), dim3(DC_T), lds, stream, a);
    return hipGetLastError();
}
template <class P>
inline hipError_t dc_launch(DcArgs &a, int lds, hipStream_t stream)
{
    return a.nb_mask ? dc_launch_form<P, true>(a, lds, stream) : dc_launch_form<P, false>(a, lds, stream);
}

}  // namespace csdr
