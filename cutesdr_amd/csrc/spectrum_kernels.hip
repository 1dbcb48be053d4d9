// spectrum_kernels.hip -- CFft display spectrum and plain N-point transforms for gfx950 (K3).
//
// Replaces CFft::PutInDisplayFFT (reference dsp/fft.cpp:267-288: Hann*2 window, I/Q swap, forward
// transform) together with the tail of CFft::CpxFFT (:562-589: |X|^2, running mean over AveSize
// frames, log10, fft-shifted into display order), and CFft::FwdFFT / RevFFT (:416-426).
// One workgroup per channel (or frame group) walks its frames in order (the running mean makes frames sequential);
// the transform is a three-pass decimation-in-time FFT with the FMA butterflies of the overlap-save kernel
// (fft_core.hpp), its output is scattered straight into display order.  8 B in + 4 B out per bin.
// The file in the order it reads:
//   SpecJob            what a workgroup works on -- channel, frame group of how many, frame count, averaging length, frame
//                      positions, partial-sum slots -- filled from the block index (uniform form) or from the launch's
//                      table of active rows (row form); everything below reads the job, not the form
//   frame loaders      where sample i of frame f comes from: rows, rows + DC, datagrams, each behind a blanker's mask
//   transforms         Passes32 (16384 points, 32 per thread) and Wide16<PassB...> (2048 / 4096 / 8192, 16 per thread:
//                      passes A and C and the fence between B and C once, pass B per size)
//   spectrum_frames    THE frame loop: prologue, frame load with window and overload test, counters, running sum,
//                      epilogue with the display-order scatter -- each rule once, for every transform and loader
//   the kernels        spectrum_kernel<14>, spectrum8 / 16 / 32_kernel<loader, form>: launch bounds around job and loop
//   fft_plain_kernel, the frame-group weights and combine, and the launcher (one size switch for both forms, bounded by
//   the loader's largest size)
#define CSDR_FMA_BFLY 1          // FMA-form decimation-in-time butterflies (fft_core.hpp)
#define CSDR_PLAIN_CONST_FMA 1
#include "launch_once.hpp"
#include <type_traits>
#include "fft_core.hpp"
#include "spectrum_passes.hpp"
#include "spectrum_kernels.h"
#include "ref_constants.hpp"

namespace csdr {

// ---- what a workgroup works on: frame group `group` of the `groups` that the nframes frames of channel ch are cut
// into.  With groups > 1 a group accumulates its frames from zero into its slot of `part` and the combine folds the
// groups in order (the running sum is the linear map sum <- alpha_f sum + p_f).  The launch has `slots` slots per channel:
// group g's partial sums are a.part + slot(g) N, its weight a.alpha[slot(g)].
struct SpecJob {
    int ch, group, groups;
    int nframes, ave_size;            // the channel's frames in this launch and its m_AveSize
    long start, step;                 // the stream loaders: frame f at sample start + f step of the call
    int slots;
    bool own_overload;                // no launcher cleared the channel's overload word: its last group does
    __device__ __forceinline__ long slot(int g) const { return (long)ch * slots + g; }
};
// The job of entry `idx` of the launch and frame group `group`; false: that group has no frames, nothing to do.
// Uniform form: entry = channel, every value the launch's.  Row form: the entry of the launch's table of active rows
// (wave-uniform loads, once per workgroup).  A row cuts ITS frame count into groups, eight frames a group at least, and
// takes the first of the launch's nparts workgroups per row; the others leave at once.  So what a row computes depends
// on its own frames alone -- not on how many frames the other rows of the launch have -- and a row below sixteen frames
// runs the one-group path, whose words are those of the frames in order.
template <bool ROWS>
__device__ __forceinline__ bool spec_job(const SpectrumArgs &a, int idx, int group, SpecJob &j)
{
    if constexpr (ROWS) {
        const SpecRow e = a.rows[idx];
        j = SpecJob{e.row, group, spectrum_groups(e.nframes, a.nparts), e.nframes, e.ave_size, (long)e.start, (long)e.step,
                    a.nparts, true};
    } else {
        j = SpecJob{idx, group, a.nparts, a.nframes, a.ave_size, a.frame_start, a.frame_step, a.nparts, false};
        return true;             // (group < nparts by the launch's grid: said outright, the compare cost the kernels SGPRs)
    }
    return group < j.groups;
}
// frames [group_frame(g), group_frame(g + 1)) are group g's
__device__ __forceinline__ int group_frame(const SpecJob &j, int g) { return (int)((long)j.nframes * g / j.groups); }
// the average count k frames after ave0: it saturates at ave_size (a count above it -- the average was shortened -- stays);
// the total count is total0 + k
__device__ __forceinline__ int ave_count_after(int ave0, int k, int ave_size)
{
    return ave0 + k < ave_size ? ave0 + k : (ave0 > ave_size ? ave0 : ave_size);
}


// ---- frame loaders: where sample i of a channel's frame f comes from.  fetch() issues the load and returns the raw
// value, decode() turns it into the complex sample where it is consumed (a prefetched frame's decode must not make the
// prefetch wait for its own loads).
struct RowLoad {                          // csdr_fft_batch_put_display: frames back to back from the row's start
    typedef v2f Raw;
    const v2f *in;
    __device__ __forceinline__ RowLoad(const SpectrumArgs &a, const SpecJob &j)
        : in(reinterpret_cast<const v2f *>(a.in) + (long)j.ch * a.in_stride) {}
    template <int N> __device__ __forceinline__ Raw fetch(int f, int i) const { return in[(long)f * N + i]; }
    __device__ __forceinline__ v2f decode(Raw r) const { return r; }
};
// the display stream (sdrinterface.cpp:889-894): frame f at sample frame_start + f frame_step of the call, minus the DC
// offset with unpack_kernel's arithmetic (a missing dc subtracts 0.0: the same words)
struct StreamDc {
    double di, dq;
    __device__ __forceinline__ StreamDc(const SpectrumArgs &a, int ch)
        : di(a.dc ? a.dc[2 * ch] : 0.0), dq(a.dc ? a.dc[2 * ch + 1] : 0.0) {}
    // (opaque: the transform gets the sample as it gets a loaded one -- left visible, the decode changed which of the
    // first butterflies' multiplies and adds the compiler fused, and the words differed from the fp32-row forms)
    __device__ __forceinline__ v2f sub(float x, float y) const { return opaque(v2f{(float)((double)x - di), (float)((double)y - dq)}); }
};
struct RowDcLoad {                        // fp32 rows
    typedef v2f Raw;
    const v2f *in; long start, step; StreamDc dc;
    __device__ __forceinline__ RowDcLoad(const SpectrumArgs &a, const SpecJob &j)
        : in(reinterpret_cast<const v2f *>(a.in) + (long)j.ch * a.in_stride), start(j.start), step(j.step), dc(a, j.ch) {}
    template <int N> __device__ __forceinline__ Raw fetch(int f, int i) const { return in[start + (long)f * step + i]; }
    __device__ __forceinline__ v2f decode(Raw r) const { return dc.sub(r.x, r.y); }
};
struct Raw24 { unsigned h0, h1, h2; };
template <int PKT>                        // datagrams (wire_format.hpp): 1028 = 256 x 16 bit, 1444 = 240 x 24 bit
struct WireLoad {
    typedef typename std::conditional<PKT == 1444, Raw24, unsigned>::type Raw;
    const unsigned char *chan; long start, step; StreamDc dc;
    __device__ __forceinline__ WireLoad(const SpectrumArgs &a, const SpecJob &j)
        : chan(a.pk + (long)j.ch * a.pk_stride), start(j.start), step(j.step), dc(a, j.ch) {}
    template <int N> __device__ __forceinline__ Raw fetch(int f, int i) const
    {
        const unsigned s = (unsigned)(start + (long)f * step) + (unsigned)i;      // < 2^31: a call stays below 2 GiB
        if constexpr (PKT == 1444) {
            const unsigned q = s / 240u, j = s - q * 240u;
            const unsigned short *h = reinterpret_cast<const unsigned short *>(chan + (q * 1444u + 4u + 6u * j));
            return Raw24{h[0], h[1], h[2]};
        } else {
            const unsigned q = s >> 8, j = s & 255u;
            return *reinterpret_cast<const unsigned *>(chan + (q * 1028u + 4u + 4u * j));
        }
    }
    __device__ __forceinline__ v2f decode(Raw r) const
    {
        if constexpr (PKT == 1444) {              // wire_sample: value << 8 in an int32, / 65536 (exact)
            const int vi = (int)((r.h0 << 8) | ((r.h1 & 0xffu) << 24));
            const int vq = (int)(((r.h1 >> 8) << 8) | (r.h2 << 16));
            return dc.sub((float)vi * (1.0f / 65536.0f), (float)vq * (1.0f / 65536.0f));
        } else {
            return dc.sub((float)(short)(r & 0xffffu), (float)(short)(r >> 16));
        }
    }
};
// The stream frame loaders behind a blanked chain call (SpectrumArgs::nb_mask; the rule is StreamSrc's,
// display_stream_kernels.h): fetch issues the inner loader's load at s - D1 (D1 = delay_n + 1, 0 when the row's blanker is
// off) plus the mask word of s, decode yields dc.sub(0, 0) under the mask and the inner decode otherwise.  The inner
// loader's start is moved back by D1 once: its fetch is the unblanked one.  No history branch here -- a frame whose
// delayed samples reach in front of the call (first sample < NB_MAX_WIDTH / 2 + 1, the largest D1) goes through the
// gather instead (capi_fft.hip: fft_put_stream), like the frame that begins in the carry.
// The mask word's shift (s & 31) travels with the word: the wide kernels fetch samples a multiple of 32 apart, so a
// thread's shifts of one frame fold into one register.  opaque() once more behind the select, so that the transform sees
// a loaded sample whichever side it came from (the words are those of the fp32-row forms).
template <class Inner>
struct BlankedLoad {
    struct Raw { typename Inner::Raw r; unsigned m, sh; };
    Inner in; const unsigned *mrow; long start, step; v2f zero;
    __device__ __forceinline__ BlankedLoad(const SpectrumArgs &a, const SpecJob &j)
        : in(a, j), mrow(a.nb_mask + (long)j.ch * a.nb_mask_stride), start(j.start), step(j.step),
          zero(in.dc.sub(0.f, 0.f))
    {
        const NbChan *nb = a.nb_state + j.ch;
        in.start -= nb->on ? nb->delay_n + 1 : 0;         // (off: the mask pass left the row all zero, as the down-converter relies on)
    }
    template <int N> __device__ __forceinline__ Raw fetch(int f, int i) const
    {
        const unsigned s = (unsigned)(start + (long)f * step) + (unsigned)i;      // < 2^31, as in WireLoad
        return Raw{in.template fetch<N>(f, i), mrow[s >> 5], s & 31u};
    }
    __device__ __forceinline__ v2f decode(Raw r) const
    {
        const v2f v = in.decode(r.r);
        return opaque(((r.m >> r.sh) & 1u) ? zero : v);
    }
};


// ---- the transforms.  What the frame loop (spectrum_frames, below) asks of a transform type X:
//   N, T, P, LDS_BYTES    points, threads, points per thread (N = T P) and the workgroup's LDS image
//   PREFETCH              whether the samples of frame f+1 are fetched while frame f goes through its transform
//   X(a, lds), settle()   loads its resident twiddles; what it computes from them, once the prologue's loads are issued
//                         (in front of them it would wait for its own load first: a memory latency per workgroup)
//   sample(q), slot(q)    which sample of a frame the thread's q-th point is, and the place in x[] it goes to
//   keep_window, window   the window value of point q: kept from the start, or read when it is used
//   run(x, lds)           the transform (its first barrier keeps it behind the previous frame's last pass)
//   bin0(t)               the bin that x[0] of thread t holds afterwards; x[r] holds bin0 + T r

// 16384 points as 512 threads x 32 points: the three passes of spectrum_passes.hpp, their inner twiddles in LDS behind
// the data.  (2048 ... 8192 points ran here too until the sixteen-point kernels below took them over: round 4.)
template <int LOG2N>
struct Passes32 {
    static_assert(LOG2N == 14, "what follows is settled for 16384 points: a smaller size would want the prefetch back");
    using Cfg = SpecCfg<LOG2N>;
    static constexpr int N = Cfg::N, T = Cfg::T, P = 32, LDS_BYTES = Cfg::LDS_BYTES;
    // No prefetch: a workgroup is 512 threads here, two waves per SIMD and so at most 256 registers per wave; with the
    // prefetched frame on top of the points and the running sums the kernel spilled 80 of them -- 324 bytes of scratch
    // per lane -- and ran at 1.5 TB/s; the second wave of the SIMD hides the loads instead (round 4).  The window is
    // read per frame for the same reason.
    static constexpr bool PREFETCH = false;
    const int t;
    v2f *tw2;
    v2f w1[Cfg::G];
    __device__ __forceinline__ Passes32(const SpectrumArgs &a, v2f *lds) : t(threadIdx.x), tw2(lds + Cfg::LDS_DATA)
    {
        for (int i = t; i < 1024; i += T) tw2[i] = reinterpret_cast<const v2f *>(a.tw2)[i];
#pragma unroll
        for (int e = 0; e < Cfg::G; e++) w1[e] = reinterpret_cast<const v2f *>(a.tw1)[Cfg::col(t, e)];
    }
    __device__ __forceinline__ void settle() {}
    __device__ __forceinline__ int sample(int q) const { return 1024 * (q % Cfg::R0) + Cfg::col(t, q / Cfg::R0); }
    static __device__ constexpr int slot(int q) { return q; }
    __device__ __forceinline__ void keep_window(const float *, int) {}
    __device__ __forceinline__ float window(const float *win, int q) const { return win[sample(q)]; }
    __device__ __forceinline__ void run(v2f (&x)[32], v2f *lds) const { fft_fwd_passes<LOG2N>(x, lds, tw2, w1); }
    static __device__ __forceinline__ int bin0(int t) { return (t >> 5) + Cfg::R0 * (t & 31); }   // (32 R0 = T)
};

// ---- 2048 / 4096 / 8192 points as T = N / 16 threads x 16 points, N = 16 x T/16 x 16 --------------------------------
// Thirty-two points per thread with the prefetched next frame and 32 running sums are 300 registers: ONE wave per
// SIMD, its vector unit 42 % busy with nothing to overlap a wave's own LDS and memory waits.  Sixteen points per thread
// fit two waves per SIMD.  Three DIT passes in registers, n = T a + 16 b + c, B = T/16:
//   A  thread t: samples T a + t (one coalesced 8-byte load per point), DFT over a, twiddle W_N^{t ka}   -> (ka, t)
//   B  the B points b of column (ka, c): DFT over b, twiddle W_{16 B}^{c kb}, back to the same places -- what a thread
//      takes of it is the size's own (PassB2048 / 4096 / 8192)
//   C  thread t = B ka + kb: its 16 consecutive points, DFT over c                   -> bin ka + 16 kb + T kc
// B -> C stays inside the B threads that own ka: no workgroup barrier.  Rows of 16 points are 18 apart in LDS (pass C
// reads them as 16-byte pieces without bank conflicts).
__device__ __forceinline__ int pad16(int pos) { return pos + ((pos >> 4) << 1); }

// 4096: B = 16, thread (ka, c) = (t >> 4, t & 15) takes the whole column, twiddle W_256^{c kb}
struct PassB4096 {
    static constexpr int LOG2B = 4, T = 16 << LOG2B;
    v2f wB;                                                           // W_256^c = W_N^{16 c}
    __device__ __forceinline__ PassB4096(const v2f *tw1, int t) : wB(tw1[16 * (t & 15)]) {}
    __device__ __forceinline__ void operator()(v2f (&x)[16], v2f *lds, int t) const
    {
        v2f *col = lds + pad16(256 * (t >> 4)) + (t & 15);                   // point b at col[18 b]
        static_for<0, 16>([&](auto B) { x[bitrev<16>(B.value)] = lds_ld8(col + 18 * B.value); });
        dft_dit<16, +1>(x);
        v2f pw[16];
        twiddle_powers<16>(opaque(wB), pw);
        static_for<1, 16>([&](auto K) { x[K.value] = cmul(x[K.value], pw[K.value]); });
        static_for<0, 16>([&](auto K) { lds_st8(col + 18 * K.value, x[K.value]); });
    }
};

// 2048 (round 4): B = 8, the eight points b of a COLUMN PAIR per thread -- thread (ka, c pair) = (t >> 3, t & 7):
// 2 x 8 points, twiddle W_128^{c kb}; point (b, c) at lds[18 (8 ka + b) + c].  B -> C inside the eight threads that own ka.
struct PassB2048 {
    static constexpr int LOG2B = 3, T = 16 << LOG2B;
    int cp;                                                           // columns 2 cp, 2 cp + 1 of ka = t >> 3
    v2f wB0, wB1;                                                     // W_128^c = W_N^{16 c}
    __device__ __forceinline__ PassB2048(const v2f *tw1, int t)
        : cp(t & 7), wB0(tw1[16 * (2 * cp)]), wB1(tw1[16 * (2 * cp + 1)]) {}
    __device__ __forceinline__ void operator()(v2f (&)[16], v2f *lds, int t) const
    {
        v2f *cell = lds + 18 * (8 * (t >> 3)) + 2 * cp;
        v2f y0[8], y1[8];
        static_for<0, 8>([&](auto B) {
            const v4f v = *reinterpret_cast<const v4f *>(cell + 18 * B.value);
            y0[bitrev<8>(B.value)] = v2f{v.x, v.y}; y1[bitrev<8>(B.value)] = v2f{v.z, v.w};
        });
        dft_dit<8, +1>(y0);
        dft_dit<8, +1>(y1);
        v2f p0[8], p1[8];
        twiddle_powers<8>(opaque(wB0), p0);
        twiddle_powers<8>(opaque(wB1), p1);
        static_for<0, 8>([&](auto K) {
            constexpr int k = K.value;
            if constexpr (k != 0) { y0[k] = cmul(y0[k], p0[k]); y1[k] = cmul(y1[k], p1[k]); }
            *reinterpret_cast<v4f *>(cell + 18 * k) = v4f{y0[k].x, y0[k].y, y1[k].x, y1[k].y};
        });
    }
};

// 8192 (round 4): B = 32, two threads' worth.  Thirty-two points per thread would be 256 threads at 300 registers
// (2.7 TB/s); instead the column (ka, c) is split by the PARITY of b over a pair of neighbouring lanes (h = t & 1) --
// each does a 16-point DIT over its b = 2 j + h, the odd one applies W_32^{kj}, and the radix-2 butterfly that joins the
// halves takes the partner's sixteen values over the DPP quad permute (1,0,3,2): no LDS, no barrier.
//   n = 512 a + 16 b + c     k = ka + 16 kb + 512 kc     kb = kj + 16 h        LDS cell of (ka, x, c): 18 (32 ka + x) + c
//   B  thread (ka, c, h)  : DFT over b as above, twiddle W_512^{c kb}, back to rows kb of the same columns
// B -> C inside the half-wave that owns ka.  One workgroup per CU would fit twice (74 KB of LDS); registers allow one.
__device__ __forceinline__ v2f pair_swap(v2f v)           // the value of lane t ^ 1
{
    return v2f{__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v.x), 0xB1, 0xf, 0xf, false)),
               __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v.y), 0xB1, 0xf, 0xf, false))};
}
struct PassB8192 {
    static constexpr int LOG2B = 5, T = 16 << LOG2B;
    int hB, cB, kaB;                                                  // (ka, c, h)
    v2f wB;                                                           // W_512^c = W_N^{16 c}
    v2f wH;                                                           // W_512^{16 c h} = W_32^{c h} = W_N^{256 c h}, c h < 16:
    __device__ __forceinline__ PassB8192(const v2f *tw1, int t)
        : hB(t & 1), cB((t >> 1) & 15), kaB(t >> 5), wB(tw1[16 * cB])
    {                                                                 // the table holds an OCTANT of W_N at N = 8192 (W_N^1024 = e^{j pi/4})
        const int m = 256 * cB * hB;                                  // < 4096: up to three eighth turns beyond the table entry
        const v2f v = tw1[m & 1023];
        const int o = (m >> 10) & 3;
        constexpr float r = 0.70710678118654752440f;
        if (o == 0) wH = v;
        else if (o == 1) wH = v2f{r * (v.x - v.y), r * (v.x + v.y)};
        else if (o == 2) wH = v2f{-v.y, v.x};
        else wH = v2f{-r * (v.x + v.y), r * (v.x - v.y)};
    }
    __device__ __forceinline__ void operator()(v2f (&x)[16], v2f *lds, int) const
    {
        v2f *col = lds + 18 * (32 * kaB + hB) + cB;                          // point b = 2 j + h at col[36 j]
        static_for<0, 16>([&](auto J) { x[bitrev<16>(J.value)] = lds_ld8(col + 36 * J.value); });
        dft_dit<16, +1>(x);                                                   // Y_h[kj]
        // the odd half times W_32^{kj} (constants), then the butterfly with the partner lane's half
        static_for<0, 16>([&](auto K) {
            constexpr int k = K.value;
            const v2f w32 = v2f{(float)__builtin_cos(6.283185307179586476925286766559 * k / 32.0),
                                (float)__builtin_sin(6.283185307179586476925286766559 * k / 32.0)};
            const v2f mine = hB ? cmul(x[k], w32) : x[k];
            const v2f other = pair_swap(mine);
            x[k] = hB ? other - mine : mine + other;          // h = 0: Y0 + w Y1 -> kb = kj;  h = 1: Y0 - w Y1 -> kb = kj + 16
        });
        v2f pw[16];
        twiddle_powers<16>(opaque(wB), pw);                   // W_512^{c kj}
        static_for<0, 16>([&](auto K) {
            constexpr int k = K.value;
            v2f v = x[k];
            if constexpr (k != 0) v = cmul(v, pw[k]);
            v = hB ? cmul(v, wH) : v;                         // times W_512^{16 c h}
            lds_st8(lds + 18 * (32 * kaB + k + 16 * hB) + cB, v);
        });
    }
};

template <class PassB>
struct Wide16 {
    static constexpr int T = PassB::T, N = 16 * T, P = 16, LDS_BYTES = (N + 2 * T) * 8;
    static constexpr bool PREFETCH = true;
    // W_N^{t ka} stay resident (30 registers) where a thread has them: the 512 threads of 8192 points, at most 256
    // registers each, recompute them per frame as every size does pass B's
    static constexpr bool PWA_RESIDENT = T < 512;
    const int t;
    const v2f wA;                                                     // W_N^t (tw1: W_N^n, n < 1024)
    const PassB pass_b;
    v2f pwA[PWA_RESIDENT ? 16 : 1];
    float wn[16];
    __device__ __forceinline__ Wide16(const SpectrumArgs &a, v2f *)
        : t(threadIdx.x), wA(reinterpret_cast<const v2f *>(a.tw1)[t]), pass_b(reinterpret_cast<const v2f *>(a.tw1), t) {}
    __device__ __forceinline__ void settle() { if constexpr (PWA_RESIDENT) twiddle_powers<16>(wA, pwA); }
    __device__ __forceinline__ int sample(int q) const { return t + T * q; }
    static __device__ constexpr int slot(int q) { return bitrev<16>(q); }
    __device__ __forceinline__ void keep_window(const float *win, int q) { wn[q] = win[sample(q)]; }
    __device__ __forceinline__ float window(const float *, int q) const { return wn[q]; }
    __device__ __forceinline__ void run(v2f (&x)[16], v2f *lds) const
    {
        // ---- pass A
        dft_dit<16, +1>(x);
        if constexpr (PWA_RESIDENT) {
            static_for<1, 16>([&](auto K) { x[K.value] = cmul(x[K.value], pwA[K.value]); });
        } else {
            v2f pw[16];
            twiddle_powers<16>(opaque(wA), pw);
            static_for<1, 16>([&](auto K) { x[K.value] = cmul(x[K.value], pw[K.value]); });
        }
        __syncthreads();                       // the previous frame's pass C has read its rows
        static_for<0, 16>([&](auto K) { lds[pad16(T * K.value + t)] = x[K.value]; });
        __syncthreads();
        // ---- pass B
        pass_b(x, lds, t);
        // B -> C stays inside the T/16 threads that own ka
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- pass C: the 16 consecutive points of row t
        const v2f *row = lds + 18 * t;
        static_for<0, 8>([&](auto J) {
            const v4f v = *reinterpret_cast<const v4f *>(row + 2 * J.value);
            x[bitrev<16>(2 * J.value)] = v2f{v.x, v.y};
            x[bitrev<16>(2 * J.value + 1)] = v2f{v.z, v.w};
        });
        dft_dit<16, +1>(x);
    }
    // pass C row t = B ka + kb: bins ka + 16 kb + T kc
    static __device__ __forceinline__ int bin0(int t) { return (t >> PassB::LOG2B) + 16 * (t & (T / 16 - 1)); }
};

// ---- the frame loop: one workgroup walks the frames f0 ... f1 of its job through transform X, loaded by Ld ----------
template <class X, class Ld>
__device__ __forceinline__ void spectrum_frames(const SpectrumArgs &a, const SpecJob &job)
{
    constexpr int N = X::N, P = X::P;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2f *lds = reinterpret_cast<v2f *>(smem_raw);
    const int t = threadIdx.x, ch = job.ch;
    const int f0 = group_frame(job, job.group), f1 = group_frame(job, job.group + 1);
    X xf(a, lds);
    const Ld ld(a, job);
    float *sum = a.sum + (long)ch * N, *pwr = a.pwr + (long)ch * N, *ave = a.ave + (long)ch * N;
    int ave_count = a.counters[2 * ch], total = a.counters[2 * ch + 1];
    total += f0;                                              // counters at this group's first frame
    ave_count = ave_count_after(ave_count, f0, job.ave_size);
    int over = 0;
    // (a word that no launcher cleared: the group that holds the channel's last frame, never an empty one, clears it,
    // and the barriers of that frame's transform lie between this store and the one at the end)
    if (job.own_overload && t == 0 && job.group == job.groups - 1) a.overload[ch] = 0;
    // every thread owns the same P bins in every frame: the running sum and mean stay in registers
    // for the whole call, only the last frame's bels are written
    int tt = t;
    asm volatile("" : "+v"(tt));              // keep the scattered addresses out of LICM's hands
    const int bin0 = X::bin0(tt);
    auto shown = [&](int r) { return (bin0 + (X::T * r + N / 2)) & (N - 1); };     // display order, fft.cpp:564-589
    float sm[P];                              // the mean is sum / count: recomputed, not carried
    static_for<0, P>([&](auto Rr) {
        constexpr int r = Rr.value;
        sm[r] = job.groups == 1 ? sum[shown(r)] : 0.f;
        xf.keep_window(a.win, r);
    });
    xf.settle();
    // the samples of frame f+1 are fetched while frame f goes through its transform (one workgroup has only a few
    // waves and several share a CU: nothing else would hide the HBM latency of a frame's loads), as raw words
    typename Ld::Raw nxt[X::PREFETCH ? P : 1];
    auto fetch = [&](int f) {
        if constexpr (X::PREFETCH) {
#pragma unroll
            for (int q = 0; q < P; q++) nxt[q] = ld.template fetch<N>(f, xf.sample(q));
        }
    };
    if (f0 < f1) fetch(f0);
    for (int f = f0; f < f1; f++) {
        v2f x[P];
        over = 0;                                                 // m_Overload = FALSE at the top of every put, fft.cpp:270
        static_for<0, P>([&](auto Q) {
            constexpr int q = Q.value;
            v2f s;
            if constexpr (X::PREFETCH) s = ld.decode(nxt[q]); else s = ld.decode(ld.template fetch<N>(f, xf.sample(q)));
            const float w = xf.window(a.win, q);
            if (s.x > refc::FFT_OVER_LIMIT_F) over = 1;                     // OVER_LIMIT, fft.cpp:30,275
            x[X::slot(q)] = v2f{w * s.y, w * s.x};                // Hann*2, I/Q swapped, fft.cpp:280-281
        });
        if (f + 1 < f1) fetch(f + 1);
        const float prev_count = (float)ave_count;
        total++;                                                  // CpxFFT counters, fft.cpp:515-517
        if (ave_count < job.ave_size) ave_count++;
        xf.run(x, lds);
        const float inv_prev = 1.0f / prev_count;                 // (one division per frame instead of one per bin: -10 %)
        static_for<0, P>([&](auto Rr) {
            constexpr int r = Rr.value;
            const float p = x[r].x * x[r].x + x[r].y * x[r].y;
            if (total <= job.ave_size) sm[r] = sm[r] + p;
            else sm[r] = sm[r] - sm[r] * inv_prev + p;            // minus the previous mean (fft.cpp:570-574)
        });
    }
    if (job.groups > 1) {
        float *dst = a.part + job.slot(job.group) * N;
        static_for<0, P>([&](auto Rr) { dst[shown(Rr.value)] = sm[Rr.value]; });
    } else if (job.nframes > 0) {
        static_for<0, P>([&](auto Rr) {
            constexpr int r = Rr.value;
            const int j = shown(r);
            const float m = sm[r] / (float)ave_count;
            sum[j] = sm[r]; pwr[j] = m;
            ave[j] = (float)((double)log10f(m + a.kc) + a.kb);
            if constexpr (P == 32 && (r & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (32 points: the bels eight at a time)
        });
    }
    if (t == 0 && job.groups == 1) { a.counters[2 * ch] = ave_count; a.counters[2 * ch + 1] = total; }
    // the flag is the last put frame's: `over` is that of the group's last frame, and only the group that holds the
    // channel's last frame writes it
    if (over && job.group == job.groups - 1) a.overload[ch] = 1;
}
// the kernels: workgroup = (entry, frame group) of the launch's nparts groups per entry
template <class X, class Ld, bool ROWS>
__device__ __forceinline__ void spectrum_kernel_body(const SpectrumArgs &a)
{
    SpecJob job;
    if (spec_job<ROWS>(a, blockIdx.x / a.nparts, blockIdx.x % a.nparts, job)) spectrum_frames<X, Ld>(a, job);
}
template <int LOG2N, class Ld = RowLoad, bool ROWS = false>
__global__ __launch_bounds__(SpecCfg<LOG2N>::T) __attribute__((amdgpu_waves_per_eu(1)))
void spectrum_kernel(SpectrumArgs a) { spectrum_kernel_body<Passes32<LOG2N>, Ld, ROWS>(a); }
template <class Ld = RowLoad, bool ROWS = false>
__global__ __launch_bounds__(128)
void spectrum8_kernel(SpectrumArgs a) { spectrum_kernel_body<Wide16<PassB2048>, Ld, ROWS>(a); }
template <class Ld = RowLoad, bool ROWS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1)))
void spectrum16_kernel(SpectrumArgs a) { spectrum_kernel_body<Wide16<PassB4096>, Ld, ROWS>(a); }
template <class Ld = RowLoad, bool ROWS = false>
__global__ __launch_bounds__(512)
void spectrum32_kernel(SpectrumArgs a) { spectrum_kernel_body<Wide16<PassB8192>, Ld, ROWS>(a); }

// plain transform: out[k] = sum_n in[n] e^{sign j 2 pi n k / N}; sign=-1 via conjugation
template <int LOG2N>
__global__ __launch_bounds__(SpecCfg<LOG2N>::T)
void fft_plain_kernel(const v2f *in, v2f *out, const v2f *tw1g, const v2f *tw2g, int sign)
{
    using Cfg = SpecCfg<LOG2N>;
    constexpr int T = Cfg::T, R0 = Cfg::R0, G = Cfg::G;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2f *lds = reinterpret_cast<v2f *>(smem_raw);
    v2f *tw2 = lds + Cfg::LDS_DATA;
    const int t = threadIdx.x;
    for (int i = t; i < 1024; i += T) tw2[i] = tw2g[i];
    v2f w1[G];
#pragma unroll
    for (int e = 0; e < G; e++) w1[e] = tw1g[Cfg::col(t, e)];
    const float cj = sign > 0 ? 1.0f : -1.0f;
    v2f x[32];
#pragma unroll
    for (int e = 0; e < G; e++)
#pragma unroll
        for (int n1 = 0; n1 < R0; n1++) {
            const v2f s = in[1024 * n1 + Cfg::col(t, e)];
            x[e * R0 + n1] = v2f{s.x, cj * s.y};
        }
    __syncthreads();
    fft_fwd_passes<LOG2N>(x, lds, tw2, w1);
    const int k0 = t >> 5, k1 = t & 31;
    __syncthreads();                       // in == out allowed: every input was read before pass 1
    static_for<0, 32>([&](auto Rr) {
        constexpr int r = Rr.value, k2 = r;
        out[k0 + R0 * (k1 + 32 * k2)] = v2f{x[r].x, cj * x[r].y};
    });
}

// The weight alpha_g = product of the per-frame factors (1 - 1/count once the average is full) of every frame group,
// and the average count after the call: the same for all bins of a channel (the combine kernel used to do this walk in
// each of its channels x N threads: 0.18 of K3's 1.6 ms).  One thread per (channel, frame group): the counters at a
// group's first frame follow from those at the call's start in closed form, so the groups' walks -- the same float
// operations in the same order as one walk over all frames -- run side by side (round 4: one thread per channel took
// 40 us of the C1 call's 940 for its 512 sequential divisions).
// One workgroup per channel (thread g = frame group g, in rounds of the block size): once every thread has read the
// counters, thread 0 moves them -- what spectrum_count_kernel did in a launch of its own.
// The job's `groups` weights go to its slots of a.alpha, the channel's average count after the call behind all slots.
static __device__ __forceinline__ void spectrum_alpha(const SpectrumArgs &a, const SpecJob &job)
{
    const int ch = job.ch;
    float *al_out = a.alpha + job.slot(0), *after = a.alpha + (long)a.channels * a.nparts + ch;
    const int ave0 = a.counters[2 * ch], total0 = a.counters[2 * ch + 1];
    __syncthreads();
    if (threadIdx.x == 0) {
        a.counters[2 * ch] = ave_count_after(ave0, job.nframes, job.ave_size);
        a.counters[2 * ch + 1] = total0 + job.nframes;
    }
    for (int g = threadIdx.x; g < job.groups; g += blockDim.x) {
        const int f0 = group_frame(job, g), f1 = group_frame(job, g + 1);
        int ave_count = ave_count_after(ave0, f0, job.ave_size), total = total0 + f0;
        float al = 1.f;                                                // product of the group's alpha_f
        for (int f = f0; f < f1; f++) {
            const float prev = (float)ave_count;
            total++;
            if (ave_count < job.ave_size) ave_count++;
            if (total > job.ave_size) al = al - al / prev;
            if (al == 0.f) break;                                      // (no averaging: the first frame already forgets everything)
        }
        al_out[g] = al;
        if (g == 0) *after = (float)ave_count_after(ave0, job.nframes, job.ave_size);
    }
}
// One workgroup per entry.  A channel of one group is finished by its frame loop, counters included: nothing here or in
// the combine (the uniform form launches neither then; a row of one group can sit in a launch of several).  (A row
// without a frame is in no table: the count after no frame of a fresh row is 0, and the combine would divide by it.)
template <bool ROWS>
__global__ void spectrum_alpha_kernel(SpectrumArgs a)
{
    SpecJob job;
    if (spec_job<ROWS>(a, blockIdx.x, 1, job)) spectrum_alpha(a, job);       // (a second group: not a channel of one)
}
// folds the frame groups (groups > 1) into the running sum, writes mean and bels
template <bool ROWS>
__global__ void spectrum_combine_kernel(SpectrumArgs a, int n)
{
    SpecJob job;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !spec_job<ROWS>(a, blockIdx.y, 1, job)) return;
    const int ch = job.ch;
    float sm = a.sum[(long)ch * n + j];
    for (int g = 0; g < job.groups; g++)
        sm = a.alpha[job.slot(g)] * sm + a.part[job.slot(g) * n + j];
    const float m = sm / a.alpha[(long)a.channels * a.nparts + ch];
    a.sum[(long)ch * n + j] = sm; a.pwr[(long)ch * n + j] = m;
    a.ave[(long)ch * n + j] = (float)((double)log10f(m + a.kc) + a.kb);
}
// (the kernel is a template argument: CSDR_MAX_LDS_ONCE keeps its flag per launch site, so per kernel and form)
template <class X, auto Kernel, bool ROWS>
static hipError_t spec_launch_one(const SpectrumArgs &a, hipStream_t s)
{
    if constexpr (X::LDS_BYTES > 64 * 1024) {             // more LDS than a kernel gets unasked
        const hipError_t e = CSDR_MAX_LDS_ONCE(Kernel, X::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    const int rows = ROWS ? a.nrows : a.channels;
    hipLaunchKernelGGL(Kernel, dim3(rows * a.nparts), dim3(X::T), X::LDS_BYTES, s, a);
    if (a.nparts > 1) {
        hipLaunchKernelGGL(spectrum_alpha_kernel<ROWS>, dim3(rows), dim3(64), 0, s, a);
        hipLaunchKernelGGL(spectrum_combine_kernel<ROWS>, dim3(X::N / 256, rows), dim3(256), 0, s, a, (int)X::N);
    }
    return hipGetLastError();
}
// One size switch, bounded by the loader's largest size (spectrum_kernels.h; the tests against MAX_LOG2N are compile-time:
// a loader is instantiated in the kernels of ITS sizes only)
template <int MAX_LOG2N, class Ld, bool ROWS>
static hipError_t spec_launch(int log2n, const SpectrumArgs &a, hipStream_t s)
{
    if (ROWS && a.nrows < 1) return hipErrorInvalidValue;
    if (log2n == 11) return spec_launch_one<Wide16<PassB2048>, &spectrum8_kernel<Ld, ROWS>, ROWS>(a, s);
    if (log2n == 12) return spec_launch_one<Wide16<PassB4096>, &spectrum16_kernel<Ld, ROWS>, ROWS>(a, s);
    if constexpr (MAX_LOG2N >= 13) if (log2n == 13) return spec_launch_one<Wide16<PassB8192>, &spectrum32_kernel<Ld, ROWS>, ROWS>(a, s);
    if constexpr (MAX_LOG2N >= 14) if (log2n == 14) return spec_launch_one<Passes32<14>, &spectrum_kernel<14, Ld, ROWS>, ROWS>(a, s);
    return hipErrorInvalidValue;
}
template <int LOG2N>
static hipError_t plain_launch_one(int sign, const float *in, float *out, const float *tw1, const float *tw2, hipStream_t s)
{
    using Cfg = SpecCfg<LOG2N>;
    hipError_t e = CSDR_MAX_LDS_ONCE((&fft_plain_kernel<LOG2N>), Cfg::LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fft_plain_kernel<LOG2N>, dim3(1), dim3(Cfg::T), Cfg::LDS_BYTES, s, (const v2f *)in, (v2f *)out,
                       (const v2f *)tw1, (const v2f *)tw2, sign);
    return hipGetLastError();
}

hipError_t spectrum_launch(int log2n, const SpectrumArgs &a, hipStream_t stream)
{
    if (a.rows) return spec_launch<PLAIN_MAX_LOG2N, RowLoad, true>(log2n, a, stream);
    return spec_launch<PLAIN_MAX_LOG2N, RowLoad, false>(log2n, a, stream);
}
template <bool ROWS>
static hipError_t stream_launch(int log2n, const SpectrumArgs &a, int pkt_len, hipStream_t stream)
{
    if (!a.pk) return spec_launch<STREAM_MAX_LOG2N, RowDcLoad, ROWS>(log2n, a, stream);
    if (pkt_len == 1444) return spec_launch<STREAM_MAX_LOG2N, WireLoad<1444>, ROWS>(log2n, a, stream);
    if (pkt_len == 1028) return spec_launch<STREAM_MAX_LOG2N, WireLoad<1028>, ROWS>(log2n, a, stream);
    return hipErrorInvalidValue;
}
hipError_t spectrum_stream_launch(int log2n, const SpectrumArgs &a, int pkt_len, hipStream_t stream)
{
    if (a.nb_mask) {             // the row form has no blanked loaders: a blanked call's frames are gathered (capi_fft.hip)
        if (a.rows || !spectrum_stream_blanked_ok(log2n, a.pk ? pkt_len : 0)) return hipErrorInvalidValue;
        if (!a.pk) return spec_launch<BLANKED_MAX_LOG2N, BlankedLoad<RowDcLoad>, false>(log2n, a, stream);
        if (pkt_len == 1444) return spec_launch<BLANKED_MAX_LOG2N, BlankedLoad<WireLoad<1444>>, false>(log2n, a, stream);
        return spec_launch<BLANKED_MAX_LOG2N, BlankedLoad<WireLoad<1028>>, false>(log2n, a, stream);
    }
    return a.rows ? stream_launch<true>(log2n, a, pkt_len, stream) : stream_launch<false>(log2n, a, pkt_len, stream);
}
hipError_t fft_plain_launch(int log2n, int sign, const float *in, float *out, const float *tw1,
                            const float *tw2, hipStream_t stream)
{
    switch (log2n) {
    case 11: return plain_launch_one<11>(sign, in, out, tw1, tw2, stream);
    case 12: return plain_launch_one<12>(sign, in, out, tw1, tw2, stream);
    case 13: return plain_launch_one<13>(sign, in, out, tw1, tw2, stream);
    case 14: return plain_launch_one<14>(sign, in, out, tw1, tw2, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace csdr
