// noiseblank_kernels.hip -- the noise blanker in front of the down-converter (K6 in DESIGN.md).
//
// noiseblank_kernel replaces CNoiseProc::ProcessBlanker (dsp/noiseproc.cpp:121-176).  The reference
// loop looks sequential (running sum, blank counter) but carries no true recurrence:
//   mag_i   = max(|re_i|, |im_i|)
//   S_i     = sum of the last mag_n+1 magnitudes           (moving sum, :143-147)
//   trig_i  = mag_i * ratio > S_i                          (:155-158)
//   blank_i = a trigger among the last width_n samples     (the counter reloaded by each trigger, :160-166)
//   out_i   = blank_i ? 0 : x_{i-delay_n-1}                (delay ring of delay_n+1 entries, :150-153)
// so S is S_start + prefix-sum(mag_i - mag_{i-mag_n-1}) in fp64 and the blank window is a prefix-max
// of trigger positions.  One workgroup per channel and segment of the call (nb_host.hpp: nb_segments) walks its
// segment in tiles of NB_T threads x 4 or 8 samples.  START: the state the call (or, for a later segment, a reduction
// over the window in front of it) begins with.  Per TILE: take the prefetched samples, read the magnitudes leaving the
// window, thread-local prefix, ring store, fetch ahead, block sum, triggers, block max of trigger positions, emit.
// FINISH: the state and the history the next call begins with.  Samples older than the call come from a per-channel
// history of the last NB_HIST raw inputs.
#include "launch_once.hpp"
#include "nb_host.hpp"
#include "wave_dpp.hpp"

namespace csdr {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(8)));
constexpr int NB_T = NB_THREADS, NB_WAVES = NB_T / 64;
// MASK: the kernel's mask mode as an instantiation of its own (no third input stream, no sample output: fewer
// registers, more waves).
// RING: the magnitudes of a workgroup's last NB_RING samples stay in LDS, so that the sample LEAVING the
// moving-sum window -- mag_n + 1 = 10 001 samples, 60 KB of datagrams, behind the new one -- is not fetched and decoded
// a second time.  That second stream was half of the mask form's traffic (counters: 2 x 3.23 GB at the fabric per
// launch of the C4 share, 4.8 TB/s -- the 96 windows of an XCD's resident workgroups are 5.8 MB against 4 MB of L2,
// so the Infinity Cache served it, not L2).  An instantiation of its own, so that neither form carries the other's
// registers; the two-stream form runs where a window does not fit the ring (nb_host.hpp: nb_choose_form).
// The sample form (three streams: new, leaving, delayed; fp32 rows out) takes the ring too, four samples per thread: its
// leaving stream was a third of 24 B per sample at the fabric.  (Round 3 tried a ring there -- 44 KB per 256-thread
// workgroup, every channel -- and dropped it: 3.36 against 2.86 ms.)
template <bool MASK, bool RING> struct NbTile { static constexpr int PER = nb_per_thread(MASK, RING), TILE = nb_tile(MASK, RING); };

// ---- wave scans (wave_dpp.hpp) ---------------------------------------------------------------------------------
__device__ __forceinline__ double wave_incl_scan_add(double v)
{
#define NB_STEP(C_, R_) v += __longlong_as_double((long long)wave_dpp64<C_, R_>((unsigned long long)__double_as_longlong(v), 0ull));
    WAVE_SCAN_STEPS(NB_STEP)
#undef NB_STEP
    return v;
}
__device__ __forceinline__ long long wave_incl_scan_add(long long v)
{
#define NB_STEP(C_, R_) v += (long long)wave_dpp64<C_, R_>((unsigned long long)v, 0ull);
    WAVE_SCAN_STEPS(NB_STEP)
#undef NB_STEP
    return v;
}
// the same for a value whose sixteen-lane row sums fit 32 bits (|v| < 2^27): the four steps inside a row are one
// v_add_u32 with a DPP operand each, only the two steps across rows carry 64 bits
__device__ __forceinline__ long long wave_incl_scan_add_i27(int v)
{
#define NB_STEP(C_, R_) v += __builtin_amdgcn_update_dpp(0, v, C_, R_, 0xf, false);
    NB_STEP(0x111, 0xf) NB_STEP(0x112, 0xf) NB_STEP(0x114, 0xf) NB_STEP(0x118, 0xf)
#undef NB_STEP
    long long w = (long long)v;
    w += (long long)wave_dpp64<0x142, 0xa>((unsigned long long)w, 0ull);
    w += (long long)wave_dpp64<0x143, 0xc>((unsigned long long)w, 0ull);
    return w;
}
// trigger positions inside a tile are 32-bit offsets from the tile's first sample (NB_NEVER: none; an older trigger
// is clamped to it -- the longest blank width is a few tiles)
constexpr int NB_NEVER = -(1 << 30);
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int nb_dpp_max(int v)
{
    const int o = __builtin_amdgcn_update_dpp(NB_NEVER, v, CTRL, ROW_MASK, 0xf, false);
    return o > v ? o : v;
}
__device__ __forceinline__ int wave_incl_scan_max(int v)
{
#define NB_STEP(C_, R_) v = nb_dpp_max<C_, R_>(v);
    WAVE_SCAN_STEPS(NB_STEP)
#undef NB_STEP
    return v;
}
// the value of the lane in front (lane 0: NB_NEVER)
__device__ __forceinline__ int wave_prev_lane(int v) { return __builtin_amdgcn_update_dpp(NB_NEVER, v, WAVE_SHR1, 0xf, 0xf, false); }

// ---- what both kernels are made of -------------------------------------------------------------------------------
// this workgroup's channel and its segment [a, b) of the call
struct NbSeg {
    int ch, seg;
    long a, b;
    bool last;
    __device__ __forceinline__ explicit NbSeg(const NbArgs &A)
    {
        ch = blockIdx.x / A.nseg; seg = blockIdx.x % A.nseg;
        a = (long)seg * A.seg_len;
        b = a + A.seg_len < A.n ? a + A.seg_len : A.n;
        last = seg == A.nseg - 1;
    }
};
// a tile's part of the segment, as offsets from the tile's first sample: samples [0, nvalid) lie in front of the
// segment's end, [0, nskip) are a later segment's warm-up (outputs dropped)
struct NbSpan {
    int nvalid, nskip;
    __device__ __forceinline__ NbSpan(const NbSeg &s, long base, int tile)
    {
        const long left = s.b - base, lead = s.a - base;
        nvalid = left < tile ? (int)left : tile; nskip = lead > 0 ? (int)lead : 0;
    }
};
// the running state of a segment: moving sum in front of the next tile, index of the last trigger relative to the
// call (<= -1 at the start), first sample to walk (a later segment starts a warm-up ahead of itself)
template <class Sum> struct NbRun { Sum S0; long long last; long first; };

// sample i of [history | call], i >= -NB_HIST: from the float rows or decoded from the datagrams as they arrived.
// FMT 0: rows or datagrams, the format at run time; 1444 / 1028: datagrams of that format
template <int FMT>
struct NbSrc {
    const f2 *in, *hist;
    const unsigned char *pk;
    int pkt_len;
    __device__ __forceinline__ NbSrc(const NbArgs &a, int ch)
    {
        in = reinterpret_cast<const f2 *>(a.in) + (long)ch * a.in_stride;
        hist = reinterpret_cast<const f2 *>(a.hist) + (long)ch * NB_HIST;
        pk = FMT || a.wire.pk ? a.wire.pk + (long)ch * a.wire.chan_stride : nullptr;
        pkt_len = FMT ? FMT : a.wire.pkt_len;
    }
    __device__ __forceinline__ f2 call(long i) const { return FMT ? wire_sample(pk, FMT, i) : (pk ? wire_sample(pk, pkt_len, i) : in[i]); }
    __device__ __forceinline__ f2 operator()(long i) const { return i >= 0 ? call(i) : hist[NB_HIST + i]; }
};

// sample i counted around the ring (start-up paths only: a tile's own position advances by the tile)
__device__ __forceinline__ int nb_ring_pos(long i) { const int r = (int)(i % NB_RING); return r < 0 ? r + NB_RING : r; }
// The two kinds of magnitude and their ring: fp32 magnitudes into an fp64 sum, ring slot = sample index mod NB_RING;
// or integers in units of 2^-8 into a 64-bit sum (the integer kernel, below), the ring in EIGHT PLANES: sample s of the
// stream (counted so that tiles start at multiples of the tile) sits in plane s mod 8 at word (s div 8) mod NB_RING / 8.
struct NbFloatMag {
    typedef float Mag; typedef double Sum;
    static __device__ __forceinline__ float of(f2 v) { return fmaxf(fabsf(v.x), fabsf(v.y)); }
    static __device__ __forceinline__ int slot(long i) { return nb_ring_pos(i); }
};
struct NbIntMag {
    typedef int Mag; typedef long long Sum;
    static constexpr int PLANE = NB_RING / 8;
    static_assert((PLANE & (PLANE - 1)) == 0 && nb_tile(true, true) / 8 <= PLANE, "plane words are a power of two");
    // (the history holds the floats of earlier datagrams: integral)
    static __device__ __forceinline__ int of(f2 v) { return (int)(NbFloatMag::of(v) * 256.0f); }
    static __device__ __forceinline__ int slot(long i) { return (int)(i & 7) * PLANE + (int)((i >> 3) & (PLANE - 1)); }
};

// START of a segment.  The call's first segment continues from the state the last call left; with a ring, the window
// in front of the call goes into it from the history, once per channel and call.  A later segment rebuilds its start
// state: the moving sum at its warm-up origin is a plain reduction over the mag_n+1 samples before it (which is the
// window the first tile needs in the ring), and width_n samples of warm-up (outputs dropped) recover the blank window
// that may reach into the segment.
template <class K, bool RING, class Src>
__device__ __forceinline__ void nb_seg_start(const NbSeg &s, const Src &X, int M1, int W, int tile, typename K::Mag *ring,
                                             typename K::Sum *wsum, NbRun<typename K::Sum> &r)
{
    const int t = threadIdx.x;
    if (s.seg == 0) {
        if (RING) {
            for (long k = -(long)M1 + t; k < 0; k += NB_T) ring[K::slot(k)] = K::of(X(k));
            __syncthreads();
        }
        return;
    }
    r.first = s.a - (long)((W + tile - 1) / tile) * tile;       // >= 0: a segment is at least four warm-ups long (nb_host.hpp)
    typename K::Sum part = 0;
    for (long k = r.first - M1 + t; k < r.first; k += NB_T) {
        const typename K::Mag m = K::of(X(k));
        part += (typename K::Sum)m;
        if (RING) ring[K::slot(k)] = m;
    }
    part = wave_incl_scan_add(part);
    if ((t & 63) == 63) wsum[t >> 6] = part;
    __syncthreads();
    r.S0 = 0;
    for (int q = 0; q < NB_WAVES; q++) r.S0 += wsum[q];
    r.last = -(1LL << 40);
    __syncthreads();
}

// FINISH: the last segment writes the state after the call (C: the state at its start; sum, last: where an `on` channel
// arrived) and the next call's history; a channel with the blanker off blanks nothing (and the consumer of a mask
// applies no delay) or passes its data through (:125-129).
template <bool MASK, class Src>
__device__ __forceinline__ void nb_finish(const NbArgs &a, const NbSeg &s, const NbChan &C, const Src &X, double sum, long long last)
{
    const int t = threadIdx.x;
    if (t == 0 && s.last) {
        NbChan N = C;
        if (C.on) {
            N.sum = sum;
            const long long age = (long long)a.n - last;
            N.since_trig = age > (1LL << 40) ? 1LL << 40 : age;
        }
        a.chan_next[s.ch] = N;
    }
    if (!C.on && MASK) {
        unsigned *mrow = a.mask + (long)s.ch * a.mask_stride;
        for (long wv = (s.a >> 5) + t; wv < ((s.b + 31) >> 5); wv += NB_T) mrow[wv] = 0u;
    }
    if (!C.on && !MASK && (X.pk || a.out != a.in)) {
        f2 *out = reinterpret_cast<f2 *>(a.out) + (long)s.ch * a.out_stride;
        for (long i = s.a + t; i < s.b; i += NB_T) out[i] = X.call(i);
    }
    // the last NB_HIST inputs of [history | this call] are the next call's history
    if (s.last) {
        f2 *hist_next = reinterpret_cast<f2 *>(a.hist_next) + (long)s.ch * NB_HIST;
        for (long j = t; j < NB_HIST; j += NB_T) hist_next[j] = X((long)a.n - NB_HIST + j);
    }
}

__device__ __forceinline__ int nb_last_rel(long long last, long base)    // the last trigger as an offset from the tile: <= -1
{
    const long long ago = last - (long long)base;
    return ago < (long long)NB_NEVER ? NB_NEVER : (int)ago;
}
// EMIT, mask form.  A thread's blank flags -- bit k: its sample k lies within W of the latest trigger at or before it
// (lt[k]: among the thread's own samples, before: in front of them) -- are a nibble (a byte with eight samples per
// thread) ...
template <int PER>
__device__ __forceinline__ unsigned nb_blank_flags(const int (&lt)[PER], int before, int W, int nvalid)
{
    unsigned nib = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int r = threadIdx.x * PER + k;
        const int l = lt[k] > before ? lt[k] : before;
        if (r < nvalid && r - l < W) nib |= 1u << k;
    }
    return nib;
}
// ... and eight (four) neighbouring lanes make a word of the mask row (tiles start at multiples of the tile length, so
// words never straddle tiles; a warm-up tile is skipped whole).  QUAD: the integer kernel's exchange, four lanes in two
// quad-perm DPP steps; else the general kernel's, __shfl_xor over the LPW = 4 or 8 lanes of a word.
template <int PER, bool QUAD>
__device__ __forceinline__ void nb_put_mask_word(unsigned *mrow, long base, unsigned nib, bool keep)
{
    constexpr int LPW = 32 / PER;                               // lanes per mask word
    static_assert(32 % PER == 0, "a thread's samples are a whole fraction of a mask word");
    const int t = threadIdx.x, sub = t & (LPW - 1);
    unsigned wv = nib << (PER * sub);
    if constexpr (QUAD) {
        static_assert(LPW == 4, "four lanes make a mask word: one quad");
        wv |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)wv, 0xb1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
        wv |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)wv, 0x4e, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
    } else {
#pragma unroll
        for (int sh = 1; sh < LPW; sh <<= 1) wv |= (unsigned)__shfl_xor((int)wv, sh);
    }
    if (sub == 0 && keep) mrow[(base + (long)t * PER) >> 5] = wv;
}

// ---- the general kernel: fp32 magnitudes, samples from rows or datagrams ---------------------------------------------
// The three loads of a tile (new sample, the one leaving the window, the delayed one) are issued one tile ahead, so that
// they are in flight while the current tile goes through its scans.
// pw: the prefetched tile.  Three streams x PER samples as fp32 pairs (stream s at 2 * PER * s); or, for a tile
// inside 24-bit datagrams, the raw words (new stream: NP = PER / 2 sample pairs = 3 NP words at 0; leaving and delayed
// stream: NP + 1 pairs each, at 3 NP and 6 NP + 3 -- a stream that starts on an odd sample touches one pair more); or, for
// the ring's mask form inside 16-bit datagrams, the PER raw words of the new stream.  Raw words are decoded where they
// are consumed, so that the fetch does not wait for itself.  A stream the form does not have (leaving: RING, delayed:
// MASK) is neither fetched nor taken.
template <bool MASK, bool RING>
struct NbPrefetch {
    static constexpr int PER = NbTile<MASK, RING>::PER, TILE = NbTile<MASK, RING>::TILE, NP = PER / 2;
    static_assert(PER % 2 == 0 && 240 % PER == 0 && 256 % PER == 0, "a thread's samples are whole sample pairs of one datagram");
    unsigned pw[6 * PER];
    bool raw24 = false, raw16 = false;                          // uniform: what the last fetch left in pw
    int M1, D1;                                                 // the lags of the leaving and of the delayed stream

    __device__ __forceinline__ void put(int s, int k, f2 v) { pw[2 * PER * s + 2 * k] = __float_as_uint(v.x); pw[2 * PER * s + 2 * k + 1] = __float_as_uint(v.y); }
    __device__ __forceinline__ f2 get(int s, int k) const { return f2{__uint_as_float(pw[2 * PER * s + 2 * k]), __uint_as_float(pw[2 * PER * s + 2 * k + 1])}; }
    static __device__ __forceinline__ void pair_words(const unsigned char *pk, unsigned e, unsigned *dst)      // e even
    {
        const unsigned *wp = wire_words24(pk, e);
        dst[0] = wp[0]; dst[1] = wp[1]; dst[2] = wp[2];
    }
    // 24-bit datagrams: a sample pair (even index) is 12 bytes at a 4-byte aligned offset and never straddles a
    // datagram; a thread's samples of a stream are NP pairs (even start) or parts of NP + 1 (odd start)
    __device__ __forceinline__ void fetch24(const unsigned char *pk, unsigned i0)
    {
        const unsigned eo = (i0 - (unsigned)M1) & ~1u, ed = (i0 - (unsigned)D1) & ~1u;
        if constexpr (RING && MASK) {
            // (a thread's samples start at a multiple of PER, which divides 240: they lie in ONE datagram, 6 bytes
            // apart -- one division instead of one per pair)
            const unsigned *wp = wire_words24(pk, i0);
#pragma unroll
            for (int k = 0; k < 3 * NP; k++) pw[k] = wp[k];
        } else {
#pragma unroll
            for (int p = 0; p < NP; p++) pair_words(pk, i0 + 2u * p, pw + 3 * p);
        }
        if (!RING) {
#pragma unroll
            for (int p = 0; p < NP; p++) pair_words(pk, eo + 2u * p, pw + 3 * NP + 3 * p);
            if (M1 & 1) pair_words(pk, eo + 2u * NP, pw + 6 * NP);      // (uniform) an odd start touches one pair more
        }
        if (!MASK) {
#pragma unroll
            for (int p = 0; p <= NP; p++) pair_words(pk, ed + 2u * p, pw + 6 * NP + 3 + 3 * p);
        }
        raw24 = true;
    }
    // 16-bit datagrams, the ring's mask form (no second or third stream to fetch): a sample is one word, 256 to a
    // datagram, a thread's samples contiguous inside one -- plain word loads (the per-sample path below cost the
    // 16-bit chain a third more in this kernel: 1.43 against 1.07 ms)
    __device__ __forceinline__ void fetch16(const unsigned char *pk, unsigned i0)
    {
        const unsigned *wp = wire_words16(pk, i0);
#pragma unroll
        for (int k = 0; k < PER; k++) pw[k] = wp[k];
        raw16 = true;
    }
    // float rows: a thread's samples of each stream are contiguous: 16-byte loads (the leaving and the delayed
    // stream are only 8-byte aligned, which a global dwordx4 load accepts).  The delayed stream goes first: the
    // compiler moves half of one of its registers right behind the loads, and waits for that load alone only if it is
    // the oldest in flight (new stream first: 2.08 against 2.03 ms for 256 receivers x 2^21, sample form with the ring)
    __device__ __forceinline__ void row_stream(const f2 *q, int s)
    {
#pragma unroll
        for (int k = 0; k < PER; k += 2) {
            const f4u v = *reinterpret_cast<const f4u *>(q + k);
            put(s, k, f2{v.x, v.y}); put(s, k + 1, f2{v.z, v.w});
        }
    }
    __device__ __forceinline__ void fetch_rows(const f2 *p)
    {
        if (!MASK) row_stream(p - D1, 2);
        if (!RING) row_stream(p - M1, 1);
        row_stream(p, 0);
    }
    // any source, sample by sample with bounds: the first tiles of a call (streams that begin in the history) and a
    // segment's last one
    template <class Src>
    __device__ __forceinline__ void fetch_edge(const Src &X, long i0, long seg_b)
    {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const long i = i0 + k;
            if (i < seg_b) { put(0, k, X.call(i)); if (!RING) put(1, k, X(i - M1)); if (!MASK) put(2, k, X(i - D1)); }
        }
    }
    // the tile at b0: all of its streams inside this call's input and the segment -> plain loads, no bounds
    template <class Src>
    __device__ __forceinline__ void fetch(const Src &X, long b0, long seg_b)
    {
        const bool inside = (RING || b0 - M1 >= 0) && (MASK || b0 - D1 >= 0) && b0 + TILE <= seg_b;
        const long i0 = b0 + (long)threadIdx.x * PER;
        raw24 = false; raw16 = false;
        if (X.pk && X.pkt_len == 1444 && inside) fetch24(X.pk, (unsigned)i0);
        else if (RING && MASK && X.pk && X.pkt_len == 1028 && inside) fetch16(X.pk, (unsigned)i0);
        else if (!X.pk && inside) fetch_rows(X.in + i0);
        else fetch_edge(X, i0, seg_b);
    }

    static __device__ __forceinline__ void pair(const unsigned *w, f2 &a, f2 &b)
    {
        const wf4 v = wire_pair_decode(wf4{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), 0.f}, 1444);
        a = f2{v.x, v.y}; b = f2{v.z, v.w};
    }
    static __device__ __forceinline__ void pairs(const unsigned *w, bool odd, f2 *dst)   // odd is uniform: each side decodes what it needs
    {
        f2 skip;
        if (odd) {
            pair(w, skip, dst[0]);
#pragma unroll
            for (int p = 1; p < NP; p++) pair(w + 3 * p, dst[2 * p - 1], dst[2 * p]);
            pair(w + 3 * NP, dst[PER - 1], skip);
        } else {
#pragma unroll
            for (int p = 0; p < NP; p++) pair(w + 3 * p, dst[2 * p], dst[2 * p + 1]);
        }
    }
    __device__ __forceinline__ void take24(f2 *x, f2 *xo, f2 *xdl) const
    {
#pragma unroll
        for (int p = 0; p < NP; p++) pair(pw + 3 * p, x[2 * p], x[2 * p + 1]);
        if (!RING) pairs(pw + 3 * NP, M1 & 1, xo);
        if (!MASK) pairs(pw + 6 * NP + 3, D1 & 1, xdl);
    }
    __device__ __forceinline__ void take16(f2 *x) const
    {
#pragma unroll
        for (int k = 0; k < PER; k++) x[k] = f2{(float)(short)(pw[k] & 0xffffu), (float)(short)(pw[k] >> 16)};   // (I low half, Q high half: wire_format.hpp)
    }
    __device__ __forceinline__ void take_floats(f2 *x, f2 *xo, f2 *xdl) const
    {
#pragma unroll
        for (int k = 0; k < PER; k++) { x[k] = get(0, k); if (!RING) xo[k] = get(1, k); if (!MASK) xdl[k] = get(2, k); }
    }
    // the prefetched tile as samples: new, leaving, delayed
    __device__ __forceinline__ void take(f2 *x, f2 *xo, f2 *xdl) const
    {
        if (raw16) take16(x);
        else if (raw24) take24(x, xo, xdl);
        else take_floats(x, xo, xdl);
    }
};

// The magnitudes leaving the window, linear ring: a thread's PER of them start at an arbitrary (uniform) offset from a
// 16-byte boundary of the ring: PER / 4 + 1 aligned reads, picked apart by that offset.  rb: ring slot of the tile's
// first sample
template <int PER>
__device__ __forceinline__ void nb_far_linear(const float *ring, int rb, int M1, float (&far)[PER])
{
    int f0 = rb - M1 + (int)threadIdx.x * PER;                  // > -NB_RING
    f0 = f0 < 0 ? f0 + NB_RING : f0;
    const float4 *src = reinterpret_cast<const float4 *>(ring);
    float q[PER + 4];
#pragma unroll
    for (int v = 0; v <= PER / 4; v++) {
        int fv = (f0 >> 2) + v;                                 // (NB_RING is a multiple of four: no 16-byte read straddles the wrap)
        fv = fv >= NB_RING / 4 ? fv - NB_RING / 4 : fv;
        const float4 w4 = src[fv];
        q[4 * v] = w4.x; q[4 * v + 1] = w4.y; q[4 * v + 2] = w4.z; q[4 * v + 3] = w4.w;
    }
    switch ((unsigned)(-M1) & 3u) {                             // = f0 & 3: the tile and the thread start at multiples of four
#define NB_PICK(O_) case O_: _Pragma("unroll") for (int k = 0; k < PER; k++) far[k] = q[O_ + k]; break;
        NB_PICK(0) NB_PICK(1) NB_PICK(2) default: NB_PICK(3)
#undef NB_PICK
    }
}
// this tile's magnitudes into the ring: read again mag_n + 1 samples from now
template <int PER>
__device__ __forceinline__ void nb_ring_store(float *ring, int rb, const float (&mag)[PER])
{
    float4 *dst = reinterpret_cast<float4 *>(ring) + ((rb + (int)threadIdx.x * PER) >> 2);
#pragma unroll
    for (int v = 0; v < PER / 4; v++) dst[v] = make_float4(mag[4 * v], mag[4 * v + 1], mag[4 * v + 2], mag[4 * v + 3]);
}
// block sum: off = the moving sum in front of this thread's samples, total = the tile's change of it (first barrier)
__device__ __forceinline__ void nb_block_sum(double run, double S0, double *wsum, double &off, double &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double incl = wave_incl_scan_add(run);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    off = S0 + (incl - run);
    for (int q = 0; q < w; q++) off += wsum[q];
    total = 0.0;
    for (int q = 0; q < NB_WAVES; q++) total += wsum[q];
}
// block max of trigger positions: before = the latest trigger in front of this thread's samples (last_rel: in front of
// the tile), tile_last = the tile's latest (second barrier)
__device__ __forceinline__ void nb_block_max(int runmax, int last_rel, int *wmax, int &before, int &tile_last)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inclm = wave_incl_scan_max(runmax);
    if (lane == 63) wmax[w] = inclm;
    __syncthreads();
    before = last_rel;
    for (int q = 0; q < w; q++) before = wmax[q] > before ? wmax[q] : before;
    const int upto = wave_prev_lane(inclm);
    if (upto > before) before = upto;
    tile_last = NB_NEVER;
    for (int q = 0; q < NB_WAVES; q++) tile_last = wmax[q] > tile_last ? wmax[q] : tile_last;
}

template <bool MASK, bool RING = false>
__global__ __launch_bounds__(NB_T)
void noiseblank_kernel(NbArgs a)
{
    constexpr int PER = NbTile<MASK, RING>::PER, TILE = NbTile<MASK, RING>::TILE;
    __shared__ double wsum[NB_WAVES];
    __shared__ int wmax[NB_WAVES];
    extern __shared__ __attribute__((aligned(16))) float nb_ring[];    // [NB_RING] (RING)
    const NbSeg s(a);
    const int t = threadIdx.x;
    const NbChan C = a.chan[s.ch];                          // state at the start of the call (the last segment writes chan_next)
    const NbSrc<0> X(a, s.ch);
    f2 *out = reinterpret_cast<f2 *>(a.out) + (long)s.ch * a.out_stride;
    unsigned *mrow = MASK ? a.mask + (long)s.ch * a.mask_stride : nullptr;
    NbRun<double> r{C.sum, -C.since_trig, 0};
    if (C.on) {
        const int M1 = C.mag_n + 1, W = C.width_n;          // (RING: the host has checked TILE <= M1 <= NB_RING - TILE)
        const double ratio = C.ratio;
        nb_seg_start<NbFloatMag, RING>(s, X, M1, W, TILE, nb_ring, wsum, r);
        NbPrefetch<MASK, RING> pf;
        pf.M1 = M1; pf.D1 = C.delay_n + 1;
        pf.fetch(X, r.first, s.b);
        int rb = RING ? nb_ring_pos(r.first) : 0;          // ring slot of the tile's first sample (tiles divide the ring)
        for (long base = r.first; base < s.b; base += TILE) {
            f2 xn[PER], xl[PER], xd[PER];                   // new, leaving the window, delayed
            float mag[PER], far[PER];
            double d[PER], run = 0.0;
            pf.take(xn, xl, xd);
            if constexpr (RING) nb_far_linear<PER>(nb_ring, rb, M1, far);
#pragma unroll
            for (int k = 0; k < PER; k++) {
                mag[k] = 0.f; d[k] = 0.0;
                if (base + (long)t * PER + k < s.b) {
                    mag[k] = NbFloatMag::of(xn[k]);
                    d[k] = (double)mag[k] - (double)(RING ? far[k] : NbFloatMag::of(xl[k]));
                }
                run += d[k];
                d[k] = run;                                 // thread-local inclusive prefix
            }
            if constexpr (RING) nb_ring_store<PER>(nb_ring, rb, mag);
            if (base + TILE < s.b) pf.fetch(X, base + TILE, s.b);      // (before the scans: in flight while they run)
            double off, total;
            nb_block_sum(run, r.S0, wsum, off, total);
            // triggers and the position of the latest one at or before each sample, as offsets from `base`
            const NbSpan v(s, base, TILE);
            int lt[PER], runmax = NB_NEVER;
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int p = t * PER + k;
                const bool trig = p < v.nvalid && (double)mag[k] * ratio > off + d[k];
                if (trig) runmax = p;
                lt[k] = runmax;
            }
            int before, tile_last;
            nb_block_max(runmax, nb_last_rel(r.last, base), wmax, before, tile_last);
            if constexpr (MASK) {
                nb_put_mask_word<PER, false>(mrow, base, nb_blank_flags<PER>(lt, before, W, v.nvalid), v.nskip == 0 && t * PER < v.nvalid);
            } else {
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int p = t * PER + k;
                    const int l = lt[k] > before ? lt[k] : before;
                    if (p < v.nvalid && p >= v.nskip) out[base + p] = (p - l < W) ? f2{0.f, 0.f} : xd[k];
                }
            }
            r.S0 += total;
            if (RING) { rb += TILE; rb = rb >= NB_RING ? rb - NB_RING : rb; }
            if (tile_last > NB_NEVER) r.last = (long long)base + tile_last;
            __syncthreads();                                // wsum / wmax reused by the next tile
        }
    }
    nb_finish<MASK>(a, s, C, X, r.S0, r.last);
}

// ---- the trace form: m_TestBenchDataBuf (noiseproc.cpp:159-175, PROFILE_7) -------------------------------------------
// What a user of the reference looks at to set threshold and width: re = m_MagAveSum / m_Ratio (0 while blanking),
// im = oldest.re + oldest.im, the delayed sample; a channel with the blanker off shows its input (:127).  The sample
// form's tile steps over the samples of a call that has ALREADY run, from the state and history that call began with
// (a.chan, a.hist: the halves the call read; capi_frontend.hip): the same ring choice, the same segments, so the same
// sums in the same order and the same decisions.  It has no sample output and no FINISH -- a.out is the trace row,
// nothing else is written -- and it is a kernel of its own, so that the sample form does not carry the division's and
// the wide stores' registers.  A thread's four trace entries are 32 contiguous bytes: two 16-byte stores (rows 16-byte
// aligned, stride even: tiles and threads start on even samples), 8-byte ones at the ends of a segment.
template <bool RING>
__global__ __launch_bounds__(NB_T)
void noiseblank_trace_kernel(NbArgs a)
{
    constexpr int PER = NbTile<false, RING>::PER, TILE = NbTile<false, RING>::TILE;
    static_assert(PER % 2 == 0, "a thread's trace entries are whole 16-byte pairs");
    __shared__ double wsum[NB_WAVES];
    __shared__ int wmax[NB_WAVES];
    extern __shared__ __attribute__((aligned(16))) float nb_ring[];    // [NB_RING] (RING)
    const NbSeg s(a);
    const int t = threadIdx.x;
    const NbChan C = a.chan[s.ch];                          // state at the start of the traced call
    const NbSrc<0> X(a, s.ch);
    f2 *tr = reinterpret_cast<f2 *>(a.out) + (long)s.ch * a.out_stride;
    if (!C.on) {
        for (long i = s.a + t; i < s.b; i += NB_T) tr[i] = X.call(i);
        return;
    }
    NbRun<double> r{C.sum, -C.since_trig, 0};
    const int M1 = C.mag_n + 1, W = C.width_n;
    const double ratio = C.ratio;
    nb_seg_start<NbFloatMag, RING>(s, X, M1, W, TILE, nb_ring, wsum, r);
    NbPrefetch<false, RING> pf;
    pf.M1 = M1; pf.D1 = C.delay_n + 1;
    pf.fetch(X, r.first, s.b);
    int rb = RING ? nb_ring_pos(r.first) : 0;
    for (long base = r.first; base < s.b; base += TILE) {
        f2 xn[PER], xl[PER], xd[PER];
        float mag[PER], far[PER];
        double d[PER], run = 0.0;
        pf.take(xn, xl, xd);
        if constexpr (RING) nb_far_linear<PER>(nb_ring, rb, M1, far);
#pragma unroll
        for (int k = 0; k < PER; k++) {
            mag[k] = 0.f; d[k] = 0.0;
            if (base + (long)t * PER + k < s.b) {
                mag[k] = NbFloatMag::of(xn[k]);
                d[k] = (double)mag[k] - (double)(RING ? far[k] : NbFloatMag::of(xl[k]));
            }
            run += d[k];
            d[k] = run;
        }
        if constexpr (RING) nb_ring_store<PER>(nb_ring, rb, mag);
        if (base + TILE < s.b) pf.fetch(X, base + TILE, s.b);
        double off, total;
        nb_block_sum(run, r.S0, wsum, off, total);
        const NbSpan v(s, base, TILE);
        int lt[PER], runmax = NB_NEVER;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int p = t * PER + k;
            const bool trig = p < v.nvalid && (double)mag[k] * ratio > off + d[k];
            if (trig) runmax = p;
            lt[k] = runmax;
        }
        int before, tile_last;
        nb_block_max(runmax, nb_last_rel(r.last, base), wmax, before, tile_last);
        if (v.nskip == 0) {                                 // (a warm-up tile is dropped whole: nskip is 0 or the tile)
            f2 e[PER];
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int p = t * PER + k;
                const int l = lt[k] > before ? lt[k] : before;
                e[k] = f2{(p - l < W) ? 0.f : (float)((off + d[k]) / ratio), (float)((double)xd[k].x + (double)xd[k].y)};
            }
#pragma unroll
            for (int k = 0; k < PER; k += 2) {
                const int p = t * PER + k;
                if (p + 1 < v.nvalid) *reinterpret_cast<float4 *>(tr + base + p) = make_float4(e[k].x, e[k].y, e[k + 1].x, e[k + 1].y);
                else if (p < v.nvalid) tr[base + p] = e[k];
            }
        }
        r.S0 += total;
        if (RING) { rb += TILE; rb = rb >= NB_RING ? rb - NB_RING : rb; }
        if (tile_last > NB_NEVER) r.last = (long long)base + tile_last;
        __syncthreads();                                    // wsum / wmax reused by the next tile
    }
}

// ---- the mask form on DATAGRAM input in integers (round 6) ---------------------------------------------------------
// A 16- or 24-bit datagram sample is an integer multiple of 2^-8
// of the float the general kernel decodes (wire_format.hpp), so the magnitudes max(|I|, |Q|) are integers below 2^23 in
// that unit and the moving sum -- at most 32768 of them -- is an integer below 2^38: every fp64 sum of the general
// kernel (and of the reference: m_MagAveSum, noiseproc.cpp:143-147) is EXACT on such input, in any order, and equals the
// 64-bit integer sum here bit for bit.  What the integers buy: no decode to float, no float -> double conversions, a
// 32-bit subtract and add per sample instead of three half-rate fp64 operations, and -- the larger part -- the trigger
// test `mag * ratio > S` (noiseproc.cpp:155-158: one conversion, one fp64 multiply, one add, one compare per sample)
// is first asked once per THREAD in fp32 with a safety margin (largest of its eight magnitudes against the smallest of
// its eight sums): a thread without a candidate -- all but a few per launch -- skips the eight fp64 tests and the per-sample
// trigger positions.  A thread with a candidate runs the general kernel's exact fp64 test on the same numbers scaled by
// 2^8 (a power of two: the products and compares round identically), so the decisions are the general kernel's, sample
// for sample.  The host takes this kernel only while EVERY sample the blanker has seen since its last set-up came from
// datagrams (NbHost::integral) -- the state it inherits (sum, history) is then integral in that unit.
// Ring form only (the window's magnitudes in LDS, as integers, in eight planes); eight samples per thread.
constexpr int NB_IPER = NbTile<true, true>::PER, NB_ITILE = NbTile<true, true>::TILE;
static_assert(NB_IPER == 8, "the packing below is written for eight samples per thread");
static_assert(NB_T == 512, "eight waves: their sums and trigger positions cross in one row of eight lanes (three DPP steps)");
// tiles the integer kernel fetches ahead (1: 760 us, 2 / 3 / 4: 722 / 723 / 724 us for 256 x 2^21 24-bit samples).  TWO: the
// occupancy is LDS's -- two workgroups of 64 KB, four waves per SIMD -- so the registers of a second buffer are free, and
// one tile ahead left 48 bytes per lane in flight against an iteration of ~3 us
constexpr int NB_MASK_PREFETCH = 2;

// |a - b| of two unsigned words, b wave-uniform: one instruction (the compiler has no builtin for it)
__device__ __forceinline__ unsigned nb_absdiff(unsigned a, unsigned b)
{
    unsigned r;
    asm("v_sad_u32 %0, %1, %2, 0" : "=v"(r) : "v"(a), "s"(b));
    return r;
}
// a thread's eight integer magnitudes from its raw words.  24 bit: two samples = I0 Q0 I1 Q1, three bytes each, in three
// words.  With the four sign bits flipped (three XORs on the packed words) a component is offset binary, b = x + 2^23,
// and |x| = |b - 2^23| is one v_sad_u32; the two components that straddle words are picked out by one v_perm_b32 each
__device__ __forceinline__ void nb_imag24(const unsigned *pw, int (&mag)[NB_IPER])
{
#pragma unroll
    for (int p = 0; p < NB_IPER / 2; p++) {
        const unsigned d0 = pw[3 * p] ^ 0x00800000u, d1 = pw[3 * p + 1] ^ 0x00008000u, d2 = pw[3 * p + 2] ^ 0x80000080u;
        const unsigned bi0 = d0 & 0x00ffffffu;
        const unsigned bq0 = __builtin_amdgcn_perm(d1, d0, 0x0c050403u);      // bytes d0[3] d1[0] d1[1] 0
        const unsigned bi1 = __builtin_amdgcn_perm(d2, d1, 0x0c040302u);      // bytes d1[2] d1[3] d2[0] 0
        const unsigned bq1 = d2 >> 8;
        const unsigned ai0 = nb_absdiff(bi0, 0x00800000u), aq0 = nb_absdiff(bq0, 0x00800000u);
        const unsigned ai1 = nb_absdiff(bi1, 0x00800000u), aq1 = nb_absdiff(bq1, 0x00800000u);
        mag[2 * p] = (int)(ai0 > aq0 ? ai0 : aq0); mag[2 * p + 1] = (int)(ai1 > aq1 ? ai1 : aq1);
    }
}
__device__ __forceinline__ void nb_imag16(const unsigned *pw, int (&mag)[NB_IPER])
{
#pragma unroll
    for (int k = 0; k < NB_IPER; k++) {
        const int i = (int)(short)(pw[k] & 0xffffu), q = (int)(short)(pw[k] >> 16);
        const int ai = i < 0 ? -i : i, aq = q < 0 ? -q : q;
        mag[k] = (ai > aq ? ai : aq) << 8;
    }
}
// The magnitudes leaving the window, ring in planes.  A thread's eight new magnitudes go to the eight planes at
// ONE word index, consecutive lanes to consecutive words (eight conflict-free 4-byte stores at constant offsets);
// and the eight leaving the window, M1 samples back, come from the planes (k - M1) mod 8 at one of two word indices,
// again lane-consecutive -- where eight consecutive words per thread (32 bytes between lanes) kept the LDS unit busy
// 41 % of the kernel with three quarters of that in bank conflicts (tools/experiments/pmc_mask_int.sh)
struct NbFarPlanes {
    static constexpr int PLANE = NbIntMag::PLANE;
    int plane[NB_IPER], hi[NB_IPER], e0;                       // plane and word step of the k-th leaving sample (uniform, fixed for the launch)
    __device__ __forceinline__ explicit NbFarPlanes(int M1)
    {
        e0 = (int)((-(long)M1) >> 3);
#pragma unroll
        for (int k = 0; k < NB_IPER; k++) { plane[k] = (int)((k - (long)M1) & 7) * PLANE; hi[k] = (int)((k - (long)M1) >> 3) - e0; }
    }
    __device__ __forceinline__ void read(const int *ring, int rb, int (&far)[NB_IPER]) const
    {
        const int p0 = ((rb >> 3) + (int)threadIdx.x + e0) & (PLANE - 1), p1 = (p0 + 1) & (PLANE - 1);
#pragma unroll
        for (int k = 0; k < NB_IPER; k++) far[k] = ring[plane[k] + (hi[k] ? p1 : p0)];
    }
};
__device__ __forceinline__ long long nb_readlane64(long long v, int l)
{
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)v >> 32), l) << 32) |
                       (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)v, l));
}
// block sum (first barrier).  The waves' sums: lane q < 8 reads wave q's, a three-step prefix inside the first row, two
// broadcasts (instead of sixteen LDS reads per thread).  wu: this wave's number as a scalar
__device__ __forceinline__ void nb_block_sum(int run, long long S0, long long *wsum, int wu, long long &off, long long &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long incl = wave_incl_scan_add_i27(run);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    long long ws = lane < NB_WAVES ? wsum[lane] : 0;
    ws += (long long)wave_dpp64<0x111, 0xf>((unsigned long long)ws, 0ull);
    ws += (long long)wave_dpp64<0x112, 0xf>((unsigned long long)ws, 0ull);
    ws += (long long)wave_dpp64<0x114, 0xf>((unsigned long long)ws, 0ull);
    total = nb_readlane64(ws, NB_WAVES - 1);
    off = S0 + (incl - run) + (wu > 0 ? nb_readlane64(ws, wu - 1) : 0);
}
// block max of trigger positions (second barrier), the waves' maxima exchanged the same way.  scan: some thread of the
// wave has a candidate (a wave without one -- nearly every wave of nearly every tile -- has no trigger: no scan)
__device__ __forceinline__ void nb_block_max(int runmax, bool scan, int last_rel, int *wmax, int wu, int &before, int &tile_last)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inclm = scan ? wave_incl_scan_max(runmax) : NB_NEVER;
    if (lane == 63) wmax[w] = inclm;
    __syncthreads();
    int wm = lane < NB_WAVES ? wmax[lane] : NB_NEVER;
    wm = nb_dpp_max<0x111, 0xf>(wm); wm = nb_dpp_max<0x112, 0xf>(wm); wm = nb_dpp_max<0x114, 0xf>(wm);
    before = last_rel;
    if (wu > 0) { const int o = __builtin_amdgcn_readlane(wm, wu - 1); before = o > before ? o : before; }
    const int upto = wave_prev_lane(inclm);
    if (upto > before) before = upto;
    tile_last = __builtin_amdgcn_readlane(wm, NB_WAVES - 1);
}

// a thread's eight samples of the tile at b0 as raw words, fetched ahead: 12 words (24 bit) or 8 (16 bit); a thread's
// samples start at a multiple of eight, which divides 240 and 256: they lie in ONE datagram
template <int FMT> constexpr int NB_IWORDS = FMT == 1444 ? 12 : 8;
template <int FMT>
__device__ __forceinline__ void nb_int_fetch(const unsigned char *pk, long b0, long seg_b, unsigned (&pw)[NB_IWORDS<FMT>])
{
    const unsigned i0 = (unsigned)(b0 + (long)threadIdx.x * NB_IPER);
    if ((long)i0 + NB_IPER <= seg_b) {
        const unsigned *wp = FMT == 1444 ? wire_words24(pk, i0) : wire_words16(pk, i0);
#pragma unroll
        for (int k = 0; k < NB_IWORDS<FMT>; k++) pw[k] = wp[k];
    } else {
#pragma unroll
        for (int k = 0; k < NB_IWORDS<FMT>; k++) pw[k] = 0u;    // past the segment: zeros (never counted: r >= nvalid)
        // (a thread that straddles the end cannot exist: the segment ends on a multiple of eight -- nb_host.hpp)
    }
}

template <int FMT>                                           // 1444: 24-bit datagrams, 1028: 16-bit
__global__ __launch_bounds__(NB_T)
void noiseblank_mask_int_kernel(NbArgs a)
{
    constexpr int PF = NB_MASK_PREFETCH, PER = NB_IPER, TILE = NB_ITILE;
    __shared__ long long wsum[NB_WAVES];
    __shared__ int wmax[NB_WAVES];
    extern __shared__ __attribute__((aligned(16))) float nb_ring[];
    int *ring = reinterpret_cast<int *>(nb_ring);           // [NB_RING] integer magnitudes, units of 2^-8, in eight planes
    const NbSeg s(a);
    const int t = threadIdx.x;
    const NbChan C = a.chan[s.ch];
    const NbSrc<FMT> X(a, s.ch);
    unsigned *mrow = a.mask + (long)s.ch * a.mask_stride;
    NbRun<long long> r{(long long)llrint(C.sum * 256.0), -C.since_trig, 0};
    if (C.on) {
        const int M1 = C.mag_n + 1, W = C.width_n;
        const double ratio = C.ratio;
        const float ratio_hi = (float)ratio * 1.000004f;    // fp32 screen: errs on the side of calling the exact test
        const NbFarPlanes far_at(M1);
        nb_seg_start<NbIntMag, true>(s, X, M1, W, TILE, ring, wsum, r);
        unsigned pwq[PF][NB_IWORDS<FMT>];                   // the tiles in flight
        nb_int_fetch<FMT>(X.pk, r.first, s.b, pwq[0]);
#pragma unroll
        for (int q = 1; q < PF; q++)
            if (r.first + q * TILE < s.b) nb_int_fetch<FMT>(X.pk, r.first + q * TILE, s.b, pwq[q]);
        int rb = nb_ring_pos(r.first);                      // the tile's first sample, counted around the ring
        const int wu = __builtin_amdgcn_readfirstlane(t >> 6);     // this wave's number, as a scalar
        for (long base0 = r.first; base0 < s.b; base0 += PF * TILE) {
#pragma unroll
            for (int q = 0; q < PF; q++) {                  // the tile at `base`, its words in pwq[q]
                const long base = base0 + q * TILE;
                if (q > 0 && base >= s.b) continue;
                unsigned (&pw)[NB_IWORDS<FMT>] = pwq[q];
                int mag[PER], far[PER];
                if constexpr (FMT == 1444) nb_imag24(pw, mag); else nb_imag16(pw, mag);
                const NbSpan v(s, base, TILE);
                const bool live = t * PER < v.nvalid;       // (nvalid is a multiple of eight: a thread is in or out whole)
                far_at.read(ring, rb, far);
                int d[PER], run = 0, mmax = 0, dmin = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    run += mag[k] - far[k];                 // (a thread past the end of a call's last tile: unused, see below)
                    d[k] = run;                             // thread-local inclusive prefix (|.| < 2^26)
                    mmax = mag[k] > mmax ? mag[k] : mmax;
                    dmin = run < dmin ? run : dmin;
                }
                if (!live) run = 0;                         // (its fetch returned zeros: magnitudes 0 into the ring; nothing into the sums)
                int *dst = ring + (rb >> 3) + t;            // (rb / 8 + t < PLANE: tiles divide the ring)
#pragma unroll
                for (int k = 0; k < PER; k++) dst[k * NbIntMag::PLANE] = mag[k];
                if (base + PF * TILE < s.b) nb_int_fetch<FMT>(X.pk, base + PF * TILE, s.b, pw);    // (before the scans)
                long long off, total;
                nb_block_sum(run, r.S0, wsum, wu, off, total);
                // triggers: once per thread in fp32 (largest magnitude against the smallest sum, 4e-6 of margin against the
                // 6e-8 of the three roundings); only a thread with a candidate runs the exact tests
                int lt[PER], runmax = NB_NEVER;
                const bool candidate = live && (float)mmax * ratio_hi >= (float)(off + (long long)dmin);
                if (candidate) {
#pragma unroll
                    for (int k = 0; k < PER; k++) {
                        const bool trig = (double)mag[k] * ratio > (double)(off + (long long)d[k]);
                        if (trig) runmax = t * PER + k;
                        lt[k] = runmax;
                    }
                }
                int before, tile_last;
                nb_block_max(runmax, __any(candidate), nb_last_rel(r.last, base), wmax, wu, before, tile_last);
                unsigned nib = 0;
                if (live && candidate) nib = nb_blank_flags<PER>(lt, before, W, TILE);
                else if (live) {
                    // no trigger among this thread's samples: sample p is blanked while p - before < W
                    const int nb = W + before - t * PER;    // how many of the eight, from the first
                    nib = nb <= 0 ? 0u : (nb >= PER ? 0xffu : (1u << nb) - 1u);
                }
                nb_put_mask_word<PER, true>(mrow, base, nib, v.nskip == 0 && live);
                r.S0 += total;
                rb += TILE; rb = rb >= NB_RING ? rb - NB_RING : rb;
                if (tile_last > NB_NEVER) r.last = (long long)base + tile_last;
                // (no barrier here: wsum is next written behind this tile's second barrier, which every wave reaches only after
                // its reads of wsum; wmax is next written behind the NEXT tile's first barrier, reached only after the reads of wmax)
            }
        }
    }
    nb_finish<true>(a, s, C, X, (double)r.S0 * (1.0 / 256.0), r.last);
}

// ---- launch ----------------------------------------------------------------------------------------------------
// (the ring forms' static + dynamic LDS are above 64 KB: the attribute once per device and kernel -- the static of
// CSDR_MAX_LDS_ONCE belongs to this template's instantiation)
template <void (*KERNEL)(NbArgs)>
static hipError_t nb_launch(const NbArgs &a, int lds_bytes, hipStream_t stream)
{
    if (lds_bytes) {
        hipError_t e = CSDR_MAX_LDS_ONCE(KERNEL, lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(KERNEL, dim3(a.channels * a.nseg), dim3(NB_T), lds_bytes, stream, a);
    return hipGetLastError();
}
hipError_t noiseblank_launch(const NbArgs &a, hipStream_t stream)
{
    constexpr int RING_BYTES = NB_RING * 4;
    switch (a.form) {
    case NB_SAMPLES:      return nb_launch<noiseblank_kernel<false, false>>(a, 0, stream);
    case NB_SAMPLES_RING: return nb_launch<noiseblank_kernel<false, true>>(a, RING_BYTES, stream);
    case NB_MASK:         return nb_launch<noiseblank_kernel<true, false>>(a, 0, stream);
    case NB_MASK_RING:    return nb_launch<noiseblank_kernel<true, true>>(a, RING_BYTES, stream);
    case NB_MASK_INT24:   return nb_launch<noiseblank_mask_int_kernel<1444>>(a, RING_BYTES, stream);
    case NB_MASK_INT16:   return nb_launch<noiseblank_mask_int_kernel<1028>>(a, RING_BYTES, stream);
    }
    return hipErrorInvalidValue;
}
hipError_t noiseblank_trace_launch(const NbArgs &a, hipStream_t stream)
{
    switch (a.form) {
    case NB_SAMPLES:      return nb_launch<noiseblank_trace_kernel<false>>(a, 0, stream);
    case NB_SAMPLES_RING: return nb_launch<noiseblank_trace_kernel<true>>(a, NB_RING * 4, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace csdr
