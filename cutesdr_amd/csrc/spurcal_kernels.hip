// spurcal_kernels.hip -- K13: the batch NCO-spur calibration.  C independent copies of CSdrInterface::NcoSpurCalibrate
// (reference interface/sdrinterface.cpp:829-848, called at :886-887 behind the in-place blanker of :884) with the
// bookkeeping of spurcal_host.hpp's spurcal_put evaluated on the device, two launches per put for every receiver.
//
// The recurrence y <- (1 - a) y + a x (:837, :839) is linear in its start value, so a stretch of m samples that begins
// at y0 ends at (1 - a)^m y0 + (what the stretch gives from 0), and stretches combine with powers of (1 - a).
// Stretches are laid out from the END of the samples a receiver uses (spurcal_put(..).samples): the run, the pass and
// the tile a sample belongs to depend on its distance to that end, every stretch in front of the end is whole, and the
// short one is the first in time -- it starts from 0 and simply has fewer steps.  So every power is that of a whole run,
// wave, pass or tile: constants, spurcal_pow on the host (Pow), and in the finish one exp per level and receiver.
//   partial kernel, grid (tile, receiver): a workgroup reads its receiver's record and leaves when the receiver is not
// calibrating or its tile lies in front of the used samples.  A thread steps the reference's recurrence from 0 over a
// run of 16 samples (the operations of :837-839 in their order, no contraction), folds its runs of the tile's four
// passes, the wave folds its lanes by shuffles, the workgroup its waves through LDS; one partial pair per tile.
//   finish kernel, one wave per receiver: folds the tiles' partials, applies (1 - a)^samples to the offsets, and writes
// offsets, count and active.  Nothing but the finish writes a record, so every workgroup of the partial kernel has read
// the arriving one.
//   loads: 16 divides both datagram sizes and a datagram put uses whole datagrams, so a run starts on a word inside one
// datagram (wide loads at 4-byte alignment); behind a blanker that is on, the run delayed by delay_n + 1 is taken pair by
// pair and zeroed under its 16 mask bits; runs that reach in front of the put or lie off the 16-sample grid go sample by
// sample.  Every path delivers the same fp32 values, and the steps are the same operations in the same order.
// The fold order depends on positions only (no atomics), and the sample source is a template input of the load, so the
// same samples give the same doubles whichever form delivered them.  Offsets inside a receiver's block are 32 bit.
#include "spurcal_kernels.h"
#include <type_traits>

// every product and sum below is rounded on its own, as the reference's statements are: no fused multiply-add, in any
// form of the load, so that the forms agree to the bit
#pragma clang fp contract(off)

namespace csdr {
namespace spur {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

struct Pow {
    double lane[6];                      // (1 - a)^(kRun << l): what 2^l runs leave of the value in front of them
    double wave;                         // ^(kRun * 64)
    double pass;                         // ^kPass
    double tile;                         // ^kTile
};

// p * y + x as the reference's two statements have it: both products and the sum rounded (no fused multiply-add)
__device__ __forceinline__ double fold(double p, double y, double x) { return p * y + x; }
__device__ __forceinline__ double step(double y, float x) { return kKeep * y + kAlpha * (double)x; }

// a receiver's samples as they arrived.  FMT: 0 fp32 rows, 1028 / 1444 datagrams
template <int FMT>
struct Raw {
    const unsigned char *chan;
    const f2 *row;
    __device__ __forceinline__ Raw(const Src &a, int ch)
        : chan(FMT ? a.wire.pk + (long)ch * a.wire.chan_stride : nullptr),
          row(FMT ? nullptr : reinterpret_cast<const f2 *>(a.in) + (long)ch * a.in_stride) {}
    __device__ __forceinline__ f2 at(int s) const
    {
        if constexpr (FMT == 0) return row[s];
        else { const wf2 v = wire_sample(chan, FMT, s); return f2{v.x, v.y}; }
    }
    // samples s0 .. s0 + 15; datagrams: s0 a multiple of 16, so the run lies in one datagram and starts on a word
    __device__ __forceinline__ void run(int s0, f2 v[kRun]) const
    {
        if constexpr (FMT == 0) {
#pragma unroll
            for (int i = 0; i < kRun; i++) v[i] = row[s0 + i];
        } else {
            constexpr int W = FMT == 1444 ? 3 : 2;           // words per sample pair
            const unsigned *w = FMT == 1444 ? wire_words24(chan, (unsigned)s0) : wire_words16(chan, (unsigned)s0);
            unsigned r[W * kRun / 2];
#pragma unroll
            for (int i = 0; i < W * kRun / 2; i++) r[i] = w[i];
#pragma unroll
            for (int k = 0; k < kRun / 2; k++) {
                const wf4 d = wire_pair_decode(wf4{__uint_as_float(r[W * k]), __uint_as_float(r[W * k + 1]),
                                                   W == 3 ? __uint_as_float(r[W * k + W - 1]) : 0.f, 0.f}, FMT);
                v[2 * k] = f2{d.x, d.y}; v[2 * k + 1] = f2{d.z, d.w};
            }
        }
    }
    // samples j0 .. j0 + 15 from any j0 >= 0 (the blanker's delayed run): datagrams pair by pair from the even index on
    // -- a pair never straddles a datagram -- with the odd ends one by one
    template <bool ODD>
    __device__ __forceinline__ void delayed(int j0, f2 v[kRun]) const
    {
        if constexpr (FMT == 0) {
#pragma unroll
            for (int i = 0; i < kRun; i++) v[i] = row[j0 + i];
        } else {
            if constexpr (ODD) { v[0] = at(j0); v[kRun - 1] = at(j0 + kRun - 1); }
#pragma unroll
            for (int i = ODD; i + 1 < kRun; i += 2) {
                const wf4 d = wire_pair_decode(wire_pair_fetch(chan, FMT, j0 + i), FMT);
                v[i] = f2{d.x, d.y}; v[i + 1] = f2{d.z, d.w};
            }
        }
    }
};

// what the blanker handed over (display_stream_kernels.h:13-17, stream_sample<true>'s rule before its DC correction)
template <int FMT>
struct Blanked {
    Raw<FMT> raw;
    const unsigned *mask;
    const f2 *hist;
    int on, d1;
    __device__ __forceinline__ Blanked(const Src &a, int ch)
        : raw(a, ch), mask(a.nb_mask + (long)ch * a.nb_mask_stride),
          hist(reinterpret_cast<const f2 *>(a.nb_hist) + (long)ch * NB_HIST + NB_HIST),
          on(a.nb_state[ch].on), d1(a.nb_state[ch].delay_n + 1) {}
    __device__ __forceinline__ f2 at(int s) const
    {
        if ((mask[s >> 5] >> (s & 31)) & 1u) return f2{0.f, 0.f};
        const int j = s - d1;
        return j < 0 ? hist[j] : raw.at(j);                  // j >= -NB_MAX_WIDTH / 2 - 1
    }
};

// the run [e - kRun, e) of a receiver's used samples, e > 0, stepped from 0; the first run in time may be short
template <int FMT, bool BLK, class S>
__device__ __forceinline__ void run_from_zero(const S &src, int e, double &yi, double &yq)
{
    yi = 0.0; yq = 0.0;
    const int s0 = e - kRun;
    bool whole = s0 >= 0 && (FMT == 0 || (s0 & (kRun - 1)) == 0);
    if constexpr (BLK) whole = whole && !src.on;
    if (whole) {
        f2 v[kRun];
        if constexpr (BLK) src.raw.run(s0, v); else src.run(s0, v);
#pragma unroll
        for (int i = 0; i < kRun; i++) { yi = step(yi, v[i].x); yq = step(yq, v[i].y); }
        return;
    }
    if constexpr (BLK) {                                     // blanker on, the run on a mask half-word, all behind the call's start
        const int j0 = s0 - src.d1;
        if (src.on && s0 >= 0 && (s0 & (kRun - 1)) == 0 && j0 >= 0) {
            f2 v[kRun];
            if (j0 & 1) src.raw.template delayed<true>(j0, v); else src.raw.template delayed<false>(j0, v);
            const unsigned m = src.mask[s0 >> 5] >> (s0 & 31);
#pragma unroll
            for (int i = 0; i < kRun; i++) {
                const bool z = (m >> i) & 1u;
                yi = step(yi, z ? 0.f : v[i].x); yq = step(yq, z ? 0.f : v[i].y);
            }
            return;
        }
    }
    for (int s = s0 < 0 ? 0 : s0; s < e; s++) {
        f2 v;
        if constexpr (BLK) v = src.on ? src.at(s) : src.raw.at(s); else v = src.at(s);
        yi = step(yi, v.x); yq = step(yq, v.y);
    }
}

template <int FMT, bool BLK>
__global__ __launch_bounds__(kThreads)
void spurcal_partial_kernel(Src a, Pow pw, const Rec *rec, double *part, int ntiles)
{
    __shared__ double red[2][kThreads / 64];
    const int ch = blockIdx.y, kt = blockIdx.x, t = threadIdx.x;
    const Rec r = rec[ch];
    if (!r.active) return;
    const int hi = spurcal_put(r.count, r.active, a.n, a.call_len).samples - kt * kTile;     // the tile is [hi - kTile, hi)
    if (hi <= 0) return;
    typename std::conditional<BLK, Blanked<FMT>, Raw<FMT>>::type src(a, ch);
    double yi = 0.0, yq = 0.0;
    for (int ps = kPasses - 1; ps >= 0; ps--) {              // forward in time
        const int e = hi - ps * kPass - (kThreads - 1 - t) * kRun;
        double ri = 0.0, rq = 0.0;
        if (e > 0) run_from_zero<FMT, BLK>(src, e, ri, rq);
        yi = fold(pw.pass, yi, ri); yq = fold(pw.pass, yq, rq);
    }
#pragma unroll
    for (int l = 0; l < 6; l++) {                            // lane t in front of lane t + (1 << l); lane 0 ends whole
        const double ni = __shfl_down(yi, 1 << l), nq = __shfl_down(yq, 1 << l);
        yi = fold(pw.lane[l], yi, ni); yq = fold(pw.lane[l], yq, nq);
    }
    if ((t & 63) == 0) { red[0][t >> 6] = yi; red[1][t >> 6] = yq; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kThreads / 64; w++) { yi = fold(pw.wave, yi, red[0][w]); yq = fold(pw.wave, yq, red[1][w]); }
        double *o = part + 2 * ((long)ch * ntiles + kt);
        o[0] = yi; o[1] = yq;
    }
}

__global__ __launch_bounds__(64)
void spurcal_finish_kernel(int n, int call_len, double tile_pow, Rec *rec, double *dc, const double *part, int ntiles)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    const Rec r = rec[ch];
    if (!r.active) return;                                   // not a bit of an inactive receiver changes
    const Put p = spurcal_put(r.count, r.active, n, call_len);
    if (p.samples > 0) {
        const int nt = (p.samples + kTile - 1) / kTile;      // tile 0 ends the used samples, tile nt - 1 begins them
        const int m = (nt + 63) / 64;                        // tiles per lane, lane 0 the last in time
        const double *pt = part + 2 * (long)ch * ntiles;
        double yi = 0.0, yq = 0.0;
        for (int k = min(nt, (lane + 1) * m) - 1; k >= lane * m; k--) {
            yi = fold(tile_pow, yi, pt[2 * k]); yq = fold(tile_pow, yq, pt[2 * k + 1]);
        }
        for (int l = 0; l < 6; l++) {                        // lane + (1 << l) lies in front of lane
            const double w = spurcal_pow((long long)m * kTile << l);
            const double fi = __shfl_down(yi, 1 << l), fq = __shfl_down(yq, 1 << l);
            yi = fold(w, fi, yi); yq = fold(w, fq, yq);
        }
        if (lane == 0) {
            const double w = spurcal_pow(p.samples);
            dc[2 * ch] = fold(w, dc[2 * ch], yi);
            dc[2 * ch + 1] = fold(w, dc[2 * ch + 1], yq);
        }
    }
    if (lane == 0) rec[ch] = Rec{p.count, p.active};
}

__global__ __launch_bounds__(64)
void spurcal_command_kernel(double *dc, Rec *rec, int lo, int hi, int cmd, double vi, double vq)
{
    const int c = lo + (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= hi) return;
    spurcal_command(cmd, vi, vq, dc + 2 * c, rec + c);
}

template <int FMT>
hipError_t partial_launch(const Src &a, const Pow &pw, int channels, const Rec *rec, double *part, int ntiles, hipStream_t stream)
{
    const dim3 grid(ntiles, channels);
    if (a.nb_mask) hipLaunchKernelGGL((spurcal_partial_kernel<FMT, true>), grid, dim3(kThreads), 0, stream, a, pw, rec, part, ntiles);
    else hipLaunchKernelGGL((spurcal_partial_kernel<FMT, false>), grid, dim3(kThreads), 0, stream, a, pw, rec, part, ntiles);
    return hipGetLastError();
}

}  // namespace

hipError_t spurcal_put_launch(const Src &a, int channels, double *dc, Rec *rec, double *part, hipStream_t stream)
{
    if (a.n <= 0 || channels <= 0) return hipSuccess;
    static const Pow pw = [] {
        Pow p;
        for (int l = 0; l < 6; l++) p.lane[l] = spurcal_pow((long long)kRun << l);
        p.wave = spurcal_pow(kRun * 64); p.pass = spurcal_pow(kPass); p.tile = spurcal_pow(kTile);
        return p;
    }();
    const int ntiles = spurcal_tiles(a.n);
    hipError_t e;
    if (!a.wire.pk) e = partial_launch<0>(a, pw, channels, rec, part, ntiles, stream);
    else if (a.wire.pkt_len == 1444) e = partial_launch<1444>(a, pw, channels, rec, part, ntiles, stream);
    else e = partial_launch<1028>(a, pw, channels, rec, part, ntiles, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spurcal_finish_kernel, dim3(channels), dim3(64), 0, stream, a.n, a.call_len, pw.tile, rec, dc, part, ntiles);
    return hipGetLastError();
}

hipError_t spurcal_command_launch(double *dc, Rec *rec, int lo, int hi, int cmd, double vi, double vq, hipStream_t stream)
{
    if (hi <= lo) return hipSuccess;
    hipLaunchKernelGGL(spurcal_command_kernel, dim3((hi - lo + 63) / 64), dim3(64), 0, stream, dc, rec, lo, hi, cmd, vi, vq);
    return hipGetLastError();
}

}  // namespace spur
}  // namespace csdr
