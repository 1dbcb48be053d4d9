// pc_scan.hpp -- the workgroup scan of the post-chain kernels (postchain_kernels.hip, K4 in DESIGN.md) and its maps.
// Every linear recurrence of K4 is solved the same way: a thread reduces its consecutive samples to ONE map of the
// running state (state entering its chunk -> state leaving it), Wg::scan composes the maps of all earlier threads, and
// the thread applies that to the state the tile started from.  Wg::scan is written once, over this interface of a map:
//   identity()        the map that changes nothing
//   after(earlier)    this o earlier: `earlier` is applied first
//   dpp<CTRL, ROW>()  the map held by the lane a DPP step reads from, identity() where the step has no source lane
//   lane63()          the map held by the wave's last lane
//   put(x) / get(x)   N doubles of a row of the workgroup's exchange area
#pragma once
#include <hip/hip_runtime.h>
#include "wave_dpp.hpp"

namespace csdr {

constexpr int PT = 1024;                 // K4's tile length (samples); here because a thread's share of a scan, Wg<NW>::LC, is cut from it
constexpr int PC_MAX_WAVES = 4;          // waves of the largest workgroup that scans

// A wave's scan steps run on the DPP network (wave_dpp.hpp) instead of __shfl_up: a tile runs some ninety such steps
// one after the other on a single wave per SIMD.  pc_dpp<CTRL, ROW_MASK>(v, ident): v of the source lane, `ident` where
// the step has none.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double pc_dpp(double v, double ident)
{
    return __longlong_as_double((long long)wave_dpp64<CTRL, ROW_MASK>((unsigned long long)__double_as_longlong(v),
                                                                       (unsigned long long)__double_as_longlong(ident)));
}

// s -> a s + b
struct Aff1 {
    static constexpr int N = 2;
    double a, b;
    static __device__ __forceinline__ Aff1 identity() { return {1.0, 0.0}; }
    __device__ __forceinline__ Aff1 after(const Aff1 &e) const { return {a * e.a, a * e.b + b}; }
    template <int C, int R> __device__ __forceinline__ Aff1 dpp() const { return {pc_dpp<C, R>(a, 1.0), pc_dpp<C, R>(b, 0.0)}; }
    __device__ __forceinline__ Aff1 lane63() const { return {__shfl(a, 63), __shfl(b, 63)}; }
    __device__ __forceinline__ void put(double *x) const { x[0] = a; x[1] = b; }
    static __device__ __forceinline__ Aff1 get(const double *x) { return {x[0], x[1]}; }
    __device__ __forceinline__ double operator()(double s) const { return a * s + b; }
};

// s -> M s + v on pairs, M = [[m[0], m[1]], [m[2], m[3]]]
struct Aff2 {
    static constexpr int N = 6;
    double m[4], v[2];
    static __device__ __forceinline__ Aff2 identity() { return {{1.0, 0.0, 0.0, 1.0}, {0.0, 0.0}}; }
    __device__ __forceinline__ Aff2 after(const Aff2 &e) const
    {
        return {{m[0] * e.m[0] + m[1] * e.m[2], m[0] * e.m[1] + m[1] * e.m[3], m[2] * e.m[0] + m[3] * e.m[2], m[2] * e.m[1] + m[3] * e.m[3]},
                {m[0] * e.v[0] + m[1] * e.v[1] + v[0], m[2] * e.v[0] + m[3] * e.v[1] + v[1]}};
    }
    template <int C, int R> __device__ __forceinline__ Aff2 dpp() const
    {
        return {{pc_dpp<C, R>(m[0], 1.0), pc_dpp<C, R>(m[1], 0.0), pc_dpp<C, R>(m[2], 0.0), pc_dpp<C, R>(m[3], 1.0)},
                {pc_dpp<C, R>(v[0], 0.0), pc_dpp<C, R>(v[1], 0.0)}};
    }
    __device__ __forceinline__ Aff2 lane63() const { return {{__shfl(m[0], 63), __shfl(m[1], 63), __shfl(m[2], 63), __shfl(m[3], 63)}, {__shfl(v[0], 63), __shfl(v[1], 63)}}; }
    __device__ __forceinline__ void put(double *x) const { x[0] = m[0]; x[1] = m[1]; x[2] = m[2]; x[3] = m[3]; x[4] = v[0]; x[5] = v[1]; }
    static __device__ __forceinline__ Aff2 get(const double *x) { return {{x[0], x[1], x[2], x[3]}, {x[4], x[5]}}; }
    __device__ __forceinline__ void operator()(double s0, double s1, double &r0, double &r1) const      // (r0, r1) = M (s0, s1) + v
    { r0 = m[0] * s0 + m[1] * s1 + v[0]; r1 = m[2] * s0 + m[3] * s1 + v[1]; }
};

// x -> max(a x + b, c): closed under composition
struct AffMax {
    static constexpr int N = 3;
    double a, b, c;
    static __device__ __forceinline__ AffMax identity() { return {1.0, 0.0, -1.0e300}; }
    __device__ __forceinline__ AffMax after(const AffMax &e) const { return {a * e.a, a * e.b + b, fmax(a * e.c + b, c)}; }
    template <int C, int R> __device__ __forceinline__ AffMax dpp() const { return {pc_dpp<C, R>(a, 1.0), pc_dpp<C, R>(b, 0.0), pc_dpp<C, R>(c, -1.0e300)}; }
    __device__ __forceinline__ AffMax lane63() const { return {__shfl(a, 63), __shfl(b, 63), __shfl(c, 63)}; }
    __device__ __forceinline__ void put(double *x) const { x[0] = a; x[1] = b; x[2] = c; }
    static __device__ __forceinline__ AffMax get(const double *x) { return {x[0], x[1], x[2]}; }
    __device__ __forceinline__ double operator()(double x) const { return fmax(a * x + b, c); }
};

// a running maximum
struct Max {
    static constexpr int N = 1;
    double v;
    static __device__ __forceinline__ Max identity() { return {-1.0e300}; }
    __device__ __forceinline__ Max after(const Max &e) const { return {fmax(v, e.v)}; }
    template <int C, int R> __device__ __forceinline__ Max dpp() const { return {pc_dpp<C, R>(v, -1.0e300)}; }
    __device__ __forceinline__ Max lane63() const { return {__shfl(v, 63)}; }
    __device__ __forceinline__ void put(double *x) const { x[0] = v; }
    static __device__ __forceinline__ Max get(const double *x) { return {x[0]}; }
};

// Two independent maps in lockstep: one wave per SIMD pays every instruction's latency, and the two dependency chains
// fill each other's gaps; one exchange, one barrier.  In the exchange row p comes first, q behind it.
template <class P, class Q>
struct Both {
    static constexpr int N = P::N + Q::N;
    P p;
    Q q;
    static __device__ __forceinline__ Both identity() { return {P::identity(), Q::identity()}; }
    __device__ __forceinline__ Both after(const Both &e) const { return {p.after(e.p), q.after(e.q)}; }
    template <int C, int R> __device__ __forceinline__ Both dpp() const { return {p.template dpp<C, R>(), q.template dpp<C, R>()}; }
    __device__ __forceinline__ Both lane63() const { return {p.lane63(), q.lane63()}; }
    __device__ __forceinline__ void put(double *x) const { p.put(x); q.put(x + P::N); }
    static __device__ __forceinline__ Both get(const double *x) { return {P::get(x), Q::get(x + P::N)}; }
};

// what a workgroup's scans and broadcasts exchange through LDS (Wg<NW> holds a pointer to it)
struct alignas(16) PcSync {               // (16: the arrays behind it are read and written in 16-byte pieces)
    double xch[2][PC_MAX_WAVES][8];      // per-wave totals of a workgroup scan; two banks used in turn, so that a scan
                                         // needs ONE workgroup barrier (the next scan's writes go to the other bank)
    double bc[4];                        // broadcast slot (thread 0 -> workgroup)
    int flag;                            // workgroup-wide "any"
};

// workgroup context: thread id, lane, wave; barrier that orders LDS traffic of the whole workgroup.
// NW waves (1 or 4); thread t owns the LC = PT / (64 NW) consecutive samples [LC t, LC t + LC) of a tile in every scan.
template <int NW>
struct Wg {
    static_assert(NW <= PC_MAX_WAVES, "PcSync::xch has a row per wave");
    static constexpr int NT = 64 * NW, LC = PT / NT;
    int t, lane, w;
    PcSync *S;
    mutable int bank = 0;                // exchange bank of the next workgroup scan (uniform)
#ifdef PC_CENSUS
    // diagnostic builds (postchain.h): the force word and what it asks of this tile, the tile's record so far, the rounds of
    // the last AGC scan that converged -- uniform over the workgroup
    mutable unsigned cen_force = 0, cen_rec = 0;
    mutable int cen_limit = 0, cen_rounds = 0;
    mutable bool cen_fail_overlap = false;
    __device__ __forceinline__ void cen_or(unsigned bits) const { cen_rec |= (unsigned)__builtin_amdgcn_readfirstlane((int)bits); }   // (scalar registers)
#endif
    __device__ __forceinline__ double (*xbank() const)[8] { double (*b)[8] = S->xch[bank]; bank ^= 1; return b; }
    // this thread's chunk of a tile of n samples: its first sample, and how many of its LC lie inside the tile
    __device__ __forceinline__ int base() const { return LC * t; }
    __device__ __forceinline__ int count(int n) const { const int c = n - LC * t; return c < 0 ? 0 : (c > LC ? LC : c); }
    __device__ __forceinline__ void sync() const
    {
        if constexpr (NW == 1) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            __syncthreads();
        }
    }
    // true on every thread if pred holds on any thread
    __device__ __forceinline__ bool any(bool pred) const
    {
        if constexpr (NW == 1) return __any(pred);
        if (t == 0) S->flag = 0;
        __syncthreads();
        if (__any(pred) && lane == 0) S->flag = 1;
        __syncthreads();
        const bool r = S->flag != 0;
        __syncthreads();
        return r;
    }
    // value held by thread 0 -> every thread
    __device__ __forceinline__ double bcast0(double v, int slot) const
    {
        if constexpr (NW == 1) return __shfl(v, 0);
        if (t == 0) S->bc[slot] = v;
        __syncthreads();
        const double r = S->bc[slot];
        __syncthreads();
        return r;
    }
    // Thread t's map is applied after those of the threads < t.  In: m = this thread's chunk map.  Out: m = the
    // composition of all EARLIER threads (exclusive), total = the composition of all threads, on every thread.
    // Six DPP steps and a wave_shr within the wave; across waves one exchange of the waves' totals and one barrier.
    template <class M>
    __device__ __forceinline__ void scan(M &m, M &total) const
    {
        static_assert(M::N <= 8, "a row of PcSync::xch holds eight doubles");
#define PC_STEP(C_, R_) m = m.after(m.template dpp<C_, R_>());
        WAVE_SCAN_STEPS(PC_STEP)
#undef PC_STEP
        M ex = m.template dpp<WAVE_SHR1, 0xf>();
        if constexpr (NW == 1) {
            total = m.lane63();
        } else {
            double (*xc)[8] = xbank();
            if (lane == 63) m.put(xc[w]);
            __syncthreads();
            M prev = M::identity();                  // the waves in front of this one
            total = M::identity();
#pragma unroll
            for (int q = 0; q < NW; q++) {
                const M x = M::get(xc[q]);
                if (q < w) prev = x.after(prev);
                total = x.after(total);
            }
            ex = ex.after(prev);
        }
        m = ex;
    }
    // exclusive prefix sum over the threads
    __device__ __forceinline__ double scan_sum_excl(double x) const
    {
        double incl = x;
#define PC_STEP(C_, R_) incl += pc_dpp<C_, R_>(incl, 0.0);
        WAVE_SCAN_STEPS(PC_STEP)
#undef PC_STEP
        double ex = incl - x;
        if constexpr (NW > 1) {
            double (*xc)[8] = xbank();
            if (lane == 63) xc[w][0] = incl;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NW; q++) if (q < w) ex += xc[q][0];
        }
        return ex;
    }
    // value of thread t-1 (thread 0 gets `first`)
    __device__ __forceinline__ float prev_thread(float v, float first) const
    {
        float p = __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), WAVE_SHR1, 0xf, 0xf, false));
        if constexpr (NW > 1) {
            double (*xc)[8] = xbank();
            if (lane == 63) xc[w][6] = (double)v;
            __syncthreads();
            if (lane == 0 && w > 0) p = (float)xc[w - 1][6];
        }
        return t == 0 ? first : p;
    }
};

}  // namespace csdr
