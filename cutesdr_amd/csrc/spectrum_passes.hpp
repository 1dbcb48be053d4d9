// spectrum_passes.hpp -- the three-pass decimation-in-time transform of N = 2048 ... 16384 points as N/32 threads x 32
// points: the 16384-point display spectrum and the plain transforms of every size (spectrum_kernels.hip: Passes32,
// fft_plain_kernel) and the batch scope's FFT view (scope_kernels.hip).  The display spectrum of 2048 ... 8192 points has
// transforms of sixteen points per thread of its own (spectrum_kernels.hip: Wide16).  A unit that includes this file
// defines CSDR_FMA_BFLY (and CSDR_PLAIN_CONST_FMA) before fft_core.hpp, as spectrum_kernels.hip does.
#pragma once
#include <type_traits>
#include "fft_core.hpp"

namespace csdr {

#define K3_SB() __builtin_amdgcn_sched_barrier(0)

template <int LOG2N>
struct SpecCfg {
    static constexpr int N = 1 << LOG2N, T = N / 32, R0 = N / 1024, G = 32 / R0;
    static constexpr int LDS_DATA = N + 2 * (N / 32);
    static constexpr int LDS_BYTES = (LDS_DATA + 1024) * 8;
    // the G columns (of the 1024 x R0 input matrix) a thread owns in pass A, in PAIRS that the workgroup's threads
    // take side by side: column pair t + T k, k < G/2.  A wave's load of one element pair is then 64 x 16 contiguous
    // bytes (with G consecutive columns per thread -- 64 bytes at N = 4096 -- every 128-byte line was consumed by four
    // separate load instructions; measured: no difference in time, the line sat in L2 either way).
    static __device__ __forceinline__ int col(int t, int e) { return 2 * (t + T * (e >> 1)) + (e & 1); }
};

// forward (positive exponent) transform of the block held as x[e*R0+n1] <-> sample 1024*n1+Cfg::col(t,e);
// on return x[k2] is spectrum bin  (t>>5) + R0*((t&31) + 32*k2).
// Three decimation-in-time passes with FMA-form butterflies (fft_core.hpp, as in the round-2 overlap-save kernel):
// the bit-reversed input order a DIT network wants costs nothing -- pass A's samples sit in registers, passes B and C
// read their points from LDS in any order -- and its outputs come out in natural order.  The 1024-point
// sub-transform k0 lives in ONE half-wave (threads 32 k0 .. 32 k0 + 31), so the exchange between passes B and C needs
// no workgroup barrier, only the wave's own program order.
template <int LOG2N>
__device__ __forceinline__ void fft_fwd_passes(v2f (&x)[32], v2f *lds, const v2f *tw2, const v2f *w1)
{
    using Cfg = SpecCfg<LOG2N>;
    constexpr int R0 = Cfg::R0, G = Cfg::G;
    const int t = threadIdx.x;
    // ---- pass A: radix-R0 over the rows n1 of column G t + e, outer twiddle W_N^{(G t + e) k0}
#pragma unroll
    for (int e = 0; e < G; e++) {
        v2f y[R0];
        static_for<0, R0>([&](auto N1) { y[bitrev<R0>(N1.value)] = x[e * R0 + N1.value]; });
        dft_dit<R0, +1>(y);
        v2f pw[R0];
        twiddle_powers<R0>(opaque(w1[e]), pw);
        static_for<1, R0>([&](auto K0) { y[K0.value] = cmul(y[K0.value], pw[K0.value]); });
#pragma unroll
        for (int i = 0; i < R0; i++) x[e * R0 + i] = y[i];
    }
    __syncthreads();                       // the previous transform's pass C has read its rows
    static_for<0, R0>([&](auto K0) {
        constexpr int k0 = K0.value;
#pragma unroll
        for (int e = 0; e < G; e++) lds[lds_pad(1024 * k0 + Cfg::col(t, e))] = x[e * R0 + k0];   // (a column pair shares a 32-group: adjacent)
    });
    __syncthreads();
    // ---- pass B: radix-32 over the 32 points of column sn of sub-transform sb, twiddle W_1024^{sn k1}, in place.
    // Cut into groups of four points like the passes of the overlap-save kernel (fft_core.hpp: head4 / tail): the
    // points are fetched in the order the first stages need them, three groups ahead of the butterflies; a tail
    // group's results are stored while the next group's butterflies issue; sched_barrier pins that order.
    const int sb = t >> 5, sn = t & 31;
    v2f *const col = lds + lds_pad(1024 * sb) + sn;          // point n1 at col[34 * n1]
    const v2f *const twc = tw2 + sn;                         // twiddle k1 at twc[32 * k1]
    {
        auto fetch = [&](auto Gg) {
            static_for<0, 4>([&](auto Q) {
                constexpr int p = 4 * Gg.value + Q.value;
                x[p] = lds_ld8(col + 34 * bitrev<32>(p));
            });
        };
        static_for<0, 3>(fetch);
        K3_SB();
        static_for<0, 8>([&](auto Gg) {
            if constexpr (Gg.value + 3 < 8) fetch(std::integral_constant<int, Gg.value + 3>{});
            dit_head4<Gg.value, 32, +1>(x);
            if constexpr ((Gg.value & 1) == 1) K3_SB();
        });
        dit_single<8, 32, +1>(x);
        K3_SB();
        v2f tw[2][4];
        static_for<1, 4>([&](auto P) { tw[0][P.value] = lds_ld8(twc + 32 * (8 * P.value)); });
        K3_SB();
        static_for<0, 9>([&](auto Ii) {
            constexpr int i = Ii.value;                      // tail group i finishes k1 = i, i+8, i+16, i+24
            if constexpr (i < 7)
                static_for<0, 4>([&](auto P) { tw[(i + 1) & 1][P.value] = lds_ld8(twc + 32 * (i + 1 + 8 * P.value)); });
            if constexpr (i < 8) {
                dit_tail<i, 32, +1>(x);
                static_for<0, 4>([&](auto P) {
                    constexpr int k1 = i + 8 * P.value;
                    if constexpr (k1 != 0) x[k1] = cmul(x[k1], tw[i & 1][P.value]);
                });
            }
            if constexpr (i > 0)
                static_for<0, 4>([&](auto P) {
                    constexpr int k1 = (i - 1) + 8 * P.value;
                    lds_st8(col + 34 * k1, x[k1]);
                });
            K3_SB();
        });
    }
    // B -> C stays inside the half-wave that owns sub-transform sb
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- pass C: radix-32 over the 32 consecutive points of row t, read as 16-byte pairs: rows q, q+4, q+8, q+12 of
    // pairs hold the inputs of head groups bitrev3(2q) and bitrev3(2q+1)
    {
        const v2f *const rowp = lds + 34 * t;
        static_for<0, 4>([&](auto Q) {
            static_for<0, 4>([&](auto P) {
                constexpr int j = Q.value + 4 * P.value;
                const v4f v = *reinterpret_cast<const v4f *>(rowp + 2 * j);
                x[bitrev<32>(2 * j)] = v2f{v.x, v.y};
                x[bitrev<32>(2 * j + 1)] = v2f{v.z, v.w};
            });
        });
        K3_SB();
        static_for<0, 4>([&](auto Q) {
            dit_head4<bitrev<8>(2 * Q.value), 32, +1>(x);
            dit_head4<bitrev<8>(2 * Q.value + 1), 32, +1>(x);
            K3_SB();
        });
        dit_single<8, 32, +1>(x);
        static_for<0, 8>([&](auto Ii) { dit_tail<Ii.value, 32, +1>(x); });
    }
}

}  // namespace csdr
