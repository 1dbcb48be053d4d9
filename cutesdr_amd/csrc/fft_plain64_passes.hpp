// fft_plain64_passes.hpp -- fp64 butterflies and Stockham passes of the batch transforms (K3q).  The fp64 siblings of
// fft_core.hpp's dft_dit and fft_batch_plain_kernels.hip's sk_load / sk_store, written apart from them so that the fp32
// instantiations stay what they are.  __host__ __device__ throughout: the same functions run in a host program that
// walks a workgroup's threads (tests/cpp/fft_plain64_emu.hip, held to the device's rule by tests/test_fft_plain64_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "fft_core.hpp"                                      // static_for, bitrev

namespace csdr {

typedef double v2d __attribute__((ext_vector_type(2)));

// cos(2 pi k / 16), correctly rounded
constexpr double kCos16d[16] = {
    1.0, 0.92387953251128675613, 0.70710678118654752440, 0.38268343236508977173,
    0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128675613,
    -1.0, -0.92387953251128675613, -0.70710678118654752440, -0.38268343236508977173,
    0.0, 0.38268343236508977173, 0.70710678118654752440, 0.92387953251128675613};

// a * w: two roundings per part
__host__ __device__ __forceinline__ v2d cmul64(v2d a, v2d w)
{
    return v2d{__builtin_fma(a.x, w.x, -(a.y * w.y)), __builtin_fma(a.x, w.y, a.y * w.x)};
}

// DIT butterfly: a' = a + b W_16^K, b' = a - b W_16^K, K in [0, 8).  Each output part is two chained FMAs on the inputs
// (two roundings), neither is derived from the other.
template <int K>
__host__ __device__ __forceinline__ void bfly64(v2d &xa, v2d &xb)
{
    static_assert(K >= 0 && K < 8, "bfly64");
    const v2d a = xa, b = xb;
    if constexpr (K == 0) {
        xa = a + b; xb = a - b;
    } else if constexpr (K == 4) {
        xa = v2d{a.x - b.y, a.y + b.x}; xb = v2d{a.x + b.y, a.y - b.x};
    } else {
        constexpr double c = kCos16d[K], s = kCos16d[(K + 12) & 15];
        xa = v2d{__builtin_fma(-b.y, s, __builtin_fma(b.x, c, a.x)), __builtin_fma(b.y, c, __builtin_fma(b.x, s, a.y))};
        xb = v2d{__builtin_fma(b.y, s, __builtin_fma(-b.x, c, a.x)), __builtin_fma(-b.y, c, __builtin_fma(-b.x, s, a.y))};
    }
}
// Decimation-in-time radix-R DFT, positive exponent, R <= 16: input y[k] in x[bitrev(k)], natural order out
template <int LEN, int R>
__host__ __device__ __forceinline__ void dit64_stage(v2d (&x)[R])
{
    constexpr int H = LEN / 2;
    static_for<0, R / LEN>([&](auto B) {
        static_for<0, H>([&](auto I) {
            constexpr int a = B.value * LEN + I.value, b = a + H;
            bfly64<I.value *(16 / LEN)>(x[a], x[b]);
        });
    });
    if constexpr (LEN < R) dit64_stage<LEN * 2, R>(x);
}
template <int R>
__host__ __device__ __forceinline__ void dft_dit64(v2d (&x)[R])
{
    static_assert(R <= 16, "dft_dit64");
    if constexpr (R > 1) dit64_stage<2, R>(x);
}

// One autosort pass of radix R over an L-point transform whose earlier passes have the product NS (the scheme of
// fft_batch_plain_kernels.hip): butterfly j < L / R takes points j + r L / R, turns point r by W_(NS R)^((j mod NS) r),
// and its R results go to (j - j mod NS) R + j mod NS + r NS.  A thread loads and transforms ALL its butterflies
// (sk_load64), the workgroup meets, then it stores them (sk_store64).  A transform is worked on by TPF threads (tl of
// them); tw is the table W_(L TWS)^m.
template <int R, int L, int TPF> struct SkRegs64 {
    static constexpr int ITERS = (L / R + TPF - 1) / TPF;
    v2d y[ITERS][R];
};
template <int R, int NS, int L, int TPF, int TWS, class Ld>
__host__ __device__ __forceinline__ void sk_load64(int tl, const v2d *tw, SkRegs64<R, L, TPF> &g, Ld ld)
{
    static_for<0, SkRegs64<R, L, TPF>::ITERS>([&](auto It) {
        const int j = tl + TPF * It.value;
        if ((L / R) % TPF == 0 || j < L / R) {
            const int k = j & (NS - 1);
            v2d (&y)[R] = g.y[It.value];
            static_for<0, R>([&](auto Rr) {
                constexpr int r = Rr.value;
                v2d v = ld(j + r * (L / R));
                if constexpr (r > 0 && NS > 1) v = cmul64(v, tw[TWS * (L / (NS * R)) * k * r]);
                y[bitrev<R>(r)] = v;
            });
            dft_dit64<R>(y);
        }
    });
}
template <int R, int NS, int L, int TPF, class St>
__host__ __device__ __forceinline__ void sk_store64(int tl, const SkRegs64<R, L, TPF> &g, St st)
{
    static_for<0, SkRegs64<R, L, TPF>::ITERS>([&](auto It) {
        const int j = tl + TPF * It.value;
        if ((L / R) % TPF == 0 || j < L / R) {
            const int k = j & (NS - 1), base = (j - k) * R + k;
            static_for<0, R>([&](auto Rr) { st(base + Rr.value * NS, g.y[It.value][Rr.value]); });
        }
    });
}

// ---- 512 ... 4096 points: one LDS image per frame, three passes RA RB RC, 256 threads
template <int LOG2N>
struct Small64Cfg {
    static constexpr int N = 1 << LOG2N, T = 256;
    static constexpr int TPF = LOG2N <= 10 ? 64 : N / 16, FPW = T / TPF;              // 4 4 2 1 frames per workgroup
    static constexpr int RA = LOG2N == 9 ? 8 : 16, RB = RA, RC = N / (RA * RB);       // 8 8 8 / 16 16 4 / 16 16 8 / 16 16 16
    // One pad element per RA: pass A's stores (butterfly j at element RA j + r) walk the image at RA + 1 elements, 36 or
    // 68 dwords, per lane.  A 16-byte store is served eight neighbouring lanes at a time over 32 banks: 36 j and 68 j
    // mod 32 = 4 j, eight different 4-bank quarters.  Pass B's stores are runs of RA neighbouring elements.
    static constexpr int PS = LOG2N == 9 ? 3 : 4;
    static constexpr int LF = N + (N >> PS);
    static constexpr int LDS_BYTES = FPW * LF * 16;
    static __host__ __device__ __forceinline__ int pad(int i) { return i + (i >> PS); }
};

// ---- the four-step sizes: N = N1 x N2, both transforms in two passes by 16 threads, 16 transforms side by side
template <int LOG2N>
struct Four64Cfg {
    static constexpr int N = 1 << LOG2N;
    static constexpr int N1 = LOG2N == 13 ? 64 : (LOG2N == 14 ? 128 : 256), N2 = N / N1;   // 64x128 128x128 256x128 256x256
    static constexpr int W = 16, TPF = 16, T = 256;
    static constexpr int ra(int l) { return l >= 128 ? 16 : 8; }
    static constexpr int lds_bytes(int l, int tw) { return (17 * l + tw) * 16; }
    static constexpr int COLS_LDS = lds_bytes(N1, 512), ROWS_LDS = lds_bytes(N2, 256);
};

}  // namespace csdr
