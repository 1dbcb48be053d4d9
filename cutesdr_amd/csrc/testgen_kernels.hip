// testgen_kernels.hip -- the batch signal generator's device half (K9 in DESIGN.md): CTestBench::CreateGeneratorSamples
// (reference gui/testbench.cpp:352-447 complex, :454-517 real) for every receiver of a batch in one launch.
//
// The host (testgen_host.hpp) has already decided everything sequential: per receiver a short table of phase segments
// (first sample, phase, phase increment, increment step, all in 128-bit turns), the pulse pattern as counters, the
// noise key and sample counter.  A lane owns one 16-byte store -- two complex or four real samples -- evaluates
//     P(t) = P0 + t * D0 + D2 * t (t - 1) / 2      (mod one turn: the wrap-around is the reduction)
// at its first sample and steps P += D, D += D2 to the next, taking the next segment's words where one starts.  The
// top bits of P give the quadrant and an argument within +-pi/4, whose sine and cosine are two short fp64 polynomials
// (truncation 7e-12); amp * cos + noise is rounded to fp32 once.  Pure write stream, no LDS, no atomics.
//
// Noise: Marsaglia's polar method as the reference's, the 31-bit draws from a counter-based generator
// (include/cutesdr_mi.h states it completely); the rejection loop is the one data-dependent loop, at most 32 rounds.
#include <hip/hip_runtime.h>
#include "testgen_kernels.h"

namespace csdr {

using tg::ChanParam;
using tg::u128;

constexpr int TG_THREADS = 256;
constexpr int TG_ATTEMPTS = 32;
static_assert(tg::kMaxSeg == 8, "testgen_kernel loads the eight segment starts as two uint4");

__device__ __forceinline__ u128 tg_load128(const uint64_t (*w)[2], unsigned s) { return ((u128)w[s][1] << 64) | w[s][0]; }

// cos and sin of 2 pi * (ph / 2^64)
__device__ __forceinline__ void tg_sincos(uint64_t ph, double &c, double &s)
{
    const uint64_t t = ph + (1ull << 61);                                     // quadrant q, offset within +-1/8 turn
    const unsigned q = (unsigned)(t >> 62);
    const int r = (int)((unsigned)(t >> 30) ^ 0x80000000u);                   // [-2^31, 2^31) in units of 2^-34 turn
    const double y = (double)r * (6.283185307179586476925286766559 / 17179869184.0);
    const double z = y * y;
    double sp = -1.0 / 39916800.0;
    sp = fma(sp, z, 1.0 / 362880.0);
    sp = fma(sp, z, -1.0 / 5040.0);
    sp = fma(sp, z, 1.0 / 120.0);
    sp = fma(sp, z, -1.0 / 6.0);
    sp = fma(sp * z, y, y);
    double cp = 1.0 / 479001600.0;
    cp = fma(cp, z, -1.0 / 3628800.0);
    cp = fma(cp, z, 1.0 / 40320.0);
    cp = fma(cp, z, -1.0 / 720.0);
    cp = fma(cp, z, 1.0 / 24.0);
    cp = fma(cp, z, -0.5);
    cp = fma(cp, z, 1.0);
    c = (q & 1u) ? sp : cp;              // q0: (cos, sin)  q1: (-sin, cos)  q2: (-cos, -sin)  q3: (sin, -cos)
    s = (q & 1u) ? cp : sp;
    if (q == 1u || q == 2u) c = -c;
    if (q >= 2u) s = -s;
}

__device__ __forceinline__ uint64_t tg_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the two Gaussian terms of sample `count` (before the amplitude); false when every attempt was rejected
__device__ __forceinline__ bool tg_noise(uint64_t key, uint64_t count, double &g1, double &g2)
{
#pragma clang fp contract(off)
    for (int a = 0; a < TG_ATTEMPTS; a++) {
        const uint64_t h = tg_mix64(key + tg::kGolden * (count * (uint64_t)TG_ATTEMPTS + (uint64_t)a));
        const double u1 = 1.0 - 2.0 * (double)(unsigned)(h >> 33) / 2147483647.0;
        const double u2 = 1.0 - 2.0 * (double)(unsigned)((h >> 2) & 0x7FFFFFFFull) / 2147483647.0;
        const double r = u1 * u1 + u2 * u2;
        if (r >= 1.0 || r == 0.0) continue;
        const double rad = sqrt(-2.0 * log(r) / r);
        g1 = u1 * rad; g2 = u2 * rad;
        return true;
    }
    return false;
}

template <int REAL>                      // 0: complex rows, two samples per lane; 1: mono rows, four
__global__ __launch_bounds__(TG_THREADS) void testgen_kernel(TestGenArgs a)
{
    constexpr int SPL = REAL ? 4 : 2;
    const int ch = blockIdx.y;
    const ChanParam *p = a.par + ch;
    const unsigned nseg = p->nseg;
    if (nseg == 0) return;               // generator off (or nothing left for this launch): the row is not touched
    const unsigned j_lo = p->j_lo, j_hi = p->j_hi;
    const unsigned jb = blockIdx.x * (unsigned)(TG_THREADS * SPL);
    if (jb >= j_hi || jb + TG_THREADS * SPL <= j_lo) return;
    const unsigned j0 = jb + threadIdx.x * SPL;
    const unsigned jf = j0 > j_lo ? j0 : j_lo;           // the lane's first sample of this launch
    const unsigned je = j0 + SPL < j_hi ? j0 + SPL : j_hi;
    if (jf >= je) return;

    // The phase at jf.  Nearly every workgroup lies inside one segment: its anchor (phase and increment at the
    // workgroup's first sample) is then uniform -- scalar arithmetic -- and a lane adds its offset of < 1024 samples.
    const unsigned jb0 = jb > j_lo ? jb : j_lo;
    unsigned st[tg::kMaxSeg + 1];        // the segment starts, all at once (one uniform load, no chain of branches)
    {
        const uint4 lo = *reinterpret_cast<const uint4 *>(&p->seg_start[0]), hi = *reinterpret_cast<const uint4 *>(&p->seg_start[4]);
        st[0] = lo.x; st[1] = lo.y; st[2] = lo.z; st[3] = lo.w; st[4] = hi.x; st[5] = hi.y; st[6] = hi.z; st[7] = hi.w;
        st[tg::kMaxSeg] = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 1; k < tg::kMaxSeg; k++) st[k] = (unsigned)k < nseg ? st[k] : 0xFFFFFFFFu;
    }
    unsigned sb = 0, nextb = 0xFFFFFFFFu;
#pragma unroll
    for (int k = tg::kMaxSeg - 1; k >= 1; k--) {
        sb += st[k] <= jb0 ? 1u : 0u;
        nextb = st[k] > jb0 ? st[k] : nextb;             // the smallest start behind jb0 (starts ascend)
    }
    unsigned s = sb, next = 0xFFFFFFFFu;
    u128 D2, D, P;
    if (nextb >= jb + TG_THREADS * SPL || nextb >= j_hi) {
        const uint64_t tb = jb0 - p->seg_start[sb];
        const unsigned tl = jf - jb0;
        D2 = tg_load128(p->seg_d2, sb);
        const u128 D0 = tg_load128(p->seg_d, sb);
        const u128 Pb = tg_load128(p->seg_p, sb) + D0 * (u128)tb + D2 * (u128)(tb * (tb - 1) / 2);  // tb < 2^32: fits
        const u128 Db = D0 + D2 * (u128)tb;
        P = Pb + Db * (u128)tl + D2 * (u128)((tl * (tl - 1u)) >> 1);                                // tl < 1024
        D = Db + D2 * (u128)tl;
    } else {                             // a segment starts inside this workgroup: every lane finds its own
#pragma unroll
        for (int k = tg::kMaxSeg - 1; k >= 1; k--) {
            s += ((unsigned)k > sb && st[k] <= jf) ? 1u : 0u;
            next = st[k] > jf ? st[k] : next;
        }
        const uint64_t t = jf - p->seg_start[s];
        D2 = tg_load128(p->seg_d2, s);
        const u128 D0 = tg_load128(p->seg_d, s);
        P = tg_load128(p->seg_p, s) + D0 * (u128)t + D2 * (u128)(t * (t - 1) / 2);
        D = D0 + D2 * (u128)t;
    }

    // pulse timer index of jf: (jf + 1) additions from pos0
    const bool gated = p->gate_on != 0;
    const uint64_t K = p->period, W = p->width;
    uint64_t pos = 0;
    if (gated) {
        const uint64_t m = (uint64_t)jf + 1, w1 = p->wrap1;
        if (m < w1) pos = p->pos0 + m;
        else {
            const unsigned k32 = K > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)K;       // m - w1 < 2^32 - 1: no second wrap then
            pos = (unsigned)(m - w1) % k32;
        }
    }
    const bool noisy = p->noise_on != 0;
    const uint64_t key = p->noise_key, count0 = p->count0;
    const double amp_on = REAL ? 3.0 * p->amp : p->amp, namp = p->noise_amp;

    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SPL; k++) {
        const unsigned j = j0 + k;
        if (j < jf || j >= je) continue;
        double c, sn;
        tg_sincos((uint64_t)(P >> 64), c, sn);
        const double amp = (!gated || pos < W) ? amp_on : 0.0;
        double re = amp * c, im = amp * sn;
        if (noisy) {
            double g1, g2;
            if (tg_noise(key, count0 + j, g1, g2)) { re += namp * g1; im += namp * g2; }
        }
        if (REAL) v[k] = (float)re;
        else { v[2 * k] = (float)re; v[2 * k + 1] = (float)im; }
        // to the next sample
        if (j + 1 == next) {
            s++;
            P = tg_load128(p->seg_p, s); D = tg_load128(p->seg_d, s); D2 = tg_load128(p->seg_d2, s);
            next = s + 1 < nseg ? p->seg_start[s + 1] : 0xFFFFFFFFu;
        } else { P += D; D += D2; }
        pos = pos + 1 >= K ? 0 : pos + 1;
    }
    float *row = a.out + (long)ch * a.stride * (REAL ? 1 : 2);
    if (jf == j0 && je == j0 + SPL) {
        *reinterpret_cast<float4 *>(row + (long)j0 * (REAL ? 1 : 2)) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < SPL; k++) {
            const unsigned j = j0 + k;
            if (j < jf || j >= je) continue;
            if (REAL) row[j] = v[k];
            else { row[2 * (long)j] = v[2 * k]; row[2 * (long)j + 1] = v[2 * k + 1]; }
        }
    }
}

hipError_t testgen_launch(const TestGenArgs &a, int real, hipStream_t s)
{
    const unsigned per = TG_THREADS * (real ? 4 : 2);
    const dim3 grid((a.n + per - 1) / per, a.channels);
    if (real) hipLaunchKernelGGL(testgen_kernel<1>, grid, dim3(TG_THREADS), 0, s, a);
    else hipLaunchKernelGGL(testgen_kernel<0>, grid, dim3(TG_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace csdr
