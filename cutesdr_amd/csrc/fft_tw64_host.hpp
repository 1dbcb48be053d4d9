// fft_tw64_host.hpp -- the fp64 twiddle tables of the batch transforms (K3q), built on the host.  Plain C++: the table
// builder is also compiled into a stand-alone sanitizer program (tests/test_fft_plain64_host.py).
//
// Every entry is the long double value rounded once to double.  The angle is reduced in integers to the first octant
// (0 ... pi/4, where cosl / sinl lose nothing to argument reduction) and the other seven octants are that value with
// swapped parts and signs: no recurrence, and W^(period/8), W^(period/4) ... are exact where they are exact.
#pragma once
#include <cmath>
#include <vector>

namespace csdr {

// cs = (cos, sin)(2 pi m / period), period a power of two >= 8
inline void tw64_entry(long m, long period, double *cs)
{
    const long double two_pi = 6.283185307179586476925286766559L;
    m &= period - 1;
    const long oct = period / 8, q = m / oct, r = m % oct;
    const long j = (q & 1) ? oct - r : r;                    // odd octants count down from their upper end
    const long double a = (long double)j * two_pi / (long double)period;
    const double c = (double)cosl(a), s = (double)sinl(a);
    switch (q) {
    case 0: cs[0] = c; cs[1] = s; break;
    case 1: cs[0] = s; cs[1] = c; break;
    case 2: cs[0] = -s; cs[1] = c; break;
    case 3: cs[0] = -c; cs[1] = s; break;
    case 4: cs[0] = -c; cs[1] = -s; break;
    case 5: cs[0] = -s; cs[1] = -c; break;
    case 6: cs[0] = s; cs[1] = -c; break;
    default: cs[0] = c; cs[1] = -s; break;
    }
    cs[0] += 0.0; cs[1] += 0.0;                              // (no negative zero)
}
// count entries W_period^m, m = 0 ... count - 1, appended to out
inline void tw64_fill(long period, long count, std::vector<double> &out)
{
    const size_t at = out.size();
    out.resize(at + 2 * (size_t)count);
    for (long m = 0; m < count; m++) tw64_entry(m, period, &out[at + 2 * (size_t)m]);
}
// the table of an n-point transform as the kernels read it (PlainBatch64Args::tw); single: one workgroup per frame
inline void fft64_tables(int n, bool single, std::vector<double> &out)
{
    out.clear();
    if (single) tw64_fill(n, n, out);
    else { tw64_fill(256, 256, out); tw64_fill(n, 256, out); }
}

}  // namespace csdr
