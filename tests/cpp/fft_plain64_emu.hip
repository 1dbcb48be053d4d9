// The K3q kernels (cutesdr_amd/csrc/fft_batch_plain64_kernels.hip) walked on the host: the pass functions of
// fft_plain64_passes.hpp are __host__ __device__, and this program runs one frame through them the way a workgroup does
// -- every thread's part of a phase in a loop, a barrier where the loop ends -- with the tables of fft_tw64_host.hpp.
// The index arithmetic, the butterflies and the rounding order are the device's (tests/test_fft_plain64_host.py holds
// the result to the rule of fft_plain64_ref.py without a GPU).  Host code only: build with --cuda-host-only.
//   fft_plain64_emu <in.bin> <out.bin> <sign>      in.bin: one frame of interleaved doubles, 512 ... 65536 points
#include "fft_plain64_passes.hpp"
#include "fft_tw64_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace csdr;

template <int LOG2N>
static void emu_small(const v2d *in, v2d *out, const v2d *tw)
{
    using Cfg = Small64Cfg<LOG2N>;
    constexpr int N = Cfg::N, TPF = Cfg::TPF, RA = Cfg::RA, RB = Cfg::RB, RC = Cfg::RC;
    std::vector<v2d> my(Cfg::LF);
    auto gld = [&](int i) { return in[i]; };
    auto gst = [&](int i, v2d v) { out[i] = v; };
    auto lld = [&](int i) { return my[Cfg::pad(i)]; };
    auto lst = [&](int i, v2d v) { my[Cfg::pad(i)] = v; };
    for (int tl = 0; tl < TPF; tl++) {
        SkRegs64<RA, N, TPF> g;
        sk_load64<RA, 1, N, TPF, 1>(tl, tw, g, gld);
        sk_store64<RA, 1, N, TPF>(tl, g, lst);
    }
    {
        std::vector<SkRegs64<RB, N, TPF>> g(TPF);
        for (int tl = 0; tl < TPF; tl++) sk_load64<RB, RA, N, TPF, 1>(tl, tw, g[tl], lld);
        for (int tl = 0; tl < TPF; tl++) sk_store64<RB, RA, N, TPF>(tl, g[tl], lst);
    }
    for (int tl = 0; tl < TPF; tl++) {
        SkRegs64<RC, N, TPF> g;
        sk_load64<RC, RA * RB, N, TPF, 1>(tl, tw, g, lld);
        sk_store64<RC, RA * RB, N, TPF>(tl, g, gst);
    }
}

template <int LOG2N>
static void emu_four(const v2d *in0, v2d *out0, const v2d *tw)
{
    using Cfg = Four64Cfg<LOG2N>;
    constexpr int N = Cfg::N, N1 = Cfg::N1, N2 = Cfg::N2, TPF = Cfg::TPF, T = Cfg::T, W = Cfg::W;
    std::vector<v2d> work(N);
    {   // launch 1
        constexpr int L = N1, TWS = 256 / L, RA = Cfg::ra(L), RB = L / RA;
        for (int bx = 0; bx < N2 / W; bx++) {
            std::vector<v2d> lds(17 * L);
            for (int phase = 0; phase < 2; phase++)
                for (int t = 0; t < T; t++) {
                    const int c = t & 15, tl = t >> 4, n2 = W * bx + c;
                    const v2d *in = in0 + n2;
                    v2d *wk = work.data() + n2;
                    auto gld = [&](int i) { return in[(long)i * N2]; };
                    auto lld = [&](int i) { return lds[17 * i + c]; };
                    auto lst = [&](int i, v2d v) { lds[17 * i + c] = v; };
                    auto gst = [&](int k1, v2d v) {
                        const int m = n2 * k1;
                        const v2d w = cmul64(tw[(m >> 8) * (65536 / N)], tw[256 + (m & 255)]);
                        wk[(long)k1 * N2] = cmul64(v, w);
                    };
                    if (phase == 0) {
                        SkRegs64<RA, L, TPF> g;
                        sk_load64<RA, 1, L, TPF, TWS>(tl, tw, g, gld);
                        sk_store64<RA, 1, L, TPF>(tl, g, lst);
                    } else {
                        SkRegs64<RB, L, TPF> g;
                        sk_load64<RB, RA, L, TPF, TWS>(tl, tw, g, lld);
                        sk_store64<RB, RA, L, TPF>(tl, g, gst);
                    }
                }
        }
    }
    {   // launch 2
        constexpr int L = N2, TWS = 256 / L, RA = Cfg::ra(L), RB = L / RA;
        for (int bx = 0; bx < N1 / W; bx++) {
            std::vector<v2d> lds(17 * L);
            const int k1_0 = W * bx;
            const v2d *wk = work.data() + (long)k1_0 * L;
            for (int i = 0; i < W * L; i++) lds[17 * (i % L) + i / L] = wk[i];
            std::vector<SkRegs64<RA, L, TPF>> ga(T);
            for (int phase = 0; phase < 3; phase++)
                for (int t = 0; t < T; t++) {
                    const int c = t & 15, tl = t >> 4;
                    v2d *out = out0 + k1_0 + c;
                    auto lld = [&](int i) { return lds[17 * i + c]; };
                    auto lst = [&](int i, v2d v) { lds[17 * i + c] = v; };
                    auto gst = [&](int k2, v2d v) { out[(long)k2 * N1] = v; };
                    if (phase == 0) sk_load64<RA, 1, L, TPF, TWS>(tl, tw, ga[t], lld);
                    else if (phase == 1) sk_store64<RA, 1, L, TPF>(tl, ga[t], lst);
                    else {
                        SkRegs64<RB, L, TPF> g;
                        sk_load64<RB, RA, L, TPF, TWS>(tl, tw, g, lld);
                        sk_store64<RB, RA, L, TPF>(tl, g, gst);
                    }
                }
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s in.bin out.bin sign\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    std::vector<v2d> x;
    double s[2];
    while (fread(s, sizeof(s), 1, fi) == 1) x.push_back(v2d{s[0], s[1]});
    fclose(fi);
    const int n = (int)x.size();
    int l2 = 0;
    while ((1 << l2) < n) l2++;
    if ((1 << l2) != n || l2 < 9 || l2 > 16) { fprintf(stderr, "%d points\n", n); return 2; }
    const double cj = atoi(argv[3]) > 0 ? 1.0 : -1.0;            // RevFFT: conjugate in, conjugate out, as the kernels do
    for (auto &v : x) v.y *= cj;
    std::vector<v2d> y(n);
    std::vector<double> tw;
    fft64_tables(n, l2 <= 12, tw);
    const v2d *t = reinterpret_cast<const v2d *>(tw.data());
    switch (l2) {
    case 9: emu_small<9>(x.data(), y.data(), t); break;
    case 10: emu_small<10>(x.data(), y.data(), t); break;
    case 11: emu_small<11>(x.data(), y.data(), t); break;
    case 12: emu_small<12>(x.data(), y.data(), t); break;
    case 13: emu_four<13>(x.data(), y.data(), t); break;
    case 14: emu_four<14>(x.data(), y.data(), t); break;
    case 15: emu_four<15>(x.data(), y.data(), t); break;
    default: emu_four<16>(x.data(), y.data(), t); break;
    }
    for (auto &v : y) v.y *= cj;
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    const bool ok = fwrite(y.data(), sizeof(v2d), y.size(), fo) == y.size();
    return (fclose(fo) == 0 && ok) ? 0 : 1;
}
