// The fp64 twiddle table builder (cutesdr_amd/csrc/fft_tw64_host.hpp) as a stand-alone program, for an
// AddressSanitizer / UBSan build on the CPU (tests/test_fft_plain64_host.py): every size's table, as the library builds
// it, written to the file named on the command line as raw doubles, size after size.
#include "fft_tw64_host.hpp"
#include <cstdio>

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "wb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<double> tw;
    for (int n = 512; n <= 65536; n *= 2) {
        csdr::fft64_tables(n, n < 8192, tw);
        if (fwrite(tw.data(), sizeof(double), tw.size(), f) != tw.size()) { perror("fwrite"); return 1; }
        // entries past a period wrap, and an odd entry of the finest table reaches every octant's interior
        double cs[2], back[2];
        csdr::tw64_entry(n + 3, n, cs);
        csdr::tw64_entry(3, n, back);
        if (cs[0] != back[0] || cs[1] != back[1]) { fprintf(stderr, "wrap at %d\n", n); return 1; }
    }
    return fclose(f) == 0 ? 0 : 1;
}
