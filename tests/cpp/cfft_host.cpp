// A host that uses CFft the way CFastFIR::SetupParameters does (dsp/fastfir.cpp: design in the time domain, FwdFFT, use
// the response), compiled against the drop-in headers with plain g++, with and without -DCSDR_CFFT_FP64.
//   cfft_host <in.bin> <out.bin>        in.bin: one frame of interleaved doubles, 512 ... 65536 points
#include <cstdio>
#include <vector>
#include "dsp/fft.h"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: cfft_host in.bin out.bin\n"); return 2; }
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::vector<TYPECPX> x;
    TYPECPX s;
    while (std::fread(&s, sizeof(s), 1, fi) == 1) x.push_back(s);
    std::fclose(fi);
    CFft fft;
    fft.SetFFTParams((qint32)x.size(), false, 0.0, 48000.0);
    fft.FwdFFT(x.data());
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    const bool ok = std::fwrite(x.data(), sizeof(TYPECPX), x.size(), fo) == x.size();
    return (std::fclose(fo) == 0 && ok) ? 0 : 1;
}
