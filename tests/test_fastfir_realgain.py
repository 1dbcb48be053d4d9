"""CPU tests of the real-gain form of the overlap-save response (no GPU): every response CFastFIR::SetupParameters can
make is H[k] = P[k] s^k with P real and s = +j (forward transform sign +1, centre tap N/4), checked on the oracle's
coefficients and on the library's host design; and host builds of the butterflies the 16384-point kernel uses for it
(fft_core.hpp: dit_head4_gain, dit_tail_middle) against a direct DFT."""
import ctypes as C
import numpy as np
import pytest

S = 1j                      # H[k] = P[k] * S**k  (host_math.hpp: fastfir_gain)
FILTERS = [(-5000, 5000, 0, 48000.0), (100, 2800, 0, 48000.0), (-2800, -100, 0, 48000.0), (-250, 250, 700, 48000.0),
           (-15000, 15000, 0, 48000.0), (300, 2700, -800, 48000.0), (-5000, 5000, 0, 62500.0)]


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_fastfir_gains.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_void_p] * 2
    lib.csdr__host_fastfir2_bin_of.argtypes = [C.c_int] * 4
    lib.csdr__host_fastfir2_gain_bin_of.argtypes = [C.c_int] * 4
    lib.csdr__host_dit_head4_gain.argtypes = [C.c_int] + [C.c_void_p] * 3
    lib.csdr__host_dit_head4_gain.restype = None
    lib.csdr__host_dft_middle.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n", [4096, 8192, 16384])
@pytest.mark.parametrize("flt", FILTERS)
def test_response_is_real_gains_times_a_quarter_block_shift(L, oracle, n, flt):
    ff = oracle.CFastFIR(n)
    assert ff.SetupParameters(*flt) == 1
    Ho = np.asarray(ff.coef(), dtype=np.complex128)
    H = np.zeros(n, dtype=np.complex128)
    P = np.zeros(n, dtype=np.float64)
    assert L.csdr__host_fastfir_gains(n, flt[0], flt[1], flt[2], flt[3], vp(H), vp(P)) == 0
    rot = np.conj(S) ** (np.arange(n) % 4)
    for name, h in (("oracle", Ho), ("library", H)):
        top = np.abs(h).max()
        imag = np.abs((h * rot).imag).max()
        print("%s n=%d %s: max|Im(H conj(s)^k)| / max|H| = %.3g" % (name, n, flt, imag / top))
        assert imag <= 1e-9 * top
    err = np.abs(P - (Ho * rot).real).max()
    print("max|P - Re(H conj(s)^k)| / max|H| = %.3g" % (err / np.abs(Ho).max()))
    assert err <= 1e-12 * np.abs(Ho).max()


def test_gain_order_follows_the_pipelined_kernels_bin_order(L):
    """float4 i of thread t holds the gains of H's float4 2i and 2i+1 (both halves), and the order is a permutation"""
    seen = np.zeros(16384, dtype=bool)
    for t in range(512):
        for i in range(8):
            for c in range(4):
                k = L.csdr__host_fastfir2_gain_bin_of(14, t, i, c)
                assert k == L.csdr__host_fastfir2_bin_of(14, t, 2 * i + (c >> 1), c & 1)
                assert k == (t >> 5) + 16 * ((t & 31) + 32 * (i + 8 * (c >> 1) + 16 * (c & 1)))
                seen[k] = True
    assert seen.all()


def dft(x, sign):
    n = len(x)
    k = np.arange(n)
    return np.exp(sign * 2j * np.pi * np.outer(k, k) / n) @ x


def bitrev(v, bits):
    return int("{:0{w}b}".format(v, w=bits)[::-1], 2)


@pytest.mark.parametrize("sign", [+1, -1])
def test_scaled_head_group_is_a_four_point_dft_of_the_scaled_points(L, sign):
    rng = np.random.default_rng(11)
    for _ in range(8):
        x = (rng.standard_normal(4) + 1j * rng.standard_normal(4)).astype(np.complex64)     # network order: x[bitrev(n)]
        g = rng.standard_normal(4).astype(np.float32)
        out = np.zeros(4, dtype=np.complex64)
        L.csdr__host_dit_head4_gain(sign, vp(x), vp(g), vp(out))
        nat = np.array([x[bitrev(n, 2)].astype(np.complex128) * float(g[bitrev(n, 2)]) for n in range(4)])
        want = dft(nat, sign)
        # fp32 butterflies of O(1) numbers, two stages: a few ulp of the largest magnitude
        assert np.abs(out - want).max() <= 8 * np.finfo(np.float32).eps * np.abs(want).max()


@pytest.mark.parametrize("r", [16, 32])
@pytest.mark.parametrize("sign", [+1, -1])
def test_middle_rows_tail_gives_rows_quarter_to_three_quarters(L, r, sign):
    rng = np.random.default_rng(r + sign)
    for _ in range(8):
        x = (rng.standard_normal(r) + 1j * rng.standard_normal(r)).astype(np.complex64)
        out = np.zeros(r // 2, dtype=np.complex64)
        assert L.csdr__host_dft_middle(r, sign, vp(x), vp(out)) == 0
        want = dft(x.astype(np.complex128), sign)
        # log2(r) fp32 stages: error grows like eps * log2(r) * max|X|
        assert np.abs(out - want[r // 4: 3 * r // 4]).max() <= 4 * np.log2(r) * np.finfo(np.float32).eps * np.abs(want).max()
