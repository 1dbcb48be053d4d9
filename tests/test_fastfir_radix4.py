"""CPU tests of the radix-4 tail groups of the 16384-point real-gain overlap-save kernel (fft_core.hpp: dit_tail_r4,
dit_tail_middle_r4; fastfir2_kernels.hip: K1_RADIX4; no GPU).

The last two stages of every register network of that kernel are four radix-2 butterflies per group of four points,
A' = A + alpha B, B' = A - alpha B, C' = C + alpha D, D' = C - alpha D, then A'' = A' + beta C', C'' = A' - beta C',
B'' = B' + s j beta D', D'' = B' - s j beta D' (alpha = beta^2, s the transform's sign).  The radix-4 form writes a unit twiddle
as j^rot m (1 + j tau), |tau| <= 1, and shares the products: eleven packed instructions instead of twelve, another
rounding order.  Checked here on host builds of the same templates the kernel compiles:
  * every group (radix 16 and 32, both signs, every group index, all four outputs and the pruned pair) against the
    four-point DFT of the twiddled points (A, beta C, alpha B, alpha beta D) in fp64;
  * the whole radix-16 / radix-32 networks on those groups against a direct fp64 DFT;
  * a numpy model of one 16384-point block whose six networks end in the radix-4 groups, fp64, against
    RevFFT(FwdFFT(x) . H), and the same block through the host builds in fp32 against the GPU tests' bound.
Bounds of the first two: the ones tests/test_fastfir_realgain.py uses for dit_head4_gain (two fp32 stages: 8 eps of the
largest output) and dit_tail_middle (log2 R stages: 4 log2(R) eps)."""
import ctypes as C
import numpy as np
import pytest

EPS = float(np.finfo(np.float32).eps)
RMS = 3000.0
GPU_TOL = 2e-5                     # the GPU tests' bound: |err| <= GPU_TOL * max|x|
NARROW = (-250, 250, 700, 48000.0)


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_dit_tail_r4.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2
    lib.csdr__host_dft_r4.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2
    lib.csdr__host_dft_middle.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.csdr__host_tw_factors.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.csdr__host_fastfir_gains.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_void_p] * 2
    return lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def noise(rng, *shape):
    return RMS * np.sqrt(0.5) * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def dft(x, sign):
    n = x.shape[-1]
    k = np.arange(n)
    return x @ np.exp(sign * 2j * np.pi * np.outer(k, k) / n)


def bitrev(v, bits):
    return int("{:0{w}b}".format(v, w=bits)[::-1], 2)


def tw_factors(k, sign):
    """e^{sign j 2 pi k/32} = j^rot m (1 + j tau), |tau| <= 1 (fft_core.hpp: tw_factors; a tie keeps rot = 0)"""
    c, s = np.cos(2 * np.pi * k / 32), sign * np.sin(2 * np.pi * k / 32)
    if abs(c) >= abs(s) - 1e-12:
        return 0, c, s / c
    return 1, s, -c / s


@pytest.mark.parametrize("sign", [+1, -1])
def test_twiddle_factors_compose_to_the_twiddle(L, sign):
    for k in range(32):
        if k % 8 == 0:
            continue                                   # 1, +-j, -1: the groups never factor those
        m, tau = C.c_double(), C.c_double()
        rot = L.csdr__host_tw_factors(k, sign, C.byref(m), C.byref(tau))
        assert abs(tau.value) <= 1.0
        w = 1j ** rot * m.value * (1 + 1j * tau.value)
        assert abs(w - np.exp(sign * 2j * np.pi * k / 32)) <= 1e-15
        prot, pm, ptau = tw_factors(k, sign)
        assert rot == prot and abs(m.value - pm) <= 1e-15 and abs(tau.value - ptau) <= 1e-15


@pytest.mark.parametrize("middle", [0, 1], ids=["all_rows", "pruned"])
@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("r", [16, 32])
def test_every_group_is_the_four_point_dft_of_the_twiddled_points(L, r, sign, middle):
    rng = np.random.default_rng(100 * r + sign + middle)
    worst = 0.0
    for i in range(r // 4):
        beta = np.exp(sign * 2j * np.pi * i / r)
        for _ in range(8):
            x = noise(rng, 4).astype(np.complex64)                     # A, B, C, D
            out = np.zeros(4, dtype=np.complex64)
            assert L.csdr__host_dit_tail_r4(r, sign, i, middle, vp(x), vp(out)) == 0
            a, b, c, d = x.astype(np.complex128)
            want = dft(np.array([a, beta * c, beta ** 2 * b, beta ** 3 * d]), sign)    # rows I, I + R/4, I + R/2, I + 3R/4
            rows = [1, 2] if middle else [0, 1, 2, 3]
            err = np.abs(out[rows] - want[rows]).max() / np.abs(want).max()
            worst = max(worst, err)
            # two fp32 stages: a few ulp of the largest magnitude (test_fastfir_realgain.py, dit_head4_gain)
            assert err <= 8 * EPS, (r, sign, i, middle, err)
    print("R=%d sign=%+d %s: largest err / max|want| over the groups %.3g (bound %.3g)" % (r, sign, "pruned" if middle else "all rows", worst, 8 * EPS))
    assert L.csdr__host_dit_tail_r4(r, sign, r // 4, middle, vp(x), vp(out)) == -1
    assert L.csdr__host_dit_tail_r4(8, sign, 0, middle, vp(x), vp(out)) == -1


@pytest.mark.parametrize("middle", [0, 1], ids=["all_rows", "middle_rows"])
@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("r", [16, 32])
def test_networks_on_radix4_tails_are_the_dft(L, r, sign, middle):
    rng = np.random.default_rng(r + sign + 7 * middle)
    worst = 0.0
    for _ in range(8):
        x = noise(rng, r).astype(np.complex64)
        out = np.zeros(r // 2 if middle else r, dtype=np.complex64)
        assert L.csdr__host_dft_r4(r, sign, middle, vp(x), vp(out)) == 0
        want = dft(x.astype(np.complex128), sign)
        got = want[r // 4: 3 * r // 4] if middle else want
        err = np.abs(out - got).max() / np.abs(want).max()
        worst = max(worst, err)
        # log2(r) fp32 stages: error grows like eps * log2(r) * max|X| (test_fastfir_realgain.py, dit_tail_middle)
        assert err <= 4 * np.log2(r) * EPS, (r, sign, middle, err)
    print("R=%d sign=%+d %s: largest err / max|X| %.3g (bound %.3g)" % (r, sign, "middle rows" if middle else "all rows", worst, 4 * np.log2(r) * EPS))


# ---- one 16384-point block ------------------------------------------------------------------------------------------
def jrot(v, rot):
    return v * 1j ** (rot % 4)


def network(x, sign, middle=False):
    """DIT transform over the last axis (R = 16 or 32 points, natural order in and out) as the kernel's register networks
    run it: radix-2 stages up to R/4, then the radix-4 tail groups, step by step as dit_tail_r4_group writes them
    (groups whose alpha is 1 or +-j as plain butterflies); middle: only rows R/4 ... 3R/4 - 1 are finished and returned"""
    r = x.shape[-1]
    bits = r.bit_length() - 1
    y = x[..., [bitrev(p, bits) for p in range(r)]].astype(np.complex128)
    ln = 2
    while ln <= r // 4:
        v = y.reshape(y.shape[:-1] + (r // ln, ln))
        a, b = v[..., : ln // 2], v[..., ln // 2:] * np.exp(sign * 2j * np.pi * np.arange(ln // 2) / ln)
        y = np.concatenate([a + b, a - b], axis=-1).reshape(y.shape)
        ln *= 2
    q = r // 4
    out = np.array(y)
    for i in range(q):
        A, B, Cc, D = y[..., i], y[..., i + q], y[..., i + 2 * q], y[..., i + 3 * q]
        ka, kb = i * (64 // r), i * (32 // r)
        if ka % 8 == 0:
            al, be = np.exp(sign * 2j * np.pi * ka / 32), np.exp(sign * 2j * np.pi * kb / 32)
            a1, b1, c1, d1 = A + al * B, A - al * B, Cc + al * D, Cc - al * D
            res = (a1 + be * c1, b1 + sign * 1j * be * d1, a1 - be * c1, b1 - sign * 1j * be * d1)
        else:
            (ra, ma, ta), (rb, mb, tb), (rg, mg, tg) = tw_factors(ka, sign), tw_factors(kb, sign), tw_factors(ka + kb, sign)
            rr, ratio, sj = rg - rb, mg / mb, (1 if sign > 0 else 3)
            bh = B + 1j * ta * B
            t1, t2 = A + jrot(bh, ra) * ma, A + jrot(bh, ra + 2) * ma
            ch, dh = Cc + 1j * tb * Cc, D + 1j * tg * D
            s1, s2 = ch + jrot(dh, rr) * ratio, ch + jrot(dh, rr + 2) * ratio
            res = (t1 + jrot(s1, rb) * mb, t2 + jrot(s2, rb + sj) * mb, t1 + jrot(s1, rb + 2) * mb, t2 + jrot(s2, rb + sj + 2) * mb)
        for p in range(4):
            out[..., i + p * q] = res[p]
    return out[..., q: 3 * q] if middle else out


def host_network(L, x, sign, middle=False):
    """the same transform over the last axis through the host build of the kernel's fp32 templates"""
    r = x.shape[-1]
    flat = np.ascontiguousarray(x.reshape(-1, r).astype(np.complex64))
    out = np.zeros((flat.shape[0], r // 2 if middle else r), dtype=np.complex64)
    for row in range(flat.shape[0]):
        assert L.csdr__host_dft_r4(r, sign, int(middle), vp(flat[row]), vp(out[row])) == 0
    return out.reshape(x.shape[:-1] + (out.shape[1],))


def block(x, H, net, rnd=lambda v: v, middle=False):
    """one 16384-point block as 16 x 32 x 32 with the kernel's six networks (every row on its own pass twiddle: the shared
    ones change no network, tests/test_fastfir_twshare.py): samples [n1, 32 m1 + sn] -> F1 over n1 -> F2 over m1 -> F3
    over sn -> times H -> I1, I2, I3.  rnd rounds what a pass leaves (fp32 for the host builds)"""
    n, r0 = 16384, 16
    a32 = np.arange(32)
    table = np.exp(2j * np.pi * np.outer(a32, a32) / 1024)                       # [k1, sn]
    power = np.exp(2j * np.pi * np.outer(np.arange(r0), np.arange(1024)) / n)    # [k0, n2]
    pos = np.array([[[k0 + r0 * (k1 + 32 * j) for j in range(32)] for k1 in range(32)] for k0 in range(r0)])
    a = rnd(net(x.reshape(r0, 1024).T, +1).T * power)                            # F1: [k0, n2]
    b = rnd(np.swapaxes(net(np.swapaxes(a.reshape(r0, 32, 32), 1, 2), +1), 1, 2) * table)      # F2: [k0, k1, sn]
    c = rnd(net(b, +1) * H[pos])                                                 # F3, times H: [k0, k1, j]
    d = rnd(net(c, -1) * np.conj(table))                                         # I1: [k0, k1, sn]
    e = rnd(np.swapaxes(net(np.swapaxes(d, 1, 2), -1), 1, 2).reshape(r0, 1024) * np.conj(power))    # I2: [k0, n2]
    if middle:
        return net(e.T, -1, middle=True).T.reshape(-1)                           # I3: rows 4 ... 11
    return net(e.T, -1).T.reshape(-1)


def direct(x, H):
    n = len(x)
    return n * np.fft.fft(np.fft.ifft(x) * H)             # forward sign +1 unnormalised, times H, inverse sign -1 unnormalised


def test_model_networks_are_dfts():
    rng = np.random.default_rng(3)
    for r in (16, 32):
        for sign in (+1, -1):
            x = noise(rng, 5, r)
            want = dft(x, sign)
            assert np.abs(network(x, sign) - want).max() <= 1e-12 * np.abs(want).max()
            assert np.abs(network(x, sign, middle=True) - want[:, r // 4: 3 * r // 4]).max() <= 1e-12 * np.abs(want).max()


def test_block_on_radix4_networks_equals_the_direct_round_trip():
    rng = np.random.default_rng(14)
    n = 16384
    x = noise(rng, n)
    H = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    want = direct(x, H)
    err = np.abs(block(x, H, network) - want).max() / np.abs(want).max()
    mid = np.abs(block(x, H, network, middle=True) - want[n // 4: 3 * n // 4]).max() / np.abs(want).max()
    print("fp64 block on radix-4 networks: max err / max|y| = %.3g, middle rows %.3g" % (err, mid))
    assert err <= 1e-10 and mid <= 1e-10


def test_fp32_block_through_the_host_builds_is_inside_the_gpu_bound(L):
    """The library's own narrow design (real gains P: the kernel's multiply; the quarter-block shift is I3 keeping rows 4 ... 11)
    and noise of 3000 rms: the block through the host builds of the fp32 networks, every pass rounded to fp32, against
    the fp64 round trip on the same multipliers -- the bound of the GPU tests"""
    n = 16384
    Hd = np.zeros(n, dtype=np.complex128)
    P = np.zeros(n, dtype=np.float64)
    assert L.csdr__host_fastfir_gains(n, *NARROW, vp(Hd), vp(P)) == 0
    rng = np.random.default_rng(5)
    x = noise(rng, n).astype(np.complex64).astype(np.complex128)
    P32 = P.astype(np.float32).astype(np.float64)
    want = direct(x, P32)[n // 4: 3 * n // 4]
    got = block(x, P32, lambda v, s, middle=False: host_network(L, v, s, middle), rnd=lambda v: v.astype(np.complex64), middle=True)
    err = np.abs(got - want).max() / np.abs(x).max()
    print("fp32 block on the host builds of the radix-4 networks: max err / max|x| = %.3g (bound %.3g)" % (err, GPU_TOL))
    assert err <= GPU_TOL


def test_the_product_builds_the_radix4_form(L):
    assert L.csdr__host_fastfir2_radix4() == 1
