"""CPU tests of the shared pass twiddles of the 16384-point pipelined overlap-save kernels (fastfir2_kernels.hip,
K1_TWSHARE; no GPU).  The identity holds at every size and the model checks it at three; the library builds it at
N = 16384 only, and the hook test pins that: no rotation at 2048, 4096 and 8192 points.

The kernels split an N = R0 x 1024 point transform as R0 x 32 x 32.  Row k1 of the middle pass is multiplied by the table
entry W_1024^(sn k1); rows 17 ... 31 take conj(entry 32 - k1) instead, which is W_32^(-sn) off, and the last pass -- a
transform over sn -- turns that factor into a circular shift of its 32 outputs by one bin.  Nothing in the kernel looks at
what bin a register holds; only the order in which H (or the gains) is uploaded does.  The same algebra one level up
(rows k0 > R0 / 2 of the outer pass on conj(power R0 - k0)) shifts a whole 1024-point sub-transform by one bin.

`Model` below is that transform pair in numpy, fp64, with either sharing switched on, and the slot -> bin map that goes
with it.  The tests check the identity against a direct DFT round trip, the library's composed slot -> bin hook against
the model's map, and that a missing or reversed rotation is a gross error at the filter the GPU test uses."""
import ctypes as C
import numpy as np
import pytest

GPU_TOL = 2e-5                     # the GPU tests' bound: |err| <= GPU_TOL * max|x| (tests/test_fastfir_twshare_gpu.py)
NARROW = (-250, 250, 700, 48000.0)


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    for name in ("csdr__host_fastfir2_bin_of", "csdr__host_fastfir2_gain_bin_of", "csdr__host_fastfir2_slot_bin",
                 "csdr__host_fastfir2_gain_slot_bin"):
        getattr(lib, name).argtypes = [C.c_int] * 4
    lib.csdr__host_fastfir2_twshare_shift.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.csdr__host_fastfir2_twshare_shift.restype = None
    lib.csdr__host_fastfir_design.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_void_p]
    return lib


class Model:
    """forward (sign +1) and inverse transform of N = r0 * 1024 points as r0 x 32 x 32 with the kernel's passes; `inner` /
    `outer`: rows from 17 of the radix-32 pass / rows above r0 / 2 of the outer pass run on the conjugate of the twiddle of
    row 32 - k1 / r0 - k0.  position (k0, k1, j) is output j of row k1 of sub-transform k0."""

    def __init__(self, r0, inner, outer):
        self.r0, self.n, self.inner, self.outer = r0, 1024 * r0, inner, outer
        a = np.arange(32)
        self.w32 = np.exp(2j * np.pi * np.outer(a, a) / 32)
        self.wr0 = np.exp(2j * np.pi * np.outer(np.arange(r0), np.arange(r0)) / r0)
        table = np.exp(2j * np.pi * np.outer(a, a) / 1024)                       # [k1, sn], the kernel's tw2
        power = np.exp(2j * np.pi * np.outer(np.arange(r0), np.arange(1024)) / self.n)      # [k0, n2], the kernel's pw
        self.tw = np.stack([np.conj(table[32 - k]) if inner and k >= 17 else table[k] for k in range(32)])
        self.itw = np.stack([table[32 - k] if inner and k >= 17 else np.conj(table[k]) for k in range(32)])
        self.pw = np.stack([np.conj(power[r0 - k]) if outer and 2 * k > r0 else power[k] for k in range(r0)])
        self.ipw = np.stack([power[r0 - k] if outer and 2 * k > r0 else np.conj(power[k]) for k in range(r0)])

    def inner_shift(self, k1):
        return 1 if self.inner and k1 >= 17 else 0

    def outer_shift(self, k0):
        return 1 if self.outer and 2 * k0 > self.r0 else 0

    def bin_of(self, k0, k1, j, direction=1, rotate=True):
        """natural bin held at position (k0, k1, j); direction = -1 rotates the wrong way, rotate=False not at all"""
        si, so = (direction * self.inner_shift(k1), direction * self.outer_shift(k0)) if rotate else (0, 0)
        sub = (k1 + 32 * ((j - si) % 32) - so) % 1024
        return k0 + self.r0 * sub

    def positions(self, **kw):
        """[k0, k1, j] -> natural bin"""
        r0 = self.r0
        return np.array([[[self.bin_of(k0, k1, j, **kw) for j in range(32)] for k1 in range(32)] for k0 in range(r0)])

    def forward(self, x):
        a = (self.wr0 @ x.reshape(self.r0, 1024)) * self.pw                      # F1: [k0, n2], n2 = 32 m1 + sn
        b = np.einsum("km,rms->rks", self.w32, a.reshape(self.r0, 32, 32)) * self.tw         # F2: [k0, k1, sn]
        return np.einsum("rks,sj->rkj", b, self.w32)                             # F3: [k0, k1, j]

    def inverse(self, c):
        d = np.einsum("rkj,js->rks", c, np.conj(self.w32)) * self.itw            # I1, I2's twiddle
        e = np.einsum("mk,rks->rms", np.conj(self.w32), d).reshape(self.r0, 1024) * self.ipw      # I2, I3's twiddle
        return (np.conj(self.wr0) @ e).reshape(-1)                               # I3 (unnormalised)

    def filter(self, x, H, **kw):
        """circular convolution of one block with the response H (natural order), multiplied where positions() says"""
        return self.inverse(self.forward(x) * H[self.positions(**kw)])


def direct(x, H):
    n = len(x)
    return n * np.fft.fft(np.fft.ifft(x) * H)             # forward sign +1 unnormalised, times H, inverse sign -1 unnormalised


@pytest.mark.parametrize("inner,outer", [(True, False), (True, True), (False, True)], ids=["inner", "inner+outer", "outer"])
@pytest.mark.parametrize("r0", [2, 4, 16], ids=["N=2048", "N=4096", "N=16384"])
def test_round_trip_on_shared_twiddles_equals_the_direct_one(r0, inner, outer):
    rng = np.random.default_rng(r0)
    n = 1024 * r0
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    H = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    m = Model(r0, inner, outer)
    pos = m.positions()
    assert np.array_equal(np.sort(pos.reshape(-1)), np.arange(n))
    want = direct(x, H)
    err = np.abs(m.filter(x, H) - want).max() / np.abs(want).max()
    plain = np.abs(Model(r0, False, False).filter(x, H) - want).max() / np.abs(want).max()
    print("r0=%d inner=%s outer=%s: max err / max|y| = %.3g (own twiddles: %.3g)" % (r0, inner, outer, err, plain))
    assert err <= 1e-10 and plain <= 1e-10
    # the spectrum itself: position (k0, k1, j) holds the bin the map says
    X = n * np.fft.ifft(x)
    assert np.abs(m.forward(x) - X[pos]).max() <= 1e-10 * np.abs(X).max()


def shifts(L, log2n, t):
    a, b = C.c_int(-9), C.c_int(-9)
    L.csdr__host_fastfir2_twshare_shift(log2n, t, C.byref(a), C.byref(b))
    return a.value, b.value


@pytest.mark.parametrize("log2n", [11, 12, 13, 14])
def test_composed_slot_map_is_a_permutation_and_the_models_map(L, log2n):
    """csdr__host_fastfir2_slot_bin / _gain_slot_bin: a permutation of the bins, the base order on every thread whose
    shifts are zero, and on every thread the model's map for the shifts the library reports -- at N = 16384 the inner one
    on rows from 17 (and, where a build shares the outer powers too, the outer one on sub-transforms above R0 / 2), none
    at the smaller sizes, whose kernels keep a twiddle per row"""
    n, r0 = 1 << log2n, (1 << log2n) // 1024
    T = n // 32
    seen = np.zeros(n, dtype=int)
    shifted = 0
    for t in range(T):
        k0, k1 = t >> 5, t & 31
        si, so = shifts(L, log2n, t)
        assert si == (1 if (k1 >= 17 and log2n == 14) else 0), (t, si)
        assert so in (0, 1) and (so == 0 or 2 * k0 > r0), (t, so)
        shifted += 1 if (si or so) else 0
        for j in range(16):
            for e in range(2):
                k = L.csdr__host_fastfir2_slot_bin(log2n, t, j, e)
                base = L.csdr__host_fastfir2_bin_of(log2n, t, j, e)
                k2 = (j >> 1) + 8 * (j & 1) + 16 * e
                assert base == k0 + r0 * (k1 + 32 * k2)
                assert k == k0 + r0 * ((k1 + 32 * ((k2 - si) % 32) - so) % 1024), (t, j, e)
                if not si and not so:
                    assert k == base
                seen[k] += 1
        for i in range(8):
            for c in range(4):
                assert L.csdr__host_fastfir2_gain_slot_bin(log2n, t, i, c) == L.csdr__host_fastfir2_slot_bin(log2n, t, 2 * i + (c >> 1), c & 1)
                if not si and not so:
                    assert L.csdr__host_fastfir2_gain_slot_bin(log2n, t, i, c) == L.csdr__host_fastfir2_gain_bin_of(log2n, t, i, c)
    assert (seen == 1).all()
    assert shifted >= (T * 15 // 32 if log2n == 14 else 0)           # the rotation is there: fifteen rows of every sub-transform


def test_a_missing_or_reversed_rotation_is_a_gross_error_at_the_gpu_tests_narrow_filter(L):
    """The library's own design for (-250, 250, 700) at 48 kHz, N = 16384, noise of 3000 rms through the model on shared
    twiddles: with the response uploaded in the unrotated order, or rotated the wrong way, the output is off by at least
    100 x the GPU test's bound -- so that test cannot pass with a wrong or missing rotation."""
    n = 16384
    H = np.zeros(n, dtype=np.complex128)
    assert L.csdr__host_fastfir_design(n, *NARROW, H.ctypes.data_as(C.c_void_p)) == 0
    # (the design carries the 1/N of the unnormalised transform pair: the pass band's gain is one)
    rng = np.random.default_rng(5)
    x = 3000.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    bound = GPU_TOL * np.abs(x).max()
    want = direct(x, H)
    for inner, outer in ((True, False), (True, True)):
        m = Model(16, inner, outer)
        assert np.abs(m.filter(x, H) - want).max() <= 1e-10 * np.abs(x).max()
        missing = np.abs(m.filter(x, H, rotate=False) - want).max()
        reversed_ = np.abs(m.filter(x, H, direction=-1) - want).max()
        print("inner=%s outer=%s: rotation missing: max err = %.4g = %.1f x bound; reversed: %.4g = %.1f x bound (bound %.4g)"
              % (inner, outer, missing, missing / bound, reversed_, reversed_ / bound, bound))
        assert missing >= 100 * bound and reversed_ >= 100 * bound
