"""The fp64 twiddle tables of the batch transforms (K3q), without a GPU: what csdr_fft_batch_prepare_f64 uploads
(reached through the csdr__host_fft_tw64 hook) must be, entry for entry at every size, the long double value rounded once
to fp64, as fft_plain64_ref.table restates it; the builder runs clean under AddressSanitizer / UBSan as a stand-alone
program on the CPU; and the kernels' pass functions, walked thread by thread in a host program, meet the rule and the
impulse bound of the device tests at every size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fft_plain64_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build
    lib = C.CDLL(_build.build())
    lib.csdr__host_fft_tw64.restype = C.c_int
    lib.csdr__host_fft_tw64.argtypes = [C.c_int, C.c_void_p, C.c_int]
    return lib


def library_table(L, n):
    count = L.csdr__host_fft_tw64(n, None, 0)
    assert count > 0
    out = np.full(count + 2, -7.0)
    assert L.csdr__host_fft_tw64(n, out.ctypes.data, count) == count
    assert (out[count:] == -7.0).all()
    return out[:count].reshape(-1, 2)


@pytest.mark.parametrize("n", P.SIZES)
def test_every_entry_is_the_rounded_long_double_value(L, n):
    P.require_long_double()
    got, want = library_table(L, n), P.table(n)
    assert got.shape == want.shape == ((n, 2) if n < 8192 else (512, 2))
    bad = np.nonzero(P.words(got) != P.words(want))[0]
    assert len(bad) == 0, "n=%d: %d entries differ, first %s" % (n, len(bad), bad[:8])
    # ... and that value is the angle's: it agrees with the fp64 library's as far as that can tell (two roundings of
    # 2^-53 and the fp64 angle's own error, two relative roundings of the angle), lies on the unit circle, is exact at the
    # axes and has equal parts on the diagonals
    period = [n] if n < 8192 else [256, n]
    for i, p in enumerate(period):
        t = got if n < 8192 else got[256 * i:256 * (i + 1)]
        a = 2.0 * np.pi * np.arange(len(t)) / p
        tol = 2.0 ** -53 * (2.0 + 2.0 * a)
        assert (np.abs(t[:, 0] - np.cos(a)) <= tol).all() and (np.abs(t[:, 1] - np.sin(a)) <= tol).all()
        assert np.abs(t[:, 0] ** 2 + t[:, 1] ** 2 - 1.0).max() <= 2.0 ** -51
        assert t[0].tolist() == [1.0, 0.0]
        if len(t) == p:
            assert t[p // 4].tolist() == [0.0, 1.0] and t[p // 2].tolist() == [-1.0, 0.0] and t[3 * p // 4].tolist() == [0.0, -1.0]
            assert t[p // 8, 0] == t[p // 8, 1] and t[3 * p // 8, 0] == -t[3 * p // 8, 1]
    assert not np.signbit(got[got == 0.0]).any(), "a negative zero"


def test_hook_refuses_other_sizes(L):
    for n in (0, 256, 1000, 131072):
        assert L.csdr__host_fft_tw64(n, None, 0) < 0


def test_builder_under_address_and_ub_sanitizer(tmp_path):
    """the table builder alone, compiled with -fsanitize=address,undefined into a program with its own main"""
    P.require_long_double()
    exe, out = str(tmp_path / "fft_tw64_san"), str(tmp_path / "tables.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "cutesdr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fft_tw64_san.cpp"),
                           "-o", exe])
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(out).reshape(-1, 2)
    want = np.concatenate([P.table(n) for n in P.SIZES])
    assert got.shape == want.shape and (P.words(got) == P.words(want)).all()


# ---- the kernels' passes walked on the host (tests/cpp/fft_plain64_emu.hip): the same pass functions, butterflies, index
# arithmetic and tables as the device's, one frame at a time, held to the device tests' rule
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    from cutesdr_amd import _build
    d = tmp_path_factory.mktemp("emu64")
    exe = str(d / "fft_plain64_emu")
    subprocess.check_call([_build._hipcc(), "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "--cuda-host-only", "-x", "hip",
                           "-I", os.path.join(ROOT, "cutesdr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fft_plain64_emu.hip"),
                           "-o", exe])

    def run(x, sign):
        np.ascontiguousarray(x, dtype=np.complex128).tofile(d / "in.bin")
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin"), str(sign)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return np.fromfile(d / "out.bin", dtype=np.complex128)
    return run


@pytest.mark.parametrize("n", P.SIZES)
def test_passes_on_the_host_meet_the_rule(emu, n):
    P.require_long_double()
    seed = P.seed_of(n, 0)
    for sign in P.SIGNS:
        e, eo = P.check_frame(emu(P.probe(n, seed), sign), n, seed, sign, "host walk")
        print("host walk n=%d sign=%+d: E / E_y = %.2f (allowed %g), the oracle's %.2f" % (n, sign, e, P.MARGIN, eo))
    amp = 3000.0
    for m in (1, n // 2 + 3):
        x = np.zeros(n, dtype=np.complex128)
        x[m] = amp
        for sign in P.SIGNS:
            err = float(np.abs(emu(x, sign).astype(P.CLD) - P.impulse_ref(n, m, sign, amp)).max())
            print("host walk impulse n=%d m=%d sign=%+d: %.3g of the allowed %.3g" % (n, m, sign, err, 4 * 2.0 ** -52 * amp))
            assert err <= 4 * 2.0 ** -52 * amp, (n, m, sign, err)
