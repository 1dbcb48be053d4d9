"""The 16384-point real-gain overlap-save kernel with its outer-pass twiddle powers resident (fastfir2_kernels.hip: K1_PWRES,
the product's build) against the build that rebuilds them in every block (K1_PWRES = 0, cutesdr_amd/libcutesdr_mi_pwres0.so),
word for word.

The powers are the same fp32 product tree on the same base twiddles, evaluated once in front of the block loop instead of
once per block, so every output word must be the same: the comparison is of bytes, not within a tolerance.  What can go wrong
is a power that a block finds overwritten (a register the loop reuses) or not yet built, so the cases are the ways the block
loop is entered and left: 1 block per call (the odd tail alone), 2 (one pair), 3 (pair and tail), 8; the runs the library
picks itself (blocks_per_wg = 0: at these channel counts it spreads a call over one workgroup per block, every run a single
block) and, where a call has more than one block, the whole call as one run (blocks_per_wg = blocks: pairs really walked,
with the tail after them) and for 8 blocks runs of 3, 3 and 2 (a run that starts at b0 > 0 on the input, not on the history);
3 channels (plain channel -> workgroup map) and 8 (the XCD map); two calls per object, the second on the history the first
left; the three filters of tests/test_fastfir_radix4_gpu.py in turn over the channels; host and device design; noise of 3000
rms, seed from (channels, blocks).  Each library runs in a fresh interpreter of its own, one after the other, asserts what it
was compiled with and the kernel of every launch, and writes its raw output words to a file.  So that two equally wrong
libraries do not pass, the product's words for 8 channels x 8 blocks are also held against the fp64 oracle at the kernels'
bound, |err| <= 2e-5 * max|x|."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-5
N, HOP = 16384, 8192
FILTERS = [(-250, 250, 700, 48000.0), (300, 2700, -800, 48000.0), (-5000, 5000, 0, 48000.0)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    """(channels, blocks per call, blocks_per_wg, device design), in the order both children walk them"""
    out = []
    for Cn in (3, 8):
        for nb in (1, 2, 3, 8):
            for bpw in [0] + ([3] if nb == 8 else []) + ([nb] if nb > 1 else []):
                for on_device in (False, True):
                    out.append((Cn, nb, bpw, on_device))
    return out


def noise(Cn, nb):
    """the two calls' input, [call, channel, sample]"""
    rng = np.random.default_rng(1000 * Cn + nb)
    return (3000.0 * (rng.standard_normal((2, Cn, nb * HOP)) + 1j * rng.standard_normal((2, Cn, nb * HOP)))).astype(np.complex64)


def words(Cn, nb):
    return 2 * Cn * nb * HOP * 8          # bytes one case writes: two calls of complex64 [channels, blocks * HOP]


def run_cases(out_path, expect_pwres):
    """(in the child) every case on the library this interpreter loaded; the output words of all of them to out_path"""
    import ctypes as C
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__fastfir_set_variant.restype = C.c_int
    L.csdr__fastfir_set_variant.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_last_kernel.restype = C.c_int
    L.csdr__fastfir_last_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.csdr__host_fastfir2_pwres.restype = C.c_int
    assert L.csdr__host_fastfir2_pwres() == expect_pwres, (L.csdr__host_fastfir2_pwres(), expect_pwres)

    def last_kernel(b):
        k, tw = C.c_int(-2), C.c_int(-2)
        assert L.csdr__fastfir_last_kernel(b.h, C.byref(k), C.byref(tw)) == 0
        return k.value

    inputs = {}
    with open(out_path, "wb") as f:
        for Cn, nb, bpw, on_device in cases():
            if (Cn, nb) not in inputs:
                inputs[(Cn, nb)] = noise(Cn, nb)
            x = inputs[(Cn, nb)]
            b = ca.FastFirBatch(Cn, N)
            flt = [FILTERS[c % 3] for c in range(Cn)]
            if on_device:
                b.setup(-5000, 5000, 0, 62500.0, channel=0)          # (per-channel filters first: the one call that reallocates)
                st = b.setup_many(list(range(Cn)), [q[0] for q in flt], [q[1] for q in flt], [q[2] for q in flt], [q[3] for q in flt])
                assert (st == 1).all()
            else:
                for c, q in enumerate(flt):
                    assert b.setup(*q, channel=c) == 1
            assert L.csdr__fastfir_set_variant(b.h, 2) == 0
            for call in (0, 1):
                y = b.process(x[call], blocks_per_wg=bpw)
                assert last_kernel(b) == 2, (Cn, nb, bpw, on_device, call, last_kernel(b))     # FASTFIR_KERNEL_PIPELINED_GAIN
                assert y.dtype == np.complex64 and y.shape == (Cn, nb * HOP)
                f.write(np.ascontiguousarray(y).tobytes())
            b.close()
    print("pwres=%d: %d cases written" % (expect_pwres, len(cases())))


def child(lib_path, out_path, expect_pwres):
    env = dict(os.environ)
    env.pop("CSDR_LIB_PATH", None)
    if lib_path:
        env["CSDR_LIB_PATH"] = lib_path
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_fastfir_pwres_gpu as t; t.run_cases(%r, %d)"
            % (ROOT, os.path.dirname(os.path.abspath(__file__)), out_path, expect_pwres))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "%d cases written" % len(cases()) in r.stdout, r.stdout[-2000:]
    return open(out_path, "rb").read()


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """{case: bytes} of the product library and of the K1_PWRES = 0 build (built here when __graft_entry__.build() has not: a
    missing compiler is an error), each from a fresh interpreter, one after the other"""
    from cutesdr_amd import _build
    name, flags = _build.PWRES0
    path = _build.alt_path(name)
    if not os.path.exists(path):
        assert _build.alt_lib(name, flags) == path
    d = tmp_path_factory.mktemp("pwres")
    raw = {"resident": child(None, str(d / "resident.bin"), 1), "pwres0": child(path, str(d / "pwres0.bin"), 0)}
    out = {}
    for which, data in raw.items():
        assert len(data) == sum(words(Cn, nb) for Cn, nb, _, _ in cases()), (which, len(data))
        at, out[which] = 0, {}
        for case in cases():
            out[which][case] = data[at:at + words(case[0], case[1])]
            at += words(case[0], case[1])
    return out


def test_resident_powers_give_the_same_words_as_powers_rebuilt_per_block(outputs):
    differ = []
    for case in cases():
        a, b = outputs["resident"][case], outputs["pwres0"][case]
        assert len(a) == len(b) == words(case[0], case[1])
        if a != b:
            wa, wb = np.frombuffer(a, dtype=np.uint32), np.frombuffer(b, dtype=np.uint32)
            differ.append((case, int((wa != wb).sum()), int(np.flatnonzero(wa != wb)[0])))
    print("%d cases, %d bytes per library; cases that differ (case, words, first word): %s"
          % (len(cases()), sum(len(v) for v in outputs["resident"].values()), differ))
    assert not differ, differ
    assert any(np.frombuffer(v, dtype=np.float32).any() for v in outputs["resident"].values())


def test_how_the_runs_are_cut_changes_no_word(outputs):
    """the same call as one workgroup per block, as one run, and as runs of 3, 3, 2: the same words (product library)"""
    for Cn in (3, 8):
        for nb in (2, 3, 8):
            for on_device in (False, True):
                want = outputs["resident"][(Cn, nb, 0, on_device)]
                for bpw in ([3] if nb == 8 else []) + [nb]:
                    assert outputs["resident"][(Cn, nb, bpw, on_device)] == want, (Cn, nb, bpw, on_device)


@pytest.mark.parametrize("bpw", [0, 3, 8])
def test_resident_words_match_the_oracle(oracle, outputs, bpw):
    """8 channels x 8 blocks x two calls of the product library against the fp64 oracle (host design)"""
    Cn, nb = 8, 8
    x = noise(Cn, nb)
    y = np.frombuffer(outputs["resident"][(Cn, nb, bpw, False)], dtype=np.complex64).reshape(2, Cn, nb * HOP)
    if "ref" not in _oracle:
        ref = []
        for c in range(Cn):
            ff = oracle.CFastFIR(N)
            assert ff.SetupParameters(*FILTERS[c % 3]) == 1
            ref.append(np.concatenate([ff.ProcessData(x[0, c].astype(np.complex128)), ff.ProcessData(x[1, c].astype(np.complex128))]))
        _oracle["ref"] = np.stack(ref)
        _oracle["ref"].setflags(write=False)
    got = np.concatenate([y[0], y[1]], axis=1)
    err = np.abs(got - _oracle["ref"]).max(axis=1) / np.abs(x).max()
    print("blocks_per_wg=%d: max err / max|x| per channel %s (bound %.3g)" % (bpw, err, TOL))
    assert (err <= TOL).all(), err


_oracle = {}
