"""The 16384-point real-gain overlap-save kernel as the product builds it -- no fetch behind the last block of a run and the
history tail stored from inside the call's last block (fastfir2_kernels.hip: K1_RUNEND), a block's loads in four pairs
(K1_LDSPREAD) -- and with the two knobs the product leaves off as well -- one round trip in front of the block loop
(K1_PROLOGUE), no twiddle table in LDS (K1_TW2LDS): cutesdr_amd/libcutesdr_mi_hbmall.so -- against the build with all four
at 0 (cutesdr_amd/libcutesdr_mi_runend0.so, the instruction stream before them), word for word.

None of the knobs touches the arithmetic, so every output word must be the same: the comparison is of bytes, not within a
tolerance.  What can go wrong is a block that computes on the zeros an empty range returns instead of on samples (the range
emptied one block early), a history half that is stale, incomplete or written by the wrong block, and a power or a twiddle
that is used before it is there.  So the cases are the ways a run is entered and left: 1 block per call (the odd tail alone,
first and last block at once), 2 (one pair: the last block is the second of a pair), 3 (pair and tail), 8 (four pairs); the
runs the library picks itself (blocks_per_wg = 0: at these channel counts one workgroup per block, so every run but one ends
inside the call and must not write the history) and the whole call as one run (blocks_per_wg = blocks); 3 channels (plain
channel -> workgroup map) and 8 (the XCD map); THREE calls per object, so the history a call's last block wrote is what the
next call starts from, in either half of the ping-pong; the three filters of tests/test_fastfir_radix4_gpu.py in turn over
the channels; host and device design; noise of 3000 rms, seed from (channels, blocks).  Each library runs in a fresh
interpreter of its own, one after the other, asserts what it was compiled with and the kernel of every launch, and writes its
raw output words, and both history halves after the last call, to a file.  So that two equally wrong libraries do not pass,
the product's words of every case are also held against the fp64 oracle at the kernels' bound, |err| <= 2e-5 * max|x|."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-5
N, HOP, CALLS = 16384, 8192, 3
PRODUCT_KNOBS = 1 | 8          # what the product ships: K1_RUNEND and K1_LDSPREAD (bits: tests/test_fastfir_runend.py)
FILTERS = [(-250, 250, 700, 48000.0), (300, 2700, -800, 48000.0), (-5000, 5000, 0, 48000.0)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    """(channels, blocks per call, blocks_per_wg, device design), in the order both children walk them"""
    return [(Cn, nb, bpw, on_device) for Cn in (3, 8) for nb in (1, 2, 3, 8) for bpw in (0, nb) for on_device in (False, True)]


def noise(Cn, nb):
    """the calls' input, [call, channel, sample]"""
    rng = np.random.default_rng(7000 * Cn + nb)
    return (3000.0 * (rng.standard_normal((CALLS, Cn, nb * HOP)) + 1j * rng.standard_normal((CALLS, Cn, nb * HOP)))).astype(np.complex64)


def out_bytes(Cn, nb):
    return CALLS * Cn * nb * HOP * 8          # the calls' complex64 [channels, blocks * HOP]


def hist_bytes(Cn):
    return 2 * Cn * HOP * 8                   # both ping-pong halves, complex64 [channels, HOP] each


def run_cases(out_path, expect_knobs):
    """(in the child) every case on the library this interpreter loaded; per case the output words of the calls and both
    history halves after the last call to out_path (which half the next call would read is asserted here)"""
    import ctypes as C
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__fastfir_set_variant.restype = C.c_int
    L.csdr__fastfir_set_variant.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_last_kernel.restype = C.c_int
    L.csdr__fastfir_last_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.csdr__fastfir_read_history.restype = C.c_int
    L.csdr__fastfir_read_history.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.csdr__host_fastfir2_hbm_knobs.restype = C.c_int
    assert L.csdr__host_fastfir2_hbm_knobs() == expect_knobs, (L.csdr__host_fastfir2_hbm_knobs(), expect_knobs)

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
            for call in range(CALLS):
                y = b.process(x[call], blocks_per_wg=bpw)
                assert last_kernel(b) == 2, (Cn, nb, bpw, on_device, call, last_kernel(b))     # FASTFIR_KERNEL_PIPELINED_GAIN
                assert y.dtype == np.complex64 and y.shape == (Cn, nb * HOP)
                f.write(np.ascontiguousarray(y).tobytes())
            hist, cur = np.zeros((2, Cn, HOP), dtype=np.complex64), C.c_int(-1)
            assert L.csdr__fastfir_read_history(b.h, hist.ctypes.data, C.byref(cur)) == 0
            assert cur.value == CALLS % 2, cur.value
            f.write(hist.tobytes())
            b.close()
    print("knobs=%d: %d cases written" % (expect_knobs, len(cases())))


def child(lib_path, out_path, expect_knobs):
    env = dict(os.environ)
    env.pop("CSDR_LIB_PATH", None)
    if lib_path:
        env["CSDR_LIB_PATH"] = lib_path
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_fastfir_runend_gpu as t; t.run_cases(%r, %d)"
            % (ROOT, os.path.dirname(os.path.abspath(__file__)), out_path, expect_knobs))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "%d cases written" % len(cases()) in r.stdout, r.stdout[-2000:]
    return open(out_path, "rb").read()


def product_knobs():
    """what the product library says it was compiled with (bits: tests/test_fastfir_runend.py)"""
    import ctypes as C
    from cutesdr_amd import _capi
    L = _capi.lib()
    L.csdr__host_fastfir2_hbm_knobs.restype = C.c_int
    return L.csdr__host_fastfir2_hbm_knobs()


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """{library: {case: (output bytes, history bytes)}} of the product library, of the all-knobs-on and of the knobs-off build
    (built here when __graft_entry__.build() has not: a missing compiler is an error), each from a fresh interpreter, one
    after the other"""
    from cutesdr_amd import _build
    paths = {}
    for name, flags in (_build.RUNEND0, _build.HBMALL):
        paths[name] = _build.alt_path(name)
        if not os.path.exists(paths[name]):
            assert _build.alt_lib(name, flags) == paths[name]
    assert product_knobs() == PRODUCT_KNOBS, product_knobs()
    d = tmp_path_factory.mktemp("runend")
    raw = {"product": child(None, str(d / "product.bin"), PRODUCT_KNOBS),
           "allon": child(paths["hbmall"], str(d / "allon.bin"), 15),
           "knobs0": child(paths["runend0"], str(d / "knobs0.bin"), 0)}
    out = {}
    for which, data in raw.items():
        assert len(data) == sum(out_bytes(Cn, nb) + hist_bytes(Cn) for Cn, nb, _, _ in cases()), (which, len(data))
        at, out[which] = 0, {}
        for case in cases():
            no, nh = out_bytes(case[0], case[1]), hist_bytes(case[0])
            out[which][case] = (data[at:at + no], data[at + no:at + no + nh])
            at += no + nh
    return out


def test_every_output_word_is_the_word_of_the_knobs_off_build(outputs):
    differ = []
    for which in ("product", "allon"):
        for case in cases():
            a, b = outputs[which][case][0], outputs["knobs0"][case][0]
            assert len(a) == len(b) == out_bytes(case[0], case[1])
            if a != b:
                wa, wb = np.frombuffer(a, dtype=np.uint32), np.frombuffer(b, dtype=np.uint32)
                differ.append((which, case, int((wa != wb).sum()), int(np.flatnonzero(wa != wb)[0])))
    print("%d cases, %d output bytes per library; cases that differ (case, words, first word): %s"
          % (len(cases()), sum(len(v[0]) for v in outputs["product"].values()), differ))
    assert not differ, differ
    assert all(np.frombuffer(v[0], dtype=np.float32).any() for v in outputs["product"].values())


def test_both_history_halves_are_those_of_the_knobs_off_build(outputs):
    """... and they are what they must be: after three calls the half the next call reads holds the tail of the third call's
    input, the other one the tail of the second's"""
    differ = []
    for case in cases():
        Cn, nb = case[0], case[1]
        a, b = outputs["product"][case][1], outputs["knobs0"][case][1]
        assert len(a) == len(b) == hist_bytes(Cn)
        if a != b:
            differ.append(case)
        if outputs["allon"][case][1] != b:
            differ.append(("allon",) + case)
        x = noise(Cn, nb)
        hist = np.frombuffer(a, dtype=np.complex64).reshape(2, Cn, HOP)
        cur = CALLS % 2
        if not (hist[cur].tobytes() == x[CALLS - 1][:, -HOP:].tobytes() and hist[cur ^ 1].tobytes() == x[CALLS - 2][:, -HOP:].tobytes()):
            differ.append(("not the input's tail",) + case)
    print("history halves that differ: %s" % differ)
    assert not differ, differ


def test_how_the_runs_are_cut_changes_no_word(outputs):
    """the same call as one workgroup per block and as one run: the same words (product library)"""
    for Cn, nb, bpw, on_device in cases():
        if bpw != 0:
            assert outputs["product"][(Cn, nb, bpw, on_device)] == outputs["product"][(Cn, nb, 0, on_device)], (Cn, nb, bpw, on_device)


_ref = {}


def reference(oracle, Cn, nb):
    """fp64 oracle on the calls of (Cn, nb), [channel, sample of all calls]: computed once, read-only"""
    if (Cn, nb) not in _ref:
        x = noise(Cn, nb)
        rows = []
        for c in range(Cn):
            ff = oracle.CFastFIR(N)
            assert ff.SetupParameters(*FILTERS[c % 3]) == 1
            rows.append(np.concatenate([ff.ProcessData(x[call, c].astype(np.complex128)) for call in range(CALLS)]))
        _ref[(Cn, nb)] = np.stack(rows)
        _ref[(Cn, nb)].setflags(write=False)
    return _ref[(Cn, nb)]


@pytest.mark.parametrize("Cn", [3, 8])
@pytest.mark.parametrize("nb", [1, 2, 3, 8])
def test_product_words_match_the_oracle(oracle, outputs, Cn, nb):
    ref, peak = reference(oracle, Cn, nb), np.abs(noise(Cn, nb)).max()
    for bpw in (0, nb):
        for on_device in (False, True):
            y = np.frombuffer(outputs["product"][(Cn, nb, bpw, on_device)][0], dtype=np.complex64).reshape(CALLS, Cn, nb * HOP)
            got = np.concatenate(list(y), axis=1)
            err = np.abs(got - ref).max(axis=1) / peak
            print("%d channels x %d blocks, blocks_per_wg=%d, %s design: max err / max|x| per channel %s (bound %.3g)"
                  % (Cn, nb, bpw, "device" if on_device else "host", err, TOL))
            assert (err <= TOL).all(), (Cn, nb, bpw, on_device, err)
