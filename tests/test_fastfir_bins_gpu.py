"""GPU parity of the overlap-save kernels (K1) bin by bin, against the fp64 oracle, on the flat periodic probe of
tests/k1_bins.py (the instrument is proved in tests/test_fastfir_bins_host.py).

Rule: on every steady window of every channel, B <= m B_y and T <= m T_y (m = 4; 6.43 for the generic kernel at 16384
points, whose twiddle powers by products cost a factor of three: k1_bins.MARGINS), where B is the largest error of one bin's
effective multiplier and T the largest error of one sample, both relative to the peak gain, and (B_y, T_y) the same
figures of scipy's fp32 transform pair on the same filter and the same probe.  The rule the other K1 tests keep,
|err| <= 2e-5 max|x|, passes a single bin that is 0.3 to 0.8 % off; this one resolves 1e-5.

Every channel has a probe seed of its own and filter FILTERS[c % 5]; the wide one (98 % of the bins in the pass band) is
the one that sees the forward passes of every bin.  A stream is four periods = eight hops, cut into calls in three
ways; windows 1, 2 and 3 of every channel are checked, every bin of each.  Which kernel a launch took is asserted
through csdr__fastfir_last_kernel after every call.  Every comparison prints
    K1BINS n kernel C cut window channel: B, B/B_y, T, T/T_y
before it asserts."""
import ctypes as C
import numpy as np
import pytest
import k1_bins as kb

pytestmark = pytest.mark.gpu
GENERIC, PIPELINED_H, PIPELINED_GAIN = 0, 1, 2          # FastFirKernel, fastfir_kernels.h
# (size, name) -> (variant, own_design, the kernel its launches must take): below 16384 points there are no gains, the
# pipelined build runs on complex H
FORMS = {}
for _n in kb.SIZES:
    FORMS[(_n, "generic")] = (0, True, GENERIC)
    FORMS[(_n, "pipelined")] = (2, True, PIPELINED_GAIN if _n == 16384 else PIPELINED_H)
FORMS[(16384, "complex_h")] = (2, False, PIPELINED_H)
FORM_IDS = ["%d-%s" % f for f in FORMS]
DEVICE_FORMS = [f for f in FORMS if f[0] in (16384, 4096)]          # the sizes whose responses are also designed on the device here
# hops per call, blocks_per_wg: one call; a single block, a pair and an odd run; runs of three with a tail of two
CUTS = {"8": ((8,), 0), "1+2+5": ((1, 2, 5), 0), "3+5/bpw3": ((3, 5), 3)}


def lib():
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__fastfir_set_variant.restype = C.c_int
    L.csdr__fastfir_set_variant.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_set_own_design.restype = C.c_int
    L.csdr__fastfir_set_own_design.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_last_kernel.restype = C.c_int
    L.csdr__fastfir_last_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def last_kernel(b):
    k, tw = C.c_int(-2), C.c_int(-2)
    assert lib().csdr__fastfir_last_kernel(b.h, C.byref(k), C.byref(tw)) == 0
    return k.value


def filter_of(c, shared):
    return kb.WIDE if shared else kb.FILTERS[c % len(kb.FILTERS)]


_refs = {}


def reference(oracle, n, Cn, shared=False):
    """(x [Cn, 4n] complex64, ref [Cn, 4n] fp64, yardsticks [(B_y, T_y)] per channel), once per (n, channel count, filters)"""
    key = (n, Cn, shared)
    if key not in _refs:
        x = np.stack([kb.stream(n, 1000 * (n // 2048) + 10 * Cn + c) for c in range(Cn)])
        ref = np.stack([kb.oracle_reference(oracle, n, x[c], filter_of(c, shared)) for c in range(Cn)])
        yard = [kb.yardstick(ref[c], x[c], n) for c in range(Cn)]
        x.setflags(write=False); ref.setflags(write=False)
        _refs[key] = (x, ref, yard)
    return _refs[key]


def make(n, Cn, form, design):
    """design: "host" (setup per channel), "device" (setup_many) or "shared" (one wide filter for every channel, h_stride 0)"""
    import cutesdr_amd as ca
    variant, own, _ = FORMS[(n, form)]
    b = ca.FastFirBatch(Cn, n)
    if design == "shared":
        assert b.setup(*kb.WIDE) == 1
    elif design == "device":
        assert b.setup(-1000, 1000, 0, 48000.0, channel=0) == 1          # (per-channel filters first: the one call that reallocates)
        flt = [filter_of(c, False) for c in range(Cn)]
        st = b.setup_many(list(range(Cn)), [f[0] for f in flt], [f[1] for f in flt], [f[2] for f in flt], [f[3] for f in flt])
        assert (st == 1).all(), st
    else:
        for c in range(Cn):
            assert b.setup(*filter_of(c, False), channel=c) == 1
    assert lib().csdr__fastfir_set_variant(b.h, variant) == 0
    if not own:
        assert lib().csdr__fastfir_set_own_design(b.h, 0) == 0
    return b


def run(b, x, n, cut, kernel):
    (calls, bpw), hop = CUTS[cut], n // 2
    assert sum(calls) * hop == x.shape[1] and last_kernel(b) == -1
    parts, at = [], 0
    for k in calls:
        parts.append(b.process(x[:, at * hop:(at + k) * hop], blocks_per_wg=bpw))
        assert last_kernel(b) == kernel, (cut, at, last_kernel(b))
        at += k
    y = np.concatenate(parts, axis=1)
    assert y.dtype == np.complex64
    return y


def check(tag, y, x, ref, yard, n, m, windows=kb.WINDOWS):
    """every channel, every window, every bin: print the figures, then hold all of them to the margin m"""
    assert y.shape == ref.shape
    bad = []
    for c in range(len(ref)):
        By, Ty = yard[c]
        for w in windows:
            B, T = kb.figures(y[c], ref[c], x[c], n, w)
            print("K1BINS %s %d %d: %.3g, %.2f, %.3g, %.2f" % (tag, w, c, B, B / By, T, T / Ty))
            if not (B <= m * By and T <= m * Ty):
                bad.append((w, c, B / By, T / Ty))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("Cn", [5, 8])
@pytest.mark.parametrize("n,form", list(FORMS), ids=FORM_IDS)
def test_every_bin_of_every_channel_host_design(oracle, n, form, Cn, cut):
    x, ref, yard = reference(oracle, n, Cn)
    b = make(n, Cn, form, "host")
    kernel = FORMS[(n, form)][2]
    y = run(b, x, n, cut, kernel)
    b.close()
    check("%d %s %d %s" % (n, form, Cn, cut), y, x, ref, yard, n, kb.margin(n, kernel))


@pytest.mark.parametrize("Cn", [5, 8])
@pytest.mark.parametrize("n,form", DEVICE_FORMS, ids=["%d-%s" % f for f in DEVICE_FORMS])
def test_every_bin_of_every_channel_device_design(oracle, n, form, Cn):
    """the responses (and at 16384 points the gains) designed by the design kernel: same streams, same references"""
    x, ref, yard = reference(oracle, n, Cn)
    b = make(n, Cn, form, "device")
    kernel = FORMS[(n, form)][2]
    y = run(b, x, n, "1+2+5", kernel)
    b.close()
    check("%d %s/device %d 1+2+5" % (n, form, Cn), y, x, ref, yard, n, kb.margin(n, kernel))


@pytest.mark.parametrize("n", kb.SIZES)
def test_every_bin_shared_wide_filter(oracle, n):
    """one response for all channels (h_stride 0), the wide filter: every channel has nearly every bin in the pass band"""
    Cn = 5
    x, ref, yard = reference(oracle, n, Cn, shared=True)
    for form in ("generic", "pipelined"):
        b = make(n, Cn, form, "shared")
        kernel = FORMS[(n, form)][2]
        y = run(b, x, n, "3+5/bpw3", kernel)
        b.close()
        check("%d %s/shared %d 3+5/bpw3" % (n, form, Cn), y, x, ref, yard, n, kb.margin(n, kernel))


@pytest.mark.parametrize("n,chunk", [(2048, 240), (16384, 19968)])
def test_every_bin_drop_in_cfastfir(oracle, n, chunk):
    """CFastFIR, the single-channel drop-in: ragged calls, the wide filter, window 1"""
    import cutesdr_amd as ca
    x = kb.stream(n, 77 + n)
    ref = kb.oracle_reference(oracle, n, x, kb.WIDE)
    ff = ca.CFastFIR(n)
    assert ff.SetupParameters(*kb.WIDE) == 1
    got = np.concatenate([ff.ProcessData(x[i:i + chunk]) for i in range(0, len(x), chunk)])
    ff.close()
    assert len(got) == len(x)
    check("%d cfastfir 1 %d" % (n, chunk), got[None], x[None], ref[None], [kb.yardstick(ref, x, n)], n, kb.MARGIN, windows=(1,))
