"""CPU tests of the noise blanker's HOST-side logic (nb_host.hpp, no GPU): the rule that cuts a call into segments and
the choice among the kernel's forms, each against a restatement of what the host code did before the two became pure
functions."""
import ctypes as C
import itertools
import numpy as np
import pytest

SAMPLES, SAMPLES_RING, MASK, MASK_RING, MASK_INT24, MASK_INT16 = range(6)      # NbForm


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_nb_geometry.argtypes = [C.c_int] + [C.c_void_p] * 3
    lib.csdr__host_nb_geometry.restype = None
    lib.csdr__host_nb_segments.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.csdr__host_nb_segments.restype = None
    lib.csdr__host_nb_form.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 2
    return lib


def geometry(L, mask):
    t, lo, hi = C.c_int(), C.c_int(), C.c_int()
    L.csdr__host_nb_geometry(mask, C.byref(t), C.byref(lo), C.byref(hi))
    return t.value, lo.value, hi.value


def test_geometry(L):
    """512 threads x 4 samples, x 8 in the ring's mask form; a ring of 16384 magnitudes, the window at least one tile
    and at most the ring less one tile"""
    assert geometry(L, 0) == (2048, 2048, 14336)
    assert geometry(L, 1) == (4096, 4096, 12288)


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("mask", [0, 1])
def test_segment_rule(L, mask, ring):
    tile = geometry(L, mask)[0]
    want = 512 if ring else (3072 if mask else 2048)          # workgroups wanted per launch
    chans = [1, 2, 5, 256, 600]
    ns = [1, tile - 1, tile, 32 * tile, 64 * tile - 1, 64 * tile, 64 * tile + 1, 1 << 21, 240 * 8739]
    grid = np.array(list(itertools.product(chans, ns)), dtype=np.int64)
    ch, n = grid[:, 0], grid[:, 1]
    # the rule as the host wrote it out before: enough segments for the wanted workgroups, none shorter than 32 tiles,
    # equal lengths rounded up to whole tiles
    nseg = np.maximum(np.minimum((want + ch - 1) // ch, n // (32 * tile)), 1)
    seg_len = -(-(-(-n // nseg)) // tile) * tile
    expect = np.stack([-(-n // seg_len), seg_len], axis=1)
    for (c, k), (e_nseg, e_len) in zip(grid, expect):
        a, b = C.c_int(), C.c_int()
        L.csdr__host_nb_segments(int(k), int(c), mask, ring, C.byref(a), C.byref(b))
        nseg_, len_ = a.value, b.value
        assert len_ > 0 and len_ % tile == 0, (c, k)
        assert nseg_ * len_ >= k > (nseg_ - 1) * len_, (c, k)
        assert nseg_ == 1 or len_ >= 32 * tile, (c, k)
        assert c * nseg_ <= want + c - 1, (c, k)
        assert (nseg_, len_) == (e_nseg, e_len), (c, k)


# channel sets: (on, mag_n, integral) per channel -> (every `on` channel inside the ring limits, every `on` channel integral).
# mag_n + 1 = 10001 fits the ring of either form; 30001 fits neither
INSIDE, OUTSIDE = 10000, 30000
CHANNEL_SETS = {
    "all inside, integral": ([(1, INSIDE, 1)] * 3, True, True),
    "one outside the ring limits": ([(1, INSIDE, 1), (1, OUTSIDE, 1), (1, INSIDE, 1)], False, True),
    "one non-integral channel that is on": ([(1, INSIDE, 1), (1, INSIDE, 0), (1, INSIDE, 1)], True, False),
    "an off channel, outside and non-integral": ([(1, INSIDE, 1), (0, OUTSIDE, 0), (1, INSIDE, 1)], True, True),
    "outside and non-integral": ([(1, OUTSIDE, 0)], False, False),
    "every channel off": ([(0, OUTSIDE, 0)] * 2, True, True),
}
# (mask, source, ring, integral) -> form; source 0 = float rows; ring / integral: eligible and switched on.
# Samples out: the ring is all that matters.  Mask out: the integer kernels take datagrams with the ring and an integral state.
FORM = {}
for src, integral in itertools.product((0, 1028, 1444), (False, True)):
    FORM[0, src, False, integral] = SAMPLES
    FORM[0, src, True, integral] = SAMPLES_RING
    FORM[1, src, False, integral] = MASK
FORM.update({(1, 0, True, False): MASK_RING, (1, 0, True, True): MASK_RING,
             (1, 1028, True, False): MASK_RING, (1, 1028, True, True): MASK_INT16,
             (1, 1444, True, False): MASK_RING, (1, 1444, True, True): MASK_INT24})


@pytest.mark.parametrize("name", list(CHANNEL_SETS))
def test_choice_of_form(L, name):
    chans, ring_ok, integral_ok = CHANNEL_SETS[name]
    on, mag_n, integral = (np.array(v, dtype=np.int32) for v in zip(*chans))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for mask, src, ring_sw, int_sw in itertools.product((0, 1), (0, 1028, 1444), (0, 1), (0, 1)):
        got = L.csdr__host_nb_form(mask, src, len(chans), vp(on), vp(mag_n), vp(integral), ring_sw, int_sw)
        assert got == FORM[mask, src, bool(ring_sw and ring_ok), bool(int_sw and integral_ok)], (mask, src, ring_sw, int_sw)


@pytest.mark.parametrize("mask", [0, 1])
def test_ring_limits_are_inclusive(L, mask):
    _, lo, hi = geometry(L, mask)
    ring_form = MASK_RING if mask else SAMPLES_RING
    one = np.ones(1, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for m1, inside in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
        got = L.csdr__host_nb_form(mask, 0, 1, vp(one), vp(np.array([m1 - 1], dtype=np.int32)), vp(one), 1, 1)
        assert (got == ring_form) == inside, m1
