"""CPU tests of the batch NCO-spur calibration's host logic (no GPU): spurcal_host.hpp's put rule and command function --
the very functions K13 evaluates on the device, through the csdr__host_spurcal_* hooks -- against the literal per-call
loop of tests/spurcal_ref.py (reference interface/sdrinterface.cpp:791-848, :886-887), the two hand-checked endings, and
the refusals that need no device."""
import ctypes as C
import pytest
from spurcal_ref import RefSpurCal, SPUR_CAL_MAXSAMPLES

PER = {1444: 240, 1028: 256}


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_spurcal_put.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.csdr__host_spurcal_put.restype = None
    lib.csdr__host_spurcal_command.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.csdr__host_spurcal_command.restype = None
    return lib


def put(L, count, active, n, call_len):
    """-> (calls that ran the recurrence, samples they cover, count, active)"""
    o = (C.c_int * 4)()
    L.csdr__host_spurcal_put(count, int(active), n, call_len, o)
    return o[0], o[1], o[2], bool(o[3])


def literal(count, active, n, call_len):
    r = RefSpurCal()
    r.count, r.active = count, active
    left = n
    while left > 0:
        m = min(call_len, left)
        r.call(m)
        left -= m
    return r.ran, min(r.ran * call_len, n), r.count, r.active


def command(L, cmd, off, count, active, vi=0.0, vq=0.0):
    o = (C.c_double * 2)(*off)
    c, a = C.c_int(count), C.c_int(int(active))
    L.csdr__host_spurcal_command(cmd, vi, vq, o, C.byref(c), C.byref(a))
    return [o[0], o[1]], c.value, bool(a.value)


@pytest.mark.parametrize("pkt_len", [1444, 1028])
@pytest.mark.parametrize("c0", [0, 1, SPUR_CAL_MAXSAMPLES - 1000, SPUR_CAL_MAXSAMPLES - 129, SPUR_CAL_MAXSAMPLES - 128,
                                SPUR_CAL_MAXSAMPLES - 120, SPUR_CAL_MAXSAMPLES - 1, SPUR_CAL_MAXSAMPLES,
                                SPUR_CAL_MAXSAMPLES + 32, SPUR_CAL_MAXSAMPLES + 5000])
def test_put_rule_matches_the_per_datagram_loop(L, pkt_len, c0):
    per = PER[pkt_len]
    for npk in (0, 1, 2, 3, 7, 8, 9, 10, 31, 2343, 2344, 2345, 2499, 2500, 2501, 2600):
        for active in (True, False):
            assert put(L, c0, active, npk * per, per) == literal(c0, active, npk * per, per), (npk, active)


def test_the_two_endings_by_hand(L):
    # 24 bit: 300000 / 120 = 2500 datagrams end on the limit exactly
    assert put(L, 0, True, 2500 * 240, 240) == (2500, 600000, 300000, True)       # ends WITH the put: still active
    assert put(L, 0, True, 2501 * 240, 240) == (2500, 600000, 300000, False)      # ends INSIDE it: the next datagram clears
    assert put(L, 300000, True, 240, 240) == (0, 0, 300000, False)                # ... or the next put's first one
    assert put(L, 300000, True, 0, 240) == (0, 0, 300000, True)                   # (an empty put has no datagram)
    # 16 bit: 300000 / 128 = 2343.75, so datagram 2343 still runs (299904 < 300000) and the count overshoots
    assert put(L, 0, True, 2343 * 256, 256) == (2343, 2343 * 256, 299904, True)
    assert put(L, 0, True, 2344 * 256, 256) == (2344, 2344 * 256, 300032, True)
    assert put(L, 0, True, 2600 * 256, 256) == (2344, 2344 * 256, 300032, False)
    assert put(L, 0, False, 2600 * 256, 256) == (0, 0, 0, False)


@pytest.mark.parametrize("call_len", [1, 2, 3, 100, 240, 255, 256, 1000])
def test_row_form_with_a_short_last_call(L, call_len):
    for c0 in (0, 7, SPUR_CAL_MAXSAMPLES - 260, SPUR_CAL_MAXSAMPLES - 1, SPUR_CAL_MAXSAMPLES):
        for n in (0, 1, 2, 3, call_len - 1, call_len, call_len + 1, 2 * call_len + 1, 3 * call_len - 1, 5 * call_len + call_len // 2, 2051):
            if n >= 0:
                assert put(L, c0, True, n, call_len) == literal(c0, True, n, call_len), (c0, n)
    # by hand: calls of 100, 100 and 50 samples add 50, 50 and (2 * 50) / 4 = 25
    assert put(L, 0, True, 250, 100) == (3, 250, 125, True)
    assert put(L, 0, True, 203, 100) == (3, 203, 101, True)                       # (2 * 3) / 4 = 1


def test_commands(L):
    SET, STARTCAL, READ = 0, 1, 2
    for cmd in (SET, STARTCAL, READ):                                              # :793: every command clears active ...
        assert command(L, cmd, [1.0, 2.0], 77, True, 3.0, 4.0)[2] == (cmd == STARTCAL)   # ... and STARTCAL sets it again
    assert command(L, SET, [1.0, 2.0], 77, True, 50.0, -3.0) == ([50.0, -3.0], 77, False)
    assert command(L, READ, [1.0, 2.0], 77, True) == ([1.0, 2.0], 77, False)
    assert command(L, STARTCAL, [1.0, 2.0], 77, False) == ([1.0, 2.0], 0, True)
    # the clamp: strictly beyond +-10.0, each offset on its own
    for v, kept in ((10.0, True), (-10.0, True), (10.000000000000002, False), (-10.000000000000002, False),
                    (9.999999999999998, True), (150.0, False), (-150.0, False), (0.0, True)):
        assert command(L, STARTCAL, [v, 1.0], 5, False)[0] == [v if kept else 0.0, 1.0], v
        assert command(L, STARTCAL, [-2.0, v], 5, False)[0] == [-2.0, v if kept else 0.0], v
    assert command(L, STARTCAL, [50.0, -3.0], 5, False) == ([0.0, -3.0], 0, True)
    # ... as the literal text has it
    for off in ([50.0, -3.0], [10.0, -10.0], [-11.0, 11.0], [0.5, 9.0]):
        r = RefSpurCal(); r.set(*off); r.start_cal()
        assert command(L, STARTCAL, off, 123, False) == (r.off, r.count, r.active)


def test_entry_points_refuse_without_a_device_or_a_handle(L):
    from cutesdr_amd import _capi
    EINVAL = _capi.CSDR_EINVAL
    if L.csdr_device_count() == 0:
        assert not L.csdr_spurcal_batch_create(0, 4)
        assert b"no HIP device" in L.csdr_last_error()
        import cutesdr_amd
        with pytest.raises(_capi.CsdrError):
            cutesdr_amd.SpurCalBatch(2)
    assert not L.csdr_spurcal_batch_create(0, 0)
    buf = (C.c_ubyte * 4096)()
    p = C.addressof(buf)
    assert L.csdr_spurcal_batch_put_packets(None, p, 2, 1444, None) == EINVAL
    assert L.csdr_spurcal_batch_put_stream(None, p, 8, 8, 4, None) == EINVAL
    assert L.csdr_spurcal_batch_put_packets_blanked(None, None, p, 2, 1444, None) == EINVAL
    assert L.csdr_spurcal_batch_put_stream_blanked(None, None, p, 8, 8, 4, None) == EINVAL
    assert L.csdr_spurcal_batch_set(None, 0, 0.0, 0.0) == EINVAL
    assert L.csdr_spurcal_batch_start_cal(None, -1) == EINVAL
    assert L.csdr_spurcal_batch_read(None, 0, None, None) == EINVAL
    assert L.csdr_spurcal_batch_get_state(None, 0, None, None, None, None) == EINVAL
    assert not L.csdr_spurcal_batch_dc(None)
    L.csdr_spurcal_batch_destroy(None)
