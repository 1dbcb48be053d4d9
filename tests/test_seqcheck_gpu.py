"""The batch datagram sequence check (csdr_seqcheck_batch, K12) against the sequential restatement in seq_ref.py (pinned
to the reference's text by its anchors, tests/test_seqcheck_host.py).  Every comparison is on integers and exact.
Five receivers carry five different streams, so a kernel that mixes rows, drops the carried state or takes datagram 0's
neighbour from another receiver fails; the datagrams' payload is random bytes, so a wrong byte offset reads noise."""
import ctypes as C

import numpy as np
import pytest

import seq_ref as R

pytestmark = pytest.mark.gpu

NPACKETS = [1, 2, 63, 64, 65, 255, 256, 257, 300]         # the lane, wave and workgroup edges
EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def pinned():
    R.check_anchors()                                     # the yardstick first


def with_gaps(start, n, gaps):
    """n numbers from `start`, datagram p preceded by gaps[p] lost ones"""
    out, s = [], start
    for p in range(n):
        for _ in range(gaps.get(p, 0) + 1):
            v = s
            s = (s + 1) & 0xffff or 1
        out.append(v)
    return out


def five_streams(n, calls, seed):
    """[5][n * calls] sequence numbers for `calls` puts of n datagrams each:
    0 clean from 0; 1 clean across 65535 -> 1; 2 gaps of 1-3 at seeded places and at datagram 0 and the last datagram of
    every call; 3 duplicates and swaps across 0x7fff/0x8000; 4 a restart (seq == 0) in the middle of a call"""
    rng = np.random.default_rng(seed)
    N = n * calls
    s0 = R.clean(0, N)
    s1 = R.clean(65536 - max(1, N // 2), N)
    gaps = {int(p): int(rng.integers(1, 4)) for p in rng.integers(0, N, max(1, N // 16))}
    for k in range(calls):
        gaps[k * n] = 1 + k % 3
        gaps[k * n + n - 1] = 3 - k % 3
    s2 = with_gaps(5, N, gaps)
    s3 = R.clean((0x8000 - N // 2) & 0xffff or 1, N)
    if N >= 2:
        i = s3.index(0x8000)
        s3[i - 1], s3[i] = s3[i], s3[i - 1]                # 0x8000 before 0x7fff
        if i + 1 < N:
            s3[i + 1] = s3[i]                              # ... and 0x7fff twice
        away = [int(j) for j in rng.integers(1, N, max(2, N // 10)) if abs(int(j) - i) > 2]      # the crossing stays as made
        for j in away[::2]:
            s3[j] = s3[j - 1]                              # duplicates
        for j in away[1::2]:
            s3[j - 1], s3[j] = s3[j], s3[j - 1]            # swaps
    s4 = R.clean(1000, N)
    mid = (calls - 1) * n + n // 2
    s4[mid:] = R.clean(0, N - mid)
    streams = [s0, s1, s2, s3, s4]
    assert all(len(s) == N for s in streams)
    return streams, rng


def buffer_of(streams, lo, hi, pkt_len, rng):
    return np.stack([R.datagrams(s[lo:hi], pkt_len, rng) for s in streams])


def state(sq, c):
    """(last, missed, events, first_gap) as seq_ref.walk returns them"""
    m, e, g, l = sq.get(c)
    return l, m, e, g


def test_the_streams_are_what_they_claim():
    streams, _ = five_streams(300, 1, 1)
    assert R.walk(streams[0])[1:] == (0, 0, -1)
    assert 65535 in streams[1] and R.walk(streams[1], last=streams[1][0])[1:] == (0, 0, -1)
    w2 = R.walk(streams[2])
    assert w2[2] >= 10 and w2[3] == 0 and w2[1] > w2[2]   # datagram 0 is a gap; some gaps are wider than one
    assert R.walk(streams[2][299:], *R.walk(streams[2][:299])[:3])[3] == 0      # ... and so is the last one
    i = streams[3].index(0x8000)
    assert streams[3][i + 1] == 0x7fff and R.walk(streams[3])[2] >= 10
    assert 0 in streams[4][100:200]
    assert abs(R.walk(streams[3])[1]) >= 65535 - 300       # the qint16 casts matter to what is compared


@pytest.mark.parametrize("pkt_len", [1028, 1444])
@pytest.mark.parametrize("n", NPACKETS)
def test_batch_equals_the_sequential_walk(n, pkt_len):
    import cutesdr_amd as ca
    streams, rng = five_streams(n, 2, 1000 * n + pkt_len)
    sq = ca.SeqCheckBatch(5)
    want = [(0, 0, 0, -1)] * 5
    assert [state(sq, c) for c in range(5)] == want       # a new object
    for call in range(2):                                 # the second put starts from the carried state
        sq.put(buffer_of(streams, call * n, (call + 1) * n, pkt_len, rng))
        want = [R.walk(streams[c][call * n:(call + 1) * n], *want[c][:3]) for c in range(5)]
        for c in range(5):
            assert state(sq, c) == want[c], (call, c)
    for c in range(5):
        assert want[c][:3] == R.walk(streams[c])[:3]


@pytest.mark.parametrize("cuts", [(100, 199), (101, 200), (99, 201)], ids=["at-and-before", "after-and-at", "before-and-after"])
def test_several_puts_equal_one_put(cuts):
    """gaps at datagrams 100 and 200 of every receiver's 300: a cut at a gap makes it datagram 0 of the next put, a cut just
    after one its put's last datagram, a cut just before one datagram 1"""
    import cutesdr_amd as ca
    pkt_len = 1444
    rng = np.random.default_rng(5)
    streams = [with_gaps(start, 300, {100: 1 + c % 3, 200: 3 - c % 3}) for c, start in enumerate((0, 65300, 32600, 7, 40000))]
    one, many = ca.SeqCheckBatch(5), ca.SeqCheckBatch(5)
    one.put(buffer_of(streams, 0, 300, pkt_len, rng))
    want = [(0, 0, 0, -1)] * 5
    for lo, hi in zip((0,) + cuts, cuts + (300,)):
        many.put(buffer_of(streams, lo, hi, pkt_len, rng))
        want = [R.walk(streams[c][lo:hi], *want[c][:3]) for c in range(5)]
        for c in range(5):
            assert state(many, c) == want[c], (lo, c)      # first_gap is this put's
    for c in range(5):
        whole = R.walk(streams[c])
        assert state(one, c) == whole and state(many, c)[:3] == whole[:3], c
        assert whole[2] == (3 if c else 2)                 # (but for receiver 0, which starts at 0, datagram 0 is an event of its own)


def test_clear_and_reset_between_puts():
    import cutesdr_amd as ca
    pkt_len, n = 1028, 70
    streams, rng = five_streams(n, 3, 9)
    bufs = [buffer_of(streams, k * n, (k + 1) * n, pkt_len, rng) for k in range(3)]
    sq = ca.SeqCheckBatch(5)
    sq.put(bufs[0])
    w = [R.walk(streams[c][:n]) for c in range(5)]
    assert sum(x[2] for x in w) > 0
    sq.clear(2)                                           # one receiver: missed, events <- 0, last kept, the others untouched
    w[2] = (w[2][0], 0, 0, w[2][3])
    assert [state(sq, c) for c in range(5)] == w
    sq.put(bufs[1])
    w = [R.walk(streams[c][n:2 * n], *w[c][:3]) for c in range(5)]
    assert [state(sq, c) for c in range(5)] == w
    sq.reset(3)                                           # one receiver: last <- 0 too
    w[3] = (0, 0, 0, w[3][3])
    assert [state(sq, c) for c in range(5)] == w
    sq.clear()                                            # all
    w = [(x[0], 0, 0, x[3]) for x in w]
    assert [state(sq, c) for c in range(5)] == w
    sq.put(bufs[2])
    w = [R.walk(streams[c][2 * n:], *w[c][:3]) for c in range(5)]
    assert [state(sq, c) for c in range(5)] == w
    assert w[3][2] > 0                                    # receiver 3 was judged from last = 0
    sq.reset()                                            # all
    assert [state(sq, c)[:3] for c in range(5)] == [(0, 0, 0)] * 5


def test_clear_is_ordered_between_puts_without_a_host_wait():
    """put, clear, put issued back to back on the device pointer form (nothing waits in between): the result is the
    second put's from the cleared counts and the first put's last"""
    import cutesdr_amd as ca
    pkt_len, n = 1444, 300
    streams, rng = five_streams(n, 2, 11)
    bufs = [buffer_of(streams, k * n, (k + 1) * n, pkt_len, rng) for k in range(2)]
    dps = []
    for b in bufs:
        dp = ca.DeviceBuffer(b.nbytes); dp.upload(b); dps.append(dp)
    ca.sync()
    sq = ca.SeqCheckBatch(5)
    sq.put(dps[0].ptr, n, pkt_len)
    sq.clear()
    sq.put(dps[1].ptr, n, pkt_len)
    for c in range(5):
        last = R.walk(streams[c][:n])[0]
        assert state(sq, c) == R.walk(streams[c][n:], last, 0, 0), c
    ca.sync()


def test_get_all_and_refused_calls():
    import cutesdr_amd as ca
    L = ca.lib()
    pkt_len, n = 1444, 65
    streams, rng = five_streams(n, 1, 13)
    raw = buffer_of(streams, 0, n, pkt_len, rng)
    dp = ca.DeviceBuffer(raw.nbytes + 8); dp.upload(raw)
    sq = ca.SeqCheckBatch(5)
    sq.put(dp.ptr, n, pkt_len)
    before = [state(sq, c) for c in range(5)]
    assert before == [R.walk(s) for s in streams]
    missed, events, first_gap = sq.get_all()
    assert missed.dtype == np.int64 and events.dtype == np.int64 and first_gap.dtype == np.int32
    assert [(int(m), int(e), int(g)) for m, e, g in zip(missed, events, first_gap)] == [x[1:] for x in before]
    d = ca.DeviceBuffer(4 * 5)                            # any pointer may be NULL
    sq.get_all_ptr(None, None, d.ptr)
    ca.sync()
    assert list(d.download(np.int32, 5)) == [x[3] for x in before]
    put = L.csdr_seqcheck_batch_put
    assert put(sq.h, C.c_void_p(dp.ptr), n, 1024, None) == EINVAL              # no such datagram
    assert put(sq.h, C.c_void_p(dp.ptr), n, 1440, None) == EINVAL
    assert put(sq.h, C.c_void_p(dp.ptr + 1), n, pkt_len, None) == EINVAL       # misaligned
    assert put(sq.h, C.c_void_p(dp.ptr + 2), n, pkt_len, None) == EINVAL
    assert put(sq.h, C.c_void_p(dp.ptr), -1, pkt_len, None) == EINVAL
    assert put(sq.h, None, n, pkt_len, None) == EINVAL
    assert put(sq.h, C.c_void_p(dp.ptr), (1 << 31) // 1444 + 1, pkt_len, None) == EINVAL      # 2 GiB per receiver
    assert L.csdr_seqcheck_batch_clear(sq.h, 5) == EINVAL and L.csdr_seqcheck_batch_reset(sq.h, 5) == EINVAL
    assert L.csdr_seqcheck_batch_get(sq.h, 5, None, None, None, None) == EINVAL
    assert L.csdr_seqcheck_batch_get(sq.h, -1, None, None, None, None) == EINVAL
    assert [state(sq, c) for c in range(5)] == before
    assert put(sq.h, C.c_void_p(dp.ptr), 0, pkt_len, None) == 0                # nothing, first_gap included
    assert [state(sq, c) for c in range(5)] == before
    assert L.csdr_seqcheck_batch_get(sq.h, 0, None, None, None, None) == 0


def test_the_chain_is_not_touched():
    """one process_packets call gives the same words whether or not a put on the same buffer and stream precedes it"""
    import cutesdr_amd as ca
    from util_signals import fm_carrier, am_carrier, tones_plus_noise
    import test_frontend_gpu as F
    import test_postchain_gpu as T
    L = ca.lib()
    pkt_len, per, fs, Cn = 1444, 240, 2e6, 3
    npk = 19968 * 30 // per
    n = npk * per
    sig = [fm_carrier(n, fs, 100e3, dbfs=-20.0), am_carrier(n, fs, 101e3, dbfs=-20.0, channel=1),
           tones_plus_noise(12, n, fs, [102e3, 102e3 + 300.0])]
    raw = np.stack([F._pack24(x) for x in sig])
    rng = np.random.default_rng(3)
    seqs = [with_gaps(start, npk, {int(p): 1 for p in rng.integers(0, npk, 9)}) for start in (0, 65000, 32000)]
    for c in range(Cn):                                   # real headers: bytes 0-1 anything, 2-3 the number
        raw[c, :, 0:2] = rng.integers(0, 256, (npk, 2), dtype=np.uint8)
        raw[c, :, 2] = np.asarray(seqs[c]) & 0xff
        raw[c, :, 3] = np.asarray(seqs[c]) >> 8
    dp = ca.DeviceBuffer(raw.nbytes); dp.upload(raw)
    cap = n // 8
    outs = []
    for with_put in (False, True):
        b = ca.DemodBatch(Cn, 2048); b.set_input_rate(fs)
        for c, name in enumerate(("FM", "AM", "CWU")):
            m, kw = T.MODES[name]
            b.set_demod(c, m, T.info(ca, **kw))
        b.commit()
        for c in range(Cn):
            b.set_freq(c, -(100e3 + 1e3 * c))
        dout = ca.DeviceBuffer(4 * Cn * cap)
        ca.sync()
        if with_put:
            sq = ca.SeqCheckBatch(Cn)
            sq.put(dp.ptr, npk, pkt_len)
        assert L.csdr_demod_batch_process_packets(b.h, C.c_void_p(dp.ptr), npk, pkt_len, None, C.c_void_p(dout.ptr), cap, None) == 0
        b.flush()
        ca.sync()
        y = dout.download(np.float32, Cn * cap).reshape(Cn, cap)
        outs.append([y[c, :b.out_count(c)].copy() for c in range(Cn)])
        if with_put:
            assert [state(sq, c) for c in range(Cn)] == [R.walk(s) for s in seqs]
    for c in range(Cn):
        assert len(outs[0][c]) > 0 or c == 2
        assert np.array_equal(outs[0][c].view(np.uint32), outs[1][c].view(np.uint32)), c
    assert sum(len(x) for x in outs[0]) > 0
