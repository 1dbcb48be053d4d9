"""csdr_noiseproc_batch_trace_last (PROFILE_7, noiseproc.cpp:159-175) on the device against nbtrace_ref.py, the
line-for-line restatement that tests/test_nbtrace_host.py pins to the reference's compiled code.

Exact inputs.  Integers (24-bit datagrams: multiples of 2^-8) of +-200 with impulses up to +-32767, what datagrams
decode to: every fp64 sum of at most 32768 such magnitudes is exact in any order, so the trace must equal the
restatement's doubles rounded once to fp32 bit for bit, and the real part must be 0 exactly where it blanks.

Shapes.  Object A: four receivers whose windows all fit the LDS ring (500 kS/s / 100 us, 2 MS/s / 50 us, 2 MS/s / 2 us,
one switched off); object B: one receiver at 100 kS/s, whose 501-sample window is shorter than a tile and forces the
two-stream form.  Calls of 1, 7, 240, 4096, 3 * 65536 + 1000 (three segments: the later ones rebuild the window sum and
run a warm-up) and 513 samples, trace_last after each, twice.  The restatement runs the long call on receivers 0 and 1
of A and on B's only; A's receiver 2 is compared up to the long call, the switched-off one throughout."""
import ctypes as C
import functools
import numpy as np
import pytest

import nbtrace_ref as N

pytestmark = pytest.mark.gpu

LONG = 3 * 65536 + 1000
# (on, sample rate, threshold, width us)
OBJ_A = [(True, 500e3, 20.0, 100.0), (True, 2e6, 20.0, 50.0), (True, 2e6, 20.0, 2.0), (False, 500e3, 20.0, 100.0)]
OBJ_B = [(True, 100e3, 20.0, 50.0)]
# samples per call; the datagram forms in whole datagrams (256 / 240 samples), the fourth call again three segments
CALLS = {0: [1, 7, 240, 4096, LONG, 513], 1028: [256 * k for k in (1, 3, 16, 772, 2)], 1444: [240 * k for k in (1, 3, 17, 820, 2)]}
LONG_RX = {"A": (0, 1, 3), "B": (0,)}                    # receivers the restatement follows through the long call


def is_long(n):
    return n >= 3 * 65536


def stream(c, total, frac):
    """receiver c's samples: +-200 with impulses; one pair 10 samples apart inside the 240-sample call"""
    rng = np.random.default_rng(100 + c)
    x = N.datagram_like(total, 40 + c)
    hits = np.flatnonzero(rng.random(total) < 3e-4)
    x[hits] = rng.integers(-32767, 32768, len(hits)) + 1j * rng.integers(-32767, 32768, len(hits))
    for i, v in ((50, 32767 + 0j), (60, complex(0, -32767)), (4000, -32767 - 32767j), (65536 + 8 + 240 + 4096 - 3, 30000 + 1j), (2 * 65536 + 4400, 5 - 28000j)):
        if i < total:
            x[i] = v
    if frac:                                             # 24-bit datagrams resolve 2^-8
        x = x + (rng.integers(0, 256, total) + 1j * rng.integers(0, 256, total)) / 256.0
        x.real = np.clip(x.real, -32768, 32767.99609375); x.imag = np.clip(x.imag, -32768, 32767.99609375)
    return x


@functools.lru_cache(maxsize=None)
def reference(obj, form):
    """(x [receivers, total], per call {receiver: (out, trace fp32, blanked)}) of object A or B over CALLS[form]"""
    settings, calls = (OBJ_A if obj == "A" else OBJ_B), CALLS[form]
    x = np.stack([stream(c + (10 if obj == "B" else 0), sum(calls), form == 1444) for c in range(len(settings))])
    refs = []
    for on, fs, th, w in settings:
        r = N.RefNoiseProc(); r.SetupBlanker(on, th, w, fs); refs.append(r)
    out, pos, alive = [], 0, set(range(len(settings)))
    for n in calls:
        if is_long(n):
            alive &= set(LONG_RX[obj])
        res = {}
        for c in sorted(alive):
            o, tb, bl = refs[c].ProcessBlanker(x[c, pos:pos + n])
            res[c] = (o.astype(np.complex64), N.trace_fp32(tb), bl)
        out.append(res)
        pos += n
    x.setflags(write=False)
    return x, out


def internals():
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__noiseproc_batch_process_packets.restype = C.c_int
    L.csdr__noiseproc_batch_process_packets.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    return ca, L


def make_blanker(ca, settings):
    nb = ca.NoiseProcBatch(len(settings))
    for c, (on, fs, th, w) in enumerate(settings):
        nb.setup(on, th, w, fs, channel=c)
    return nb


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


PATTERN = np.float32(-12345.5)


class Trace:
    """a trace buffer [channels][stride] complex fp32 with a pattern behind every row's n samples"""

    def __init__(self, ca, channels, nmax):
        self.ca, self.ch, self.stride = ca, channels, (nmax + 3) & ~1
        self.buf = ca.DeviceBuffer(channels * self.stride * 8)
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.ch * self.stride * 2, PATTERN, dtype=np.float32))

    def get(self):
        self.ca.sync()
        return self.buf.download(np.complex64, self.ch * self.stride).reshape(self.ch, self.stride)

    def untouched(self):
        return (self.get().view(np.float32) == PATTERN).all()


def run_exact(obj, form):
    """the calls of CALLS[form] through csdr_noiseproc_batch_process (form 0) or the packets form, trace_last behind each
    call, twice; a twin object that never traces must write the same outputs, word for word"""
    from test_display_stream_gpu import make_packets
    ca, L = internals()
    settings = OBJ_A if obj == "A" else OBJ_B
    x, ref = reference(obj, form)
    Cn, per = len(settings), {0: 1, 1028: 256, 1444: 240}[form]
    nb, twin = make_blanker(ca, settings), make_blanker(ca, settings)
    nmax = max(CALLS[form])
    din = ca.DeviceBuffer(Cn * (nmax // per * form if form else nmax * 8))
    dout, dtwin = ca.DeviceBuffer(Cn * nmax * 8), ca.DeviceBuffer(Cn * nmax * 8)
    tr = Trace(ca, Cn, nmax)
    pos, blanked, shown = 0, 0, 0
    for k, n in enumerate(CALLS[form]):
        part = x[:, pos:pos + n]
        pos += n
        outs = []
        for b, do in ((nb, dout), (twin, dtwin)):
            if form:
                din.upload(make_packets(part, form))
                assert L.csdr__noiseproc_batch_process_packets(b.h, C.c_void_p(din.ptr), n // per, form, C.c_void_p(do.ptr), n, None) == 0
            else:
                din.upload(part.astype(np.complex64))
                b.process_ptr(din.ptr, n, n, do.ptr, n)
            ca.sync()
            outs.append(do.download(np.complex64, Cn * n).reshape(Cn, n))
            if b is nb:
                tr.fill()
                args = dict(d_packets=din.ptr, npackets=n // per, pkt_len=form) if form else dict(d_in=din.ptr, in_stride=n)
                assert nb.trace_last(tr.buf.ptr, tr.stride, n, **args) == 0
                got = tr.get()
                assert nb.trace_last(tr.buf.ptr, tr.stride, n, **args) == 0
                assert np.array_equal(words(tr.get()), words(got)), k                     # run twice: identical rows
        assert np.array_equal(words(outs[0]), words(outs[1])), k                         # the traced object's process = the twin's
        assert (got[:, n:].view(np.float32) == PATTERN).all(), k                         # nothing behind the n samples
        for c, (o, want, bl) in ref[k].items():
            assert np.array_equal(words(outs[0][c]), words(o)), (k, c)
            bad = np.flatnonzero(words(got[c, :n]).reshape(-1, 2) != words(want).reshape(-1, 2))
            assert len(bad) == 0, (k, c, bad[:8], got[c, bad[:4] // 2], want[bad[:4] // 2])
            if settings[c][0]:
                assert ((got[c, :n].real == 0.0) == bl).all(), (k, c)
                blanked += int(bl.sum()); shown += int((~bl).sum())
    return blanked, shown


@pytest.mark.parametrize("form", [0, 1028, 1444], ids=["rows", "pkt1028", "pkt1444"])
def test_ring_object_is_bit_exact(form):
    blanked, shown = run_exact("A", form)
    assert blanked > 1000 and shown > 100000, (blanked, shown)


@pytest.mark.parametrize("form", [0, 1444], ids=["rows", "pkt1444"])
def test_two_stream_object_is_bit_exact(form):
    blanked, shown = run_exact("B", form)
    assert blanked > 100 and shown > 100000, (blanked, shown)


# ---------------------------------------------------------------------------------------------------- behind a chain
def make_chain(ca, channels, fs):
    import test_postchain_gpu as T
    b = ca.DemodBatch(channels, 2048); b.set_input_rate(fs)
    m, kw = T.MODES["AM"]
    for c in range(channels):
        b.set_demod(c, m, T.info(ca, **kw))
    b.commit()
    for c in range(channels):
        b.set_freq(c, -100e3 - 1000.0 * c)
    return b


def chain_mask(L, b, channels, n):
    """the mask the chain's last blanked call left: bool [channels, n] (csdr__demod_batch_last_blank)"""
    import cutesdr_amd as ca
    blank = (C.c_longlong * 4)()                         # DcBlank: mask, mask_stride, state, hist
    call = (C.c_longlong * 4)()
    L.csdr__demod_batch_last_blank.restype = C.c_int
    L.csdr__demod_batch_last_blank.argtypes = [C.c_void_p] * 5
    assert L.csdr__demod_batch_last_blank(b.h, C.cast(blank, C.c_void_p), C.cast(call, C.c_void_p), None, None) == 0
    mask_ptr, stride = blank[0], blank[1]
    w = np.empty(channels * stride, dtype=np.uint32)
    assert L.csdr_dev_download(0, w.ctypes.data_as(C.c_void_p), C.c_void_p(mask_ptr), w.nbytes) == 0
    bits = np.unpackbits(w.reshape(channels, stride).view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


@pytest.mark.parametrize("form", [0, 1444], ids=["process_blanked", "process_packets"])
def test_behind_a_chains_mask_pass(form):
    """two receivers at 2 MS/s (50 and 2 us) in front of an AM chain, two calls: the trace equals the restatement bit for
    bit (integral input: every sum exact), and its real part is 0 exactly where the mask the call left has a set bit"""
    from test_display_stream_gpu import make_packets
    ca, L = internals()
    fs, Cn, per = 2e6, 2, (240 if form else 1)
    settings = [(True, fs, 20.0, 50.0), (True, fs, 20.0, 2.0)]
    n = 240 * 256                                        # a multiple of every decimation of the plan and of both datagram sizes
    x = np.stack([stream(20 + c, 2 * n, bool(form)) for c in range(Cn)])
    refs = []
    for on, f, th, w in settings:
        r = N.RefNoiseProc(); r.SetupBlanker(on, th, w, f); refs.append(r)
    b, nb = make_chain(ca, Cn, fs), make_blanker(ca, settings)
    cap = n // 8 + 2048 + 4096
    din, dout = ca.DeviceBuffer(Cn * (n // per * form if form else n * 8)), ca.DeviceBuffer(Cn * cap * 4)
    tr = Trace(ca, Cn, n)
    for k in range(2):
        part = x[:, k * n:(k + 1) * n]
        if form:
            din.upload(make_packets(part, form))
            assert L.csdr_demod_batch_process_packets(b.h, C.c_void_p(din.ptr), n // per, form, nb.h, C.c_void_p(dout.ptr), cap, None) == 0
            args = dict(d_packets=din.ptr, npackets=n // per, pkt_len=form)
        else:
            din.upload(part.astype(np.complex64))
            assert L.csdr_demod_batch_process_blanked(b.h, C.c_void_p(din.ptr), n, n, nb.h, C.c_void_p(dout.ptr), cap, None) == 0
            args = dict(d_in=din.ptr, in_stride=n)
        assert nb.trace_last(tr.buf.ptr, tr.stride, n, **args) == 0
        got = tr.get()
        mask = chain_mask(L, b, Cn, n)
        for c in range(Cn):
            o, tb, bl = refs[c].ProcessBlanker(part[c])
            assert np.array_equal(words(got[c, :n]), words(N.trace_fp32(tb))), (k, c)
            assert ((got[c, :n].real == 0.0) == mask[c]).all() and 0 < mask[c].sum() < n, (k, c)
    b.flush()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_trace_untouched():
    """CSDR_ESTATE before any call, after a set-up, with another count, another buffer, another packet length; CSDR_EINVAL
    for bad arguments; nothing written in any of them"""
    from test_display_stream_gpu import make_packets
    ca, L = internals()
    ESTATE, EINVAL = ca._capi.CSDR_ESTATE, ca._capi.CSDR_EINVAL
    n = 3840                                             # 15 x 256 = 16 x 240
    settings = OBJ_A[:2]
    nb = make_blanker(ca, settings)
    x = np.stack([stream(30 + c, n, False) for c in range(2)])
    din, din2, dout = ca.DeviceBuffer(2 * n * 8), ca.DeviceBuffer(2 * n * 8), ca.DeviceBuffer(2 * n * 8)
    dpk = ca.DeviceBuffer(2 * 16 * 1444)
    din.upload(x.astype(np.complex64)); din2.upload(x.astype(np.complex64))
    tr = Trace(ca, 2, n)
    raw = lambda *a: L.csdr_noiseproc_batch_trace_last(nb.h, *a)
    P = C.c_void_p
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=din.ptr, in_stride=n) == ESTATE          # before any call
    nb.process_ptr(din.ptr, n, n, dout.ptr, n)
    assert nb.trace_last(tr.buf.ptr, tr.stride, n - 2, d_in=din.ptr, in_stride=n) == ESTATE      # another count
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=din2.ptr, in_stride=n) == ESTATE         # another buffer
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=din.ptr, in_stride=n + 2) == ESTATE      # another stride
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_packets=dpk.ptr, npackets=15, pkt_len=1028) == ESTATE   # datagrams behind a rows call
    assert raw(P(din.ptr), n, None, 0, 0, n, None, tr.stride, None) == EINVAL                    # no trace buffer
    assert raw(P(din.ptr), n, None, 0, 0, n, P(tr.buf.ptr), n - 2, None) == EINVAL               # rows too short
    assert raw(P(din.ptr), n, None, 0, 0, n, P(tr.buf.ptr + 8), tr.stride - 2, None) == EINVAL   # misaligned
    assert raw(None, n, P(dpk.ptr), 15, 1000, n, P(tr.buf.ptr), tr.stride, None) == EINVAL       # no such datagram
    assert raw(None, n, P(dpk.ptr), 15, 1444, n, P(tr.buf.ptr), tr.stride, None) == EINVAL       # 15 x 240 != n
    assert tr.untouched()
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=din.ptr, in_stride=n) == 0               # the right one, after all that
    assert not tr.untouched()
    tr.fill()
    nb.setup(True, 25.0, 100.0, 500e3, channel=0)
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=din.ptr, in_stride=n) == ESTATE          # a set-up in between
    # behind a datagram call: another packet length with the same count and buffer
    dpk.upload(make_packets(x, 1028))
    dout2 = ca.DeviceBuffer(2 * n * 8)
    assert L.csdr__noiseproc_batch_process_packets(nb.h, P(dpk.ptr), 15, 1028, P(dout2.ptr), n, None) == 0
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_packets=dpk.ptr, npackets=16, pkt_len=1444) == ESTATE
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=dpk.ptr, in_stride=n) == ESTATE          # rows behind a datagram call
    assert tr.untouched()
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_packets=dpk.ptr, npackets=15, pkt_len=1028) == 0


# ---------------------------------------------------------------------------------------------------- general fp32 rows
GENERAL_SEED, GENERAL_N, GENERAL_FS = 2024, 20000, 500e3


def general_rows():
    rng = np.random.default_rng(GENERAL_SEED)
    x = 1500.0 * (rng.standard_normal((2, GENERAL_N)) + 1j * rng.standard_normal((2, GENERAL_N)))
    x[rng.random((2, GENERAL_N)) < 5e-4] += 25000.0
    x[:, 7000] = 30000.0; x[:, 7012] = complex(0.0, -30000.0)
    return x.astype(np.complex64)


def reverse_window_decisions(x, r):
    """the trigger test of :155-158 with each window's sum taken over the same mag_n + 1 magnitudes from the newest to
    the oldest (the restatement's running sum is another order of the same terms): bool per sample"""
    mag = np.maximum(np.abs(x.real.astype(np.float64)), np.abs(x.imag.astype(np.float64)))
    m1 = r.m_MagSamples + 1
    padded = np.concatenate([np.zeros(m1 - 1), mag])
    win = np.lib.stride_tricks.sliding_window_view(padded, m1)         # row i: samples i - mag_n .. i
    trig = np.zeros(len(mag), dtype=bool)
    for a in range(0, len(mag), 2000):
        s = np.cumsum(win[a:a + 2000, ::-1], axis=1)[:, -1]            # sequential, newest first
        trig[a:a + 2000] = mag[a:a + 2000] * r.m_Ratio > s
    return trig


def test_general_fp32_rows_behind_process():
    """Gaussian noise plus impulses, two receivers at 500 kS/s (100 and 20 us), one call behind _process.  Decisions:
    the real part is 0 exactly where that call's output is (0, 0) -- the delayed input never is, past the empty delay
    line --, bit for bit, because form and cut are the call's.  Values: two fp64 sums of at most 32768 fp32 terms differ
    by far less than an fp32 ulp, so their roundings to fp32 differ by at most one ulp: 2^-22 relative covers it.  The
    restatement's own decisions may differ where a test ties to the last bits of a sum: at most 0.1 % of the samples.
    That cap is a condition on the input, so GENERAL_SEED is chosen such that, on the CPU, the restatement summed
    forwards and the same windows summed in reverse decide identically (asserted below: 0 differing triggers)."""
    ca, L = internals()
    x = general_rows()
    n = GENERAL_N
    settings = [(True, GENERAL_FS, 20.0, 100.0), (True, GENERAL_FS, 20.0, 20.0)]
    nb = make_blanker(ca, settings)
    din, dout = ca.DeviceBuffer(2 * n * 8), ca.DeviceBuffer(2 * n * 8)
    din.upload(x)
    nb.process_ptr(din.ptr, n, n, dout.ptr, n)
    tr = Trace(ca, 2, n)
    assert nb.trace_last(tr.buf.ptr, tr.stride, n, d_in=din.ptr, in_stride=n) == 0
    got = tr.get()
    out = dout.download(np.complex64, 2 * n).reshape(2, n)
    for c, (on, fs, th, w) in enumerate(settings):
        r = N.RefNoiseProc(); r.SetupBlanker(on, th, w, fs)
        o, tb, bl = r.ProcessBlanker(x[c].astype(np.complex128))
        # the condition on the seed: the restatement's decisions do not depend on the order of its sums
        assert (bl == blank_flags(reverse_window_decisions(x[c], r), r.m_WidthSamples)).all(), c
        d = r.m_DelaySamples + 1
        zero = (out[c].real == 0.0) & (out[c].imag == 0.0)
        assert (x[c, :n - d] != 0).all()
        assert ((got[c, d:n].real == 0.0) == zero[d:]).all(), c
        disagree = int(((got[c, :n].real == 0.0) != bl).sum())
        print("receiver %d: %d of %d decisions differ from the restatement's" % (c, disagree, n))
        assert disagree <= n // 1000, (c, disagree)
        both = ~bl & (got[c, :n].real != 0.0)
        want = tb.real[both]
        rel = np.abs(got[c, :n].real[both].astype(np.float64) - want) / np.abs(want)
        print("receiver %d: largest relative difference of a shown sum %.3g" % (c, rel.max()))
        assert both.sum() > n // 2 and rel.max() <= 2.0 ** -22, (c, rel.max())
        assert np.array_equal(words(got[c, :n].imag.copy()), words(N.trace_fp32(tb).imag.copy())), c   # the delayed sample: exact


def blank_flags(trig, width):
    """the blank flags that triggers give: a trigger at i blanks i .. i + width - 1 (:157-166)"""
    n = len(trig)
    last = np.maximum.accumulate(np.where(trig, np.arange(n), -10 ** 9))
    return np.arange(n) - last < width
