"""The resampler and sound-sink kernels (K5 / K5b: resample_kernel, resample_batch_kernel, soundsink_batch_kernel<1|2>)
under the K5 word rule of tests/resampler_ref.py, through the C ABI, in five forms: CFractResampler (four overloads),
ResamplerBatch (float and int16), CSoundOut, SoundSinkBatch mono and stereo.

  impulse trains  every output is one table entry times a power of two: the float forms must equal fp32(the oracle's
                  fp64 output) bit for bit (a table index one entry off leaves under 11 % of the words equal, a wrong
                  input address changes the power of two); the int16 forms and the sinks run the same trains under
                  the int16 rule (the sinks at volume 99 and 87: their gain follows the volume law, 1 and 0.494).
  dense rows      |got - y| <= 30 u S on every float sample; every decided word equal, every undecided word lo or hi;
                  at most 2 % undecided on the low-level rows; at least 10 % decided-and-clipped on the clip rows
                  (every form has one: the sinks' clip is their own code).
  sound sinks     six receivers, per put, the batch sink's words from its tap and the single sink's through its queue,
                  the oracle's CSoundOut beside them for the state: counts, level, correction, fill average, ppm equal.

The bounds are derived in resampler_ref.py, not measured here; the cap on every row is checked from the reference
alone in tests/test_resampler_words_host.py.  Every test prints its figures per form."""
import ctypes as C

import numpy as np
import pytest

import resampler_ref as R

pytestmark = pytest.mark.gpu


def cols(a):
    """complex (n,) -> (n, 2) re / im; everything else as it is"""
    a = np.asarray(a)
    return np.stack([a.real, a.imag], axis=1) if np.iscomplexobj(a) else a


def fp32_of(want):
    return cols(want).astype(np.float32).astype(np.float64)


def trains(cpx):
    x = R.impulse_train(4096)
    return x + 1j * R.impulse_train(4096, offset=7, first=5) if cpx else x


# --------------------------------------------------------------------------------------------------------------
# form 1: CFractResampler

@pytest.mark.parametrize("rate", R.IMPULSE_RATES)
def test_one_stream_impulse_train(oracle, rate):
    import cutesdr_amd as ca
    for cpx in (False, True):
        g, o = ca.CFractResampler(), oracle.CFractResampler()
        g.Init(4096); o.Init(4096)
        n = nz = 0
        for p in R.split(trains(cpx), R.IMPULSE_CALLS):
            got, want = g.Resample(p, rate), o.Resample(p, rate)
            assert len(got) == len(want)
            assert np.array_equal(cols(got), fp32_of(want)), (rate, cpx)
            n += cols(got).size
            nz += np.count_nonzero(cols(got))
        print("CFractResampler %s rate %g: %d of %d float words equal bit for bit (%d non-zero)" %
              ("complex" if cpx else "real", rate, n, n, nz))
        assert nz > n // 2
        for gain in (1.0, 0.5):
            g, h = ca.CFractResampler(), R.Resampler()
            g.Init(4096)
            t = R.Tally("CFractResampler %s int16 impulses, rate %g gain %g" % ("complex" if cpx else "real", rate, gain))
            for p in R.split(trains(cpx), R.IMPULSE_CALLS):
                y, S = h.resample(p, rate)
                got = g.Resample(p, rate, gain)
                assert len(got) == len(y)
                t.words(got, y, S, gain)
            print(t)
            assert t.ok, str(t)


@pytest.mark.parametrize("kind,rate,gain,peak", R.DENSE, ids=["%s-%g" % (d[0], d[1]) for d in R.DENSE])
def test_one_stream_dense_rows(kind, rate, gain, peak):
    """all four overloads over the ragged calls (1, 1, 1, 27, 28, 29, 0, 2048) and the 256 / 257-output calls"""
    import cutesdr_amd as ca
    calls, re = R.dense_row(kind, peak, 1, rate)
    im = R.dense_row(kind, peak, 51, rate)[1]
    h, ref = R.Resampler(), []
    for p, q in zip(re, im):
        ref.append(h.resample(p + 1j * q, rate))
    counts = [len(y) for y, _ in ref]
    assert calls[:8] == R.RAGGED and counts[6] == 0
    if rate >= 1.0:
        assert counts[8:10] == [256, 257]
    else:
        assert 256 <= counts[8] <= 262 and 257 <= counts[9] <= 263
    Y, S = np.concatenate([y for y, _ in ref]), np.concatenate([s for _, s in ref])
    for cpx in (False, True):
        gf, gi = ca.CFractResampler(), ca.CFractResampler()
        gf.Init(4096); gi.Init(4096)
        t = R.Tally("CFractResampler %s, %s rate %g gain %g peak %g" % ("complex" if cpx else "real", kind, rate, gain, peak))
        for i, (p, q) in enumerate(zip(re, im)):
            x = p + 1j * q if cpx else p
            y, s = ref[i] if cpx else (ref[i][0][:, 0], ref[i][1][:, 0])
            a, b = gf.Resample(x, rate), gi.Resample(x, rate, gain)
            assert len(a) == len(b) == len(y), (i, len(a), len(b), len(y))
            t.floats(cols(a), y, s).words(b, y, s, gain)
        print(t)
        assert t.ok, str(t)
        if kind == "clip":
            assert t.decided_clipped >= 0.10 * t.nw
        else:
            assert gain * peak <= 1000.0
            for w in range(2 if cpx else 1):
                assert R.undecided_share(Y[:, w], S[:, w], gain) <= R.CAP
            assert t.share <= R.CAP


# --------------------------------------------------------------------------------------------------------------
# form 2: ResamplerBatch

def batch_call(b, ca, x, rate, gain, pad=37):
    """resample_ptr with in_stride = n + pad; the padding holds a value that would wreck any sample that read it"""
    Cn, n = x.shape
    stride = n + pad
    a = np.full((Cn, stride), 3.0e30, dtype=np.float32)
    a[:, :n] = x
    cap = int(n / rate) + 8
    din = ca.DeviceBuffer(a.nbytes)
    dout = ca.DeviceBuffer(Cn * cap * 4)
    din.upload(a)
    k = b.resample_ptr(din.ptr, stride, n, rate, dout.ptr, cap, gain)
    ca.sync()
    out = dout.download(np.float32 if gain is None else np.int16, Cn * cap).reshape(Cn, cap)
    return out[:, :k].copy()


@pytest.mark.parametrize("rate", R.IMPULSE_RATES)
def test_batch_impulse_train(oracle, rate):
    import cutesdr_amd as ca
    Cn = 5
    x = np.stack([R.impulse_train(4096, offset=5 * c, first=c) for c in range(Cn)])
    b = ca.ResamplerBatch(Cn)
    refs = [oracle.CFractResampler() for _ in range(Cn)]
    for r in refs:
        r.Init(4096)
    n = at = 0
    for m in R.IMPULSE_CALLS:
        got = batch_call(b, ca, x[:, at:at + m], rate, None)
        for c in range(Cn):
            want = refs[c].Resample(x[c, at:at + m], rate)
            assert got.shape[1] == len(want)
            assert np.array_equal(got[c].astype(np.float64), fp32_of(want)), (rate, c)
        n += got.size
        at += m
    print("ResamplerBatch rate %g: %d of %d float words equal bit for bit" % (rate, n, n))
    for gain in (1.0, 0.5):
        b, hs, at = ca.ResamplerBatch(Cn), [R.Resampler() for _ in range(Cn)], 0
        t = R.Tally("ResamplerBatch int16 impulses, rate %g gain %g" % (rate, gain))
        for m in R.IMPULSE_CALLS:
            got = batch_call(b, ca, x[:, at:at + m], rate, gain)
            for c in range(Cn):
                y, S = hs[c].resample(x[c, at:at + m], rate)
                assert got.shape[1] == len(y)
                t.words(got[c], y, S, gain)
            at += m
        print(t)
        assert t.ok, str(t)


@pytest.mark.parametrize("rate", R.BATCH_RATES)
def test_batch_dense_rows(rate):
    """five channels of different content, in_stride > n, float and int16 calls in turn (the history ping-pong is
    crossed by both), the ragged calls, the 256 / 257-output pair twice (each count once as float and once as int16) and two 2048-sample calls"""
    import cutesdr_amd as ca
    Cn, gain = len(R.BATCH_ROWS), R.BATCH_GAIN
    rows = [R.dense_row(kind, peak, 300 + c, rate, extra=R.BATCH_EXTRA) for c, (kind, peak) in enumerate(R.BATCH_ROWS)]
    calls = rows[0][0]
    b, hs = ca.ResamplerBatch(Cn), [R.Resampler() for _ in range(Cn)]
    ts = [R.Tally("ResamplerBatch rate %g row %d (%s)" % (rate, c, R.BATCH_ROWS[c][0])) for c in range(Cn)]
    YS = [[] for _ in range(Cn)]
    for i, n in enumerate(calls):
        x = np.stack([rows[c][1][i] for c in range(Cn)]).reshape(Cn, n)
        g = None if i % 2 == 0 else gain
        got = batch_call(b, ca, x, rate, g)
        for c in range(Cn):
            y, S = hs[c].resample(x[c], rate)
            YS[c].append((y, S))
            assert got.shape[1] == len(y), (i, c)
            if g is None:
                ts[c].floats(got[c], y, S)
            else:
                ts[c].words(got[c], y, S, g)
    assert calls[7] == 2048 and calls[10] == 2048            # one as int16, one as float
    if rate >= 1.0:                                          # 256 outputs as float (call 8) and as int16 (call 11), 257 likewise
        assert [len(YS[0][i][0]) for i in (8, 9, 11, 12)] == [256, 257, 256, 257]
    for c, t in enumerate(ts):
        print(t)
        assert t.ok and t.nf > 500 and t.nw > 500, str(t)
        Y, S = np.concatenate([y for y, _ in YS[c]]), np.concatenate([s for _, s in YS[c]])
        if R.BATCH_ROWS[c][0] == "clip":
            assert t.decided_clipped >= 0.10 * t.nw
        else:
            assert R.undecided_share(Y, S, gain) <= R.CAP and t.share <= R.CAP


# --------------------------------------------------------------------------------------------------------------
# forms 3-5: the sound sinks

class BatchSink:
    """SoundSinkBatch behind the SinkDriver's side interface; the words come from the tap"""

    def __init__(self, ca, Cn, stereo):
        self.ca, self.b, self.w = ca, ca.SoundSinkBatch(Cn, stereo), 2 if stereo else 1

    def rate(self, c, r):
        self.b.ChangeUserDataRate(c, r)

    def volume(self, c, v):
        self.b.SetVolume(c, v)

    def put(self, rows, counts):
        return self.b.PutOutQueue(rows, counts)

    def get(self, c, n):
        return self.b.GetOutQueue(c, n)

    def state(self, c):
        b = self.b
        return (b.level(c), b.rate_correction(c), b.ave_level(c), b.ppm_error(c))

    def tap(self, c, k):
        d_rows, stride, d_counts = self.b.tap()
        cnt = np.zeros(self.b.channels, dtype=np.int32)
        assert self.ca.lib().csdr_dev_download(0, cnt.ctypes.data_as(C.c_void_p), C.c_void_p(d_counts), cnt.nbytes) == 0
        assert cnt[c] == k
        out = np.zeros(k * self.w, dtype=np.int16)
        if k:
            src = d_rows + 2 * c * stride * self.w
            assert self.ca.lib().csdr_dev_download(0, out.ctypes.data_as(C.c_void_p), C.c_void_p(src), out.nbytes) == 0
        return out.reshape(k, 2) if self.w == 2 else out


class SingleSinks:
    """one CSoundOut on the GPU per receiver; the words come through the queue"""

    def __init__(self, ca, Cn, stereo):
        self.s = [ca.CSoundOut(stereo) for _ in range(Cn)]

    def rate(self, c, r):
        self.s[c].ChangeUserDataRate(r)

    def volume(self, c, v):
        self.s[c].SetVolume(v)

    def put(self, rows, counts):
        return [self.s[c].PutOutQueue(rows[c, :counts[c]]) if counts[c] else 0 for c in range(len(self.s))]

    def get(self, c, n):
        return self.s[c].GetOutQueue(n)

    def state(self, c):
        s = self.s[c]
        return (s.level(), s.rate_correction(), s.ave_level(), s.ppm_error())

    def tap(self, c, k):
        return None


def check_sinks(name, got, log, ref, caps):
    """got: a driver's log; log / ref: the oracle's run and the fp64 reference of its puts"""
    assert len(got) == len(log)
    for c in range(len(log)):
        assert len(got[c]) == len(log[c]) == len(ref[c])
        t = R.Tally("%s receiver %d" % (name, c))
        for i, (rec, (y, S)) in enumerate(zip(log[c], ref[c])):
            g = got[c][i]
            assert g["k"] == rec["k"] == len(y), (c, i, g["k"], rec["k"], len(y))
            assert g["state"] == rec["state"] and g["rate"] == rec["rate"], (c, i)     # level, correction, average, ppm
            assert g["words"] is not None, (c, i)
            t.words(g["words"], y, S, rec["gain"])
        print(t)
        assert t.ok, str(t)
        if caps:
            assert t.share <= R.CAP
        elif caps is None:                                     # a clip row: no cap, a good share saturated
            assert t.decided_clipped >= 0.10 * t.nw


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_batch_sink_per_put(oracle, stereo):
    import cutesdr_amd as ca
    log, ref = R.oracle_sink_run(oracle, stereo)
    d = R.SinkDriver(BatchSink(ca, 6, stereo), R.SINK_RATES, R.SINK_VOLUMES, stereo)
    d.run(R.sink_rows(stereo), R.sink_plan())
    check_sinks("SoundSinkBatch %s" % ("stereo" if stereo else "mono"), d.log, log, ref, True)
    corr = {r["corr"] for r in d.log[5] if len(r["x"])}
    assert len(corr - {0.0}) >= 2                              # receiver 5 ran under two different corrections
    assert [r["k"] for r in d.log[3] if len(r["x"]) in (1024, 2048)] == [1024, 2048, 1024]      # whole chunks


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_single_sinks_per_put(oracle, stereo):
    import cutesdr_amd as ca
    log, ref = R.oracle_sink_run(oracle, stereo)
    d = R.SinkDriver(SingleSinks(ca, 6, stereo), R.SINK_RATES, R.SINK_VOLUMES, stereo)
    d.run(R.sink_rows(stereo), R.sink_plan())
    assert not any(d.pending)
    check_sinks("CSoundOut %s" % ("stereo" if stereo else "mono"), d.log, log, ref, True)


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_sinks_clip_rows(oracle, stereo):
    """three loud receivers (gain * peak 47000 ... 60000) through the batch sink and the single sinks: the lo / hi rule
    everywhere, +-32767 included, no cap, at least 10 % of every receiver's words decided and clipped"""
    import cutesdr_amd as ca
    log, ref = R.oracle_sink_run(oracle, stereo, clip=True)
    for name, side in (("SoundSinkBatch", BatchSink(ca, 3, stereo)), ("CSoundOut", SingleSinks(ca, 3, stereo))):
        d = R.SinkDriver(side, R.CLIP_SINK_RATES, R.CLIP_SINK_VOLUMES, stereo)
        d.run(R.clip_sink_rows(stereo), R.clip_sink_plan())
        assert not any(d.pending)
        check_sinks("%s %s clip" % (name, "stereo" if stereo else "mono"), d.log, log, ref, None)


@pytest.mark.parametrize("volume", [99, 87])
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_sinks_impulse_train(oracle, stereo, volume):
    """six receivers at the six impulse rates (user rate = 48000 rate), three puts each, both kinds of sink"""
    import cutesdr_amd as ca
    rates = [48000.0 * r for r in R.IMPULSE_RATES]
    streams = [R.impulse_train(4096, offset=3 * c, first=c) for c in range(6)]
    if stereo:
        streams = [np.stack([s, R.impulse_train(4096, offset=3 * c + 11, first=c + 4)], axis=1) for c, s in enumerate(streams)]
    plan = [("put", [n] * 6) for n in R.IMPULSE_CALLS]
    o = R.SinkDriver(R.OracleSinks(oracle, 6, stereo), rates, [volume] * 6, stereo).run(streams, plan)
    ref = [R.sink_reference(log) for log in o.log]
    for name, side in (("SoundSinkBatch", BatchSink(ca, 6, stereo)), ("CSoundOut", SingleSinks(ca, 6, stereo))):
        d = R.SinkDriver(side, rates, [volume] * 6, stereo).run(streams, plan).flush()
        check_sinks("%s %s impulses volume %d" % (name, "stereo" if stereo else "mono", volume), d.log, o.log, ref, False)
