"""Batch sound sink (csdr_soundsink_batch_*): C independent CSoundOut sinks (interface/soundout.cpp:155-468,
non-blocking mode) behind the batched chain, resampled together on the device.  Every receiver is checked against
its own oracle CSoundOut (or against its own single csdr_soundsink on the GPU) driven with the same puts and gets:
resampled counts exact, queue level / correction / fill average / ppm identical after every get, samples within
1 LSB.  The last two tests run without a GPU."""
import os
import threading
import time

import numpy as np
import pytest

RATES = [62500.0, 31250.0, 15625.0, 48000.0, 24000.0, 11025.0]
VOLUMES = [80, 99, 70, 0, 90, 75]                      # receiver 3 muted
PPM = [800.0, -800.0, 500.0, -300.0, 650.0, -700.0]     # each producer's clock error against its sound card
TICK_HZ = [100, 50, 125, 80, 200, 64]                  # each sound card pops 48000 / tick_hz samples per tick
PUT_S = 0.02                                           # one batched put every 20 ms of simulated time
UNDERFLOW_RX, UNDERFLOW_AT = 1, (4.0, 4.6)             # this producer delivers nothing for 0.6 s: its queue runs dry
OVERFLOW_RX, OVERFLOW_AT = 2, (5.0, 5.5)               # this sound card pops nothing for 0.5 s: its queue fills


def schedule(seconds, rates=RATES, extra=()):
    """The event list both sides replay: ("put", counts, starts), ("get", channel, n), plus `extra` control events
    (time, event) merged in by time.  Puts come first at equal times."""
    C = len(rates)
    ev = [(t, 2, e) for t, e in extra]
    delivered = [0] * C
    for p in range(1, int(round(seconds / PUT_S)) + 1):
        t = p * PUT_S
        counts, starts = [], []
        for c in range(C):
            avail = int(rates[c] * (1.0 + PPM[c] * 1e-6) * t)
            stalled = c == UNDERFLOW_RX and UNDERFLOW_AT[0] <= t < UNDERFLOW_AT[1]
            starts.append(delivered[c])
            counts.append(0 if stalled else avail - delivered[c])
            delivered[c] = avail
        ev.append((t, 0, ("put", counts, starts)))
    for c in range(C):
        for m in range(1, int(seconds * TICK_HZ[c]) + 1):
            t = m / TICK_HZ[c]
            if c == OVERFLOW_RX and OVERFLOW_AT[0] <= t < OVERFLOW_AT[1]:
                continue
            ev.append((t, 1, ("get", c, 48000 // TICK_HZ[c])))
    ev.sort(key=lambda e: (e[0], e[1]))
    return [e for _, _, e in ev]


def signal(c, start, n, fs, stereo):
    k = np.arange(n) + start
    x = 9000.0 * np.sin(2 * np.pi * (700.0 + 150.0 * c) * k / fs)
    if stereo:
        x = x + 1j * 9000.0 * np.cos(2 * np.pi * (500.0 + 100.0 * c) * k / fs)
    return x.astype(np.complex64 if stereo else np.float32)


class BatchSide:
    def __init__(self, b):
        self.b = b

    def put(self, rows, counts):
        return list(self.b.PutOutQueue(rows, counts))

    def get(self, c, n):
        return self.b.GetOutQueue(c, n)

    def rate(self, c, r):
        self.b.ChangeUserDataRate(c, r)

    def volume(self, c, v):
        self.b.SetVolume(c, v)

    def state(self, c):
        b = self.b
        return (b.level(c), b.rate_correction(c), b.ave_level(c), b.ppm_error(c))


class SinglesSide:
    """One CSoundOut per receiver (the oracle's, or the GPU's single sink) fed the same rows through the host"""

    def __init__(self, sinks):
        self.s = sinks

    def put(self, rows, counts):
        out = []
        for c, s in enumerate(self.s):
            n = int(counts[c])
            x = rows[c, :n]
            out.append(s.PutOutQueue(x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)) if n else 0)
        return out

    def get(self, c, n):
        return self.s[c].GetOutQueue(n)

    def rate(self, c, r):
        for i in (range(len(self.s)) if c < 0 else [c]):
            self.s[i].ChangeUserDataRate(r)

    def volume(self, c, v):
        for i in (range(len(self.s)) if c < 0 else [c]):
            self.s[i].SetVolume(v)

    def state(self, c):
        s = self.s[c]
        return (s.level(), s.rate_correction(), s.ave_level(), s.ppm_error())


def replay(side, events, rates, stereo, volumes=VOLUMES):
    """Run the events; returns per-put counts [puts][C], per-receiver popped samples, per-receiver traces and, per
    receiver, whether it overflowed / underflowed (seen from the level around each put / get), and where in the
    traces each rate change came."""
    C = len(rates)
    for c in range(C):
        side.rate(c, rates[c])
        side.volume(c, volumes[c])
    cur_rates = list(rates)
    counts, popped, trace = [], [[] for _ in range(C)], [[] for _ in range(C)]
    over, under, marks = [False] * C, [False] * C, []
    for e in events:
        if e[0] == "put":
            _, n, starts = e
            T = max(max(n), 1)
            rows = np.zeros((C, T), dtype=np.complex64 if stereo else np.float32)
            for c in range(C):
                rows[c, :n[c]] = signal(c, starts[c], n[c], cur_rates[c], stereo)
            before = [side.state(c)[0] for c in range(C)]
            k = side.put(rows, n)
            for c in range(C):
                over[c] |= side.state(c)[0] < before[c] + k[c]
            counts.append(list(k))
        elif e[0] == "get":
            _, c, n = e
            before = side.state(c)[0]
            popped[c].append(side.get(c, n))
            st = side.state(c)
            under[c] |= st[0] > before
            trace[c].append(st)
        elif e[0] == "rate":
            marks.append([len(t) for t in trace])
            side.rate(e[1], e[2])
            for c in (range(C) if e[1] < 0 else [e[1]]):
                cur_rates[c] = e[2]
        elif e[0] == "volume":
            side.volume(e[1], e[2])
    return (np.array(counts), [np.concatenate(p) for p in popped], [np.array(t) for t in trace], over, under, marks)


def compare(got, want):
    cg, pg, tg, og, ug = got[:5]
    cw, pw, tw, ow, uw = want[:5]
    assert np.array_equal(cg, cw)                                   # resampled counts of every receiver, every put
    for c in range(len(pg)):
        assert np.array_equal(tg[c], tw[c]), c                      # level, correction, average, ppm after every get
        assert pg[c].shape == pw[c].shape, c
        assert np.abs(pg[c].astype(np.int32) - pw[c].astype(np.int32)).max() <= 1, c
    assert og == ow and ug == uw


def check_run(res, volumes=VOLUMES):
    counts, popped, trace, over, under = res[:5]
    assert over[OVERFLOW_RX] and under[UNDERFLOW_RX]
    assert (counts[:, UNDERFLOW_RX] == 0).any()                    # the stalled producer's rows carried n_in = 0
    for c, p in enumerate(popped):
        if volumes[c] == 0:
            assert not p.any(), c
        else:
            assert np.abs(p.astype(np.int32)).max() > 1000, c
        assert trace[c][-1, 1] != 0.0, c                            # every rate loop has started correcting


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_mixed_rates_match_the_oracle(oracle, stereo):
    """Six receivers at six user rates and volumes (one muted), each producer and sound card on its own clock,
    9.5 simulated seconds: one queue overflows, one runs dry, every rate loop corrects."""
    import cutesdr_amd as ca
    ev = schedule(9.5)
    got = replay(BatchSide(ca.SoundSinkBatch(len(RATES), stereo)), ev, RATES, stereo)
    want = replay(SinglesSide([oracle.CSoundOut(stereo) for _ in RATES]), ev, RATES, stereo)
    compare(got, want)
    check_run(want)


@pytest.mark.gpu
def test_receivers_are_independent(oracle):
    """Mid-stream: one receiver's rate changes, then every receiver's (channel -1; one is already at that rate, its
    queue must stay), a volume changes, one receiver gets empty rows for a while; everything against the oracle."""
    import cutesdr_amd as ca
    extra = [(2.005, ("rate", 0, 50000.0)), (3.005, ("volume", 4, 40)), (6.005, ("rate", -1, 48000.0))]
    ev = schedule(7.5, extra=extra)
    for e in ev:                                                    # receiver 5: no audio for 0.2 s
        if e[0] == "put" and 2.6 <= e[2][5] / RATES[5] < 2.8:
            e[1][5] = 0
    got = replay(BatchSide(ca.SoundSinkBatch(len(RATES))), ev, RATES, False)
    want = replay(SinglesSide([oracle.CSoundOut() for _ in RATES]), ev, RATES, False)
    compare(got, want)
    trace = want[2]
    assert (want[0][:, 5] == 0).sum() >= 9
    m = want[5][-1]                                                 # the traces from the channel -1 change on
    assert trace[3][m[3]:, 0].min() > 4000                          # receiver 3 was at 48 kHz already: its queue stays
    for c in (0, 1, 2, 4, 5):                                       # the others were cleared and started up again
        assert trace[c][m[c]:, 0].min() < 2000 and trace[c][-1, 3] == 0, c


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_batch_matches_single_sinks_on_the_gpu(stereo):
    """The same rows and get schedule through C single csdr_soundsinks: counts and traces equal, samples within 1."""
    import cutesdr_amd as ca
    ev = schedule(9.5)
    got = replay(BatchSide(ca.SoundSinkBatch(len(RATES), stereo)), ev, RATES, stereo)
    want = replay(SinglesSide([ca.CSoundOut(stereo) for _ in RATES]), ev, RATES, stereo)
    compare(got, want)
    check_run(got)


@pytest.mark.gpu
def test_end_to_end_behind_the_demod_batch():
    """DemodBatch (AM, FM, USB, SAM) -> SoundSinkBatch straight from the device rows, rates from get_output_rate and
    counts from out_count, against single sinks fed the same rows through the host."""
    import cutesdr_amd as ca
    from test_postchain_gpu import MODES, info, make_input
    names = ["AM", "FM", "USB", "SAM"]
    fs, T, calls = 2e6, 1 << 17, 24
    C = len(names)
    b = ca.DemodBatch(C, 2048)
    b.set_input_rate(fs)
    for c, name in enumerate(names):
        m, kw = MODES[name]
        if name == "USB":
            kw = dict(kw, HiCutmax=5000)                            # a narrower maximum: a third output rate
        b.set_demod(c, m, info(ca, **kw))
    b.commit()
    for c in range(C):
        b.set_freq(c, -100e3)
    rates = [b.output_rate(c) for c in range(C)]
    assert len(set(rates)) >= 3, rates
    x = np.stack([make_input(name, T * calls, fs) for name in names]).astype(np.complex64)
    sink, singles = ca.SoundSinkBatch(C), [ca.CSoundOut() for _ in range(C)]
    for c in range(C):
        sink.ChangeUserDataRate(c, rates[c]); singles[c].ChangeUserDataRate(rates[c])
        sink.SetVolume(c, 95); singles[c].SetVolume(95)
    cap = T + 2048
    din, dout = ca.DeviceBuffer(C * T * 8), ca.DeviceBuffer(C * cap * 4)
    pop = int(48000 * T / fs)
    got, want, loud = [[] for _ in range(C)], [[] for _ in range(C)], [0] * C
    for call in range(calls):
        din.upload(np.ascontiguousarray(x[:, call * T:(call + 1) * T]))
        b.process_ptr(din.ptr, T, T, dout.ptr, cap)
        ca.sync()
        counts = np.array([b.out_count(c) for c in range(C)], dtype=np.int32)
        k = sink.put_ptr(dout.ptr, cap, counts)
        rows = dout.download(np.float32, C * cap).reshape(C, cap)
        for c in range(C):
            assert k[c] == (singles[c].PutOutQueue(rows[c, :counts[c]].astype(np.float64)) if counts[c] else 0)
            g, w = sink.GetOutQueue(c, pop), singles[c].GetOutQueue(pop)
            assert (sink.level(c), sink.ave_level(c), sink.rate_correction(c)) == \
                (singles[c].level(), singles[c].ave_level(), singles[c].rate_correction())
            got[c].append(g); want[c].append(w)
            loud[c] = max(loud[c], int(np.abs(w.astype(np.int32)).max()))
    for c in range(C):
        assert np.abs(np.concatenate(got[c]).astype(np.int32) - np.concatenate(want[c]).astype(np.int32)).max() <= 1
        assert loud[c] > 0, names[c]
        assert singles[c].level() > 0


@pytest.mark.gpu
def test_rejected_puts_change_nothing(oracle):
    """A row over 8192 samples, or one too long for its queue at its rate: CSDR_EINVAL, nothing changes, the
    following puts still match the oracle exactly."""
    import ctypes
    import cutesdr_amd as ca
    from cutesdr_amd import _capi
    rates, C = [62500.0, 11025.0, 48000.0], 3
    b = ca.SoundSinkBatch(C)
    refs = [oracle.CSoundOut() for _ in range(C)]
    for c in range(C):
        b.ChangeUserDataRate(c, rates[c]); refs[c].ChangeUserDataRate(rates[c])
        b.SetVolume(c, 90); refs[c].SetVolume(90)
    T = 8200
    rows = np.stack([signal(c, 0, T, rates[c], False) for c in range(C)])
    dev = ca.DeviceBuffer(rows.nbytes)
    dev.upload(rows)
    L = _capi.lib()

    def raw_put(counts):
        n = np.array(counts, dtype=np.int32)
        k = np.full(C, -7, dtype=np.int32)
        rc = L.csdr_soundsink_batch_put(b.h, ctypes.c_void_p(dev.ptr), T, n.ctypes.data_as(ctypes.c_void_p),
                                        k.ctypes.data_as(ctypes.c_void_p), None)
        return rc, k
    start = [0] * C
    for step in range(30):
        if step in (5, 17):
            for bad in ([1000, 1000, 8193], [1000, 3800, 1000]):   # > 8192; 3800 / (11025 / 48000) + 8 > 16384
                rc, k = raw_put(bad)
                assert rc == _capi.CSDR_EINVAL and (k == -7).all(), bad
        n = [1200, 300, 1000]
        x = np.stack([signal(c, start[c], T, rates[c], False) for c in range(C)])
        dev.upload(x)
        rc, k = raw_put(n)
        assert rc == _capi.CSDR_OK
        for c in range(C):
            assert k[c] == refs[c].PutOutQueue(x[c, :n[c]].astype(np.float64))
            g, w = b.GetOutQueue(c, 700), refs[c].GetOutQueue(700)
            assert np.abs(g.astype(np.int32) - w.astype(np.int32)).max() <= 1
            assert (b.level(c), b.ave_level(c)) == (refs[c].level(), refs[c].ave_level())
            start[c] += n[c]


@pytest.mark.gpu
def test_one_producer_many_consumers():
    """One thread puts while one thread per receiver gets (ctypes releases the GIL): no error, and every receiver's
    pushed - popped equals its level up to whole underflows (each get takes more than a put brings, so no queue
    overflows), within a time limit."""
    import cutesdr_amd as ca
    C, puts, rate = 8, 300, 48000.0
    b = ca.SoundSinkBatch(C)
    b.ChangeUserDataRate(-1, rate)
    b.SetVolume(-1, 99)
    T = 960
    rows = np.stack([signal(c, 0, T, rate, False) for c in range(C)])
    counts = np.full(C, T, dtype=np.int32)
    for _ in range(10):                                             # past the start-up: level > half the queue
        b.PutOutQueue(rows, counts)
    for c in range(C):
        b.GetOutQueue(c, 1)
    base = [b.level(c) for c in range(C)]
    pushed, popped, gets, errors = [0] * C, [0] * C, [0] * C, []
    done = threading.Event()

    def producer():
        try:
            for i in range(puts):
                last = list(gets)
                deadline = time.perf_counter() + 30
                while any(gets[c] == last[c] for c in range(C)) and time.perf_counter() < deadline:
                    time.sleep(0.0002)                              # every consumer has popped since the last put
                k = b.PutOutQueue(rows, counts)
                for c in range(C):
                    pushed[c] += int(k[c])
        except Exception as e:                                      # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    def consumer(c):
        try:
            n = 1024 + 37 * c                                       # more than a put brings: the queues never overflow
            while not done.is_set():
                popped[c] += len(b.GetOutQueue(c, n))
                gets[c] += 1
                b.level(c); b.rate_correction(c); b.ave_level(c); b.ppm_error(c)
                time.sleep(0.0005 * (c % 3))
        except Exception as e:                                      # noqa: BLE001
            errors.append(e)
    t0 = time.perf_counter()
    threads = [threading.Thread(target=producer)] + [threading.Thread(target=consumer, args=(c,)) for c in range(C)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors
    assert time.perf_counter() - t0 < 120
    for c in range(C):
        assert popped[c] > 0 and pushed[c] > 0
        # an underflow backs the tail up a quarter (level + 4096) and hands out one sample without taking it off the
        # queue (soundout.cpp:344-351): level = base + pushed - popped + 4097 * underflows
        assert (base[c] + pushed[c] - popped[c] - b.level(c)) % 4097 == 0, c
        assert 0 <= b.level(c) < 16384


def test_no_cpu_fallback_for_the_batch_sink():
    from cutesdr_amd import _build, _capi
    _build.build()
    L = _capi.lib()
    if L.csdr_device_count() > 0:
        pytest.skip("GPU present")
    assert not L.csdr_soundsink_batch_create(0, 4, 0)
    assert b"no HIP device" in L.csdr_last_error()
    import cutesdr_amd
    with pytest.raises(_capi.CsdrError):
        cutesdr_amd.SoundSinkBatch(4)


def test_the_batch_sink_holds_no_device_wide_synchronisation():
    """put, get and the setters wait on the caller's stream at most, never on the whole device (source scan)."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cutesdr_amd", "csrc")

    def body(path, signature):
        txt = open(os.path.join(root, path)).read()
        i = txt.index(signature)
        j = txt.index("{", i)
        depth, k = 0, j
        while True:
            depth += txt[k] == "{"
            depth -= txt[k] == "}"
            k += 1
            if depth == 0:
                return txt[j:k]
    for sig in ("int csdr_soundsink_batch_put(", "int csdr_soundsink_batch_get(",
                "int csdr_soundsink_batch_change_user_data_rate(", "int csdr_soundsink_batch_set_volume(",
                "double csdr_soundsink_batch_get_rate_correction(", "double csdr_soundsink_batch_get_ave_level(",
                "int csdr_soundsink_batch_get_level(", "int csdr_soundsink_batch_get_ppm_error("):
        b = body("capi_soundsink_batch.hip", sig)
        assert "hipDeviceSynchronize" not in b and "hipMemcpy(" not in b, sig
    put = body("capi_soundsink_batch.hip", "int csdr_soundsink_batch_put(")
    assert put.count("hipStreamSynchronize((hipStream_t)stream)") == 1
    q = open(os.path.join(root, "soundsink_queue.hpp")).read()
    assert "hipDeviceSynchronize" not in q
    # both sinks run the same queue rules
    for f in ("capi_soundsink.hip", "capi_soundsink_batch.hip"):
        assert '#include "soundsink_queue.hpp"' in open(os.path.join(root, f)).read()
