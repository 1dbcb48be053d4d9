"""The fp64 statement of CFractResampler (reference dsp/fractresampler.cpp:85-184) and the K5 word rule that
tests/test_resampler_words_host.py and tests/test_resampler_words_gpu.py hold the resampler and sound-sink kernels
to.  Plain numpy, nothing from oracle/: the Blackman-Harris windowed sinc table in fp64, the sequential time chain
`while (int)t < n: emit t; t += rate`, then `t -= n`, and the 28-sample history, one object per stream.

Each call returns, per output sample, y = the fp64 dot product and S = sum_j |x_j w_k(j)| over the 28 taps.

The rule, u = 2^-24:
  float   |got - y| <= 30 u S.  Derived, not measured: the fp32 table entry is rounded once, each product once, and
          28 terms take at most 27 additions: gamma_29 S; 30 covers the (1 - 29 u) denominator.  FMA contraction
          only removes roundings.  The inputs must be fp32 values, so that the ABI's fp64 -> fp32 conversion adds
          nothing.
  int16   d = 32 u gain S (two more roundings: (float)gain and the product), lo = trunc(clip(y gain - d)),
          hi = trunc(clip(y gain + d)), clip to +-32767.  A sample with lo == hi is decided: the word must EQUAL it.
          An undecided word must be lo or hi.  The clipped value is part of it: |y gain| >= 32767 + d gives exactly
          +-32767; gain 0 gives 0.
  cap     a condition on the rows, so that the int16 rule keeps its teeth: on the low-level rows (gain max|x| <=
          1000) at most 2 % of a row's samples may be undecided.
"""
import functools

import numpy as np

PERIODS, PTS = 28, 10000                                     # SINC_PERIODS, SINC_PERIOD_PTS (fractresampler.cpp:50-53)
LEN = PERIODS * PTS + 1                                      # SINC_LENGTH (:57)
MAXV = 32767.0                                               # MAX_SOUNDCARDVAL (:59)
U = 2.0 ** -24
CAP = 0.02
CHUNK = 1024                                                 # the sound-sink kernel's output times per LDS chunk

_table = None


def table():
    """Init's table (:101-114) in fp64"""
    global _table
    if _table is None:
        i = np.arange(LEN, dtype=np.float64)
        two_pi = 2.0 * np.pi
        w = (0.35875 - 0.48829 * np.cos((two_pi * i) / (LEN - 1)) + 0.14128 * np.cos((2.0 * two_pi * i) / (LEN - 1))
             - 0.01168 * np.cos((3.0 * two_pi * i) / (LEN - 1)))
        fi = np.pi * (i - LEN // 2) / PTS
        fi[LEN // 2] = 1.0
        _table = w * np.sin(fi) / fi
        _table[LEN // 2] = 1.0
    return _table


def time_chain(t, n, rate):
    """:157-178: the output times of a call of n input samples, and the accumulator it leaves behind"""
    times = []
    while int(t) < n:
        times.append(t)
        t += rate
    return np.array(times, dtype=np.float64), t - float(n)


def taps(times, width=PERIODS):
    """input positions j = (int)t + 1 .. + 28 in [history | call] and table indices (:165-168), per output"""
    it = times.astype(np.int64)
    j = it[:, None] + np.arange(1, width + 1)[None, :]
    k = ((j.astype(np.float64) - times[:, None]) * float(PTS)).astype(np.int64)
    return j, k


class Resampler:
    """One stream: real (n,) or two-component (n, 2) input (a complex128 array is taken as its re / im columns)"""

    def __init__(self):
        self.t = 0.0
        self.hist = np.zeros((PERIODS, 2))

    def resample(self, x, rate):
        """-> y, S of shape (nout,) for real input, (nout, 2) for complex input"""
        x = np.asarray(x)
        cpx = np.iscomplexobj(x) or x.ndim == 2
        if np.iscomplexobj(x):
            x = np.stack([x.real, x.imag], axis=1)
        x = x.astype(np.float64).reshape(len(x), 2 if cpx else 1)
        n = len(x)
        buf = np.zeros((PERIODS + n, 2))
        buf[:PERIODS] = self.hist
        buf[PERIODS:, :x.shape[1]] = x
        times, self.t = time_chain(self.t, n, float(rate))
        self.times = times
        if len(times):
            j, k = taps(times)
            p = buf[j] * table()[k][:, :, None]               # (nout, 28, 2)
            y, S = p.sum(axis=1), np.abs(p).sum(axis=1)
        else:
            y, S = np.zeros((0, 2)), np.zeros((0, 2))
        self.hist = buf[n:n + PERIODS].copy()                 # :179-182
        return (y, S) if cpx else (y[:, 0], S[:, 0])


def f32(x):
    """the nearest fp32 values, as fp64: the inputs of every rule here"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def float_ratio(got, y, S):
    """|got - y| / (30 u S) per sample; a tap window of zeros must give exactly 0"""
    got, y, S = (np.asarray(a, dtype=np.float64).ravel() for a in (got, y, S))
    err = np.abs(got - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S > 0, err / (30.0 * U * S), np.where(err > 0, np.inf, 0.0))
    return r


def word_bounds(y, S, gain):
    v, d = np.asarray(y) * gain, 32.0 * U * abs(gain) * np.asarray(S)
    lo = np.trunc(np.clip(v - d, -MAXV, MAXV)).astype(np.int64)
    hi = np.trunc(np.clip(v + d, -MAXV, MAXV)).astype(np.int64)
    return lo, hi


def undecided_share(y, S, gain):
    lo, hi = word_bounds(y, S, gain)
    return float((lo != hi).mean()) if lo.size else 0.0


def old_rule_ok(got, y, gain):
    """the rule the suite had before: within 1 LSB of the fp64 word"""
    want = np.trunc(np.clip(np.asarray(y) * gain, -MAXV, MAXV)).astype(np.int64)
    return bool((np.abs(np.asarray(got, dtype=np.int64).ravel() - want.ravel()) <= 1).all())


class Tally:
    """What one form did under the rules, summed over calls"""

    def __init__(self, name):
        self.name = name
        self.ratio = 0.0                  # largest err / (30 u S)
        self.nf = self.nw = 0             # float samples, words
        self.undecided = self.decided_equal = self.decided_clipped = 0
        self.bad_float = self.bad_decided = self.bad_undecided = 0

    def floats(self, got, y, S):
        r = float_ratio(got, y, S)
        assert r.shape == np.asarray(y).ravel().shape
        if r.size:
            self.ratio = max(self.ratio, float(r.max()))
        self.nf += r.size
        self.bad_float += int((r > 1.0).sum())
        return self

    def words(self, got, y, S, gain):
        got = np.asarray(got).astype(np.int64).ravel()
        lo, hi = (a.ravel() for a in word_bounds(y, S, gain))
        assert got.shape == lo.shape, (got.shape, lo.shape)
        dec = lo == hi
        self.nw += got.size
        self.undecided += int((~dec).sum())
        self.decided_equal += int((dec & (got == lo)).sum())
        self.decided_clipped += int((dec & (np.abs(lo) == int(MAXV))).sum())
        self.bad_decided += int((dec & (got != lo)).sum())
        self.bad_undecided += int((~dec & (got != lo) & (got != hi)).sum())
        return self

    @property
    def share(self):
        return self.undecided / self.nw if self.nw else 0.0

    @property
    def ok(self):
        return self.bad_float == 0 and self.bad_decided == 0 and self.bad_undecided == 0

    def __str__(self):
        s = "%s:" % self.name
        if self.nf:
            s += " %d float samples, largest err / (30 u S) = %.3f, %d over;" % (self.nf, self.ratio, self.bad_float)
        if self.nw:
            s += (" %d words, undecided %.3f %%, decided and equal %d of %d (%d clipped), undecided off lo/hi %d" %
                  (self.nw, 100.0 * self.share, self.decided_equal, self.nw - self.undecided, self.decided_clipped,
                   self.bad_undecided))
        return s


# ---------------------------------------------------------------------------------------------------------------
# the rows both test files use

IMPULSE_RATES = [1.0, 0.999871, 62500.0 / 48000.0, 11025.0 / 48000.0, 0.7312, 2.5]
IMPULSE_CALLS = (1400, 1371, 1325)                           # 4096 samples; an impulse sits in the last 28 of the first two


def impulse_train(n, offset=0, first=0):
    """impulses 29 samples apart, +-2^(1 + i mod 12), everything else exactly 0: at most one inside any 28-tap
    window, so every output is one table entry times a power of two and the sum rounds nothing"""
    x = np.zeros(n)
    pos = np.arange(offset, n, PERIODS + 1)
    i = np.arange(len(pos)) + first
    x[pos] = np.where(i % 2 == 0, 1.0, -1.0) * 2.0 ** (1 + i % 12)
    return x


def split(x, lengths):
    out, at = [], 0
    for n in lengths:
        out.append(x[at:at + n])
        at += n
    assert at <= len(x)
    return out


def row(kind, n, peak, seed):
    """a dense row of fp32 values with max|x| <= peak"""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        x = rng.standard_normal(n)
        x *= peak / np.abs(x).max()
    elif kind == "sine":
        x = peak * np.sin(2 * np.pi * (0.0137 + 0.001 * (seed % 7)) * np.arange(n) + 0.1 * seed)
    elif kind == "uniform":
        x = peak * rng.uniform(-1.0, 1.0, n)
    elif kind == "clip":                                     # a loud tone with some noise on it: clips at gain > 1.1
        x = 0.97 * peak * np.sin(2 * np.pi * 0.0071 * np.arange(n)) + 0.03 * peak * rng.uniform(-1.0, 1.0, n)
    else:
        raise ValueError(kind)
    x = f32(0.9999 * x)
    assert np.abs(x).max() <= peak
    return x


# dense rows of the one-stream and one-clock forms: (kind, rate, gain, peak); gain * peak <= 1000 except the clip row
DENSE = [("gauss", 0.7312, 0.64, 1500.0), ("sine", 62500.0 / 48000.0, 1.0, 1000.0), ("uniform", 2.5, 0.1, 10000.0),
         ("gauss", 0.23, 1.0, 1000.0), ("uniform", 1.0, 0.64, 1500.0), ("clip", 1.302, 1.7, 30000.0)]
EDGE = "edge"
RAGGED = (1, 1, 1, 27, 28, 29, 0, 2048)                      # the history slides by one three times, then around 28


def count_to(t, rate, want):
    """the shortest call that emits at least `want` samples from accumulator t (exactly `want` at rates >= 1)"""
    for _ in range(want - 1):
        t += rate
    return int(t) + 1


def dense_calls(rate, extra=()):
    """RAGGED, then the calls whose output counts are 256 and 257 (the block edge of the one-thread-per-output
    kernels), then `extra`: call lengths, or EDGE for another 256 / 257 pair"""
    t, calls = 0.0, []
    for item in RAGGED + (EDGE,) + tuple(extra):
        for n in ((256, 257) if item == EDGE else (item,)):
            if item == EDGE:
                n = count_to(t, rate, n)
            calls.append(n)
            t = time_chain(t, n, rate)[1]
    return tuple(calls)


def dense_row(kind, peak, seed, rate, extra=()):
    calls = dense_calls(rate, extra)
    return calls, split(row(kind, sum(calls), peak, seed), calls)


BATCH_RATES = [0.7312, 62500.0 / 48000.0, 2.5]
BATCH_GAIN = 0.64
BATCH_EXTRA = (2048, EDGE)                                    # float / int16 in turn: the second pair swaps the forms
BATCH_ROWS = [("gauss", 1500.0), ("sine", 1200.0), ("uniform", 1560.0), ("gauss", 300.0), ("clip", 80000.0)]


# ---------------------------------------------------------------------------------------------------------------
# the sound-sink run: six receivers, the same puts and gets on every side

SINK_RATES = [62500.0, 31250.0, 15625.37, 48000.0, 24000.0, 11025.0]
SINK_VOLUMES = [80, 99, 0, 90, 70, 75]                       # receiver 2 muted
SINK_KINDS = ["gauss", "sine", "uniform", "gauss", "sine", "uniform"]
_EDGE = [0, 1, 27, 28, 29, 1500]


def sink_gain(vol):
    """SetVolume (interface/soundout.cpp:180-189)"""
    return 0.0 if vol == 0 else 10.0 ** ((vol - 99.0) / 39.2)


def sink_plan():
    """("put", counts) / ("get", receiver, n).  Every side drains each receiver's queue after every put; the "get"
    events here are the long ones that run receiver 5's rate loop (the first update comes 6 s of consumed samples
    after the start-up, soundout.cpp:326-331, :456-468).
    Two puts take every queue past its start-up; six puts rotate 0, 1, 27, 28, 29, 1500 samples through the
    receivers (each in one batch); receiver 3 at 48 kHz gets exactly 1024 and then 2048 samples (output counts a
    multiple of the chunk: the kernel's last round is empty); receiver 5 at 11025 gets 3700 (16 chunks)."""
    ev = [("put", [5400, 5400, 2700, 4200, 4200, 1900]), ("put", [5400, 0, 0, 4200, 0, 0])]
    for p in range(6):
        ev.append(("put", [_EDGE[(c + p) % 6] for c in range(6)]))
    ev += [("put", [1500, 1500, 1500, 1024, 1500, 3700]), ("get", 5, 300000),
           ("put", [700, 300, 29, 2048, 1, 3700]), ("get", 5, 50000),
           ("put", [1, 27, 0, 1024, 28, 1000]), ("put", [29, 0, 1500, 1, 27, 28])]
    return ev


def sink_rows(stereo):
    """each receiver's whole stream, low under its volume: gain * max|x| <= 1000 (the muted one: 1000)"""
    total = [sum(e[1][c] for e in sink_plan() if e[0] == "put") for c in range(6)]
    rows = []
    for c in range(6):
        g = sink_gain(SINK_VOLUMES[c])
        peak = 1000.0 / g if g else 1000.0
        x = row(SINK_KINDS[c], total[c], peak, 100 + c)
        if stereo:
            x = np.stack([x, row(SINK_KINDS[(c + 1) % 6], total[c], peak, 200 + c)], axis=1)
        rows.append(x)
    return rows


# the clip run: three receivers loud enough that about half of every row saturates, no cap
CLIP_SINK_RATES = [62500.0, 48000.0, 11025.0]
CLIP_SINK_VOLUMES = [99, 90, 99]
CLIP_SINK_PEAKS = [60000.0, 80000.0, 60000.0]                # gain * peak = 60000, 47100, 60000


def clip_sink_plan():
    """two puts past every start-up (no queue overflows), then a chunk multiple, a short and a tiny row"""
    return [("put", [5400, 4200, 1900]), ("put", [5400, 4200, 1000]), ("put", [1500, 2048, 29])]


def clip_sink_rows(stereo):
    total = [sum(e[1][c] for e in clip_sink_plan()) for c in range(3)]
    rows = []
    for c in range(3):
        x = row("clip", total[c], CLIP_SINK_PEAKS[c], 400 + c)
        if stereo:
            x = np.stack([x, -row("clip", total[c], CLIP_SINK_PEAKS[c], 500 + c)[::-1]], axis=1)
        rows.append(x)
    return rows


class SinkDriver:
    """Replays puts and gets on one side and keeps, per receiver, one record per put: rate (read before the put),
    gain, input, resampled count, state after the put, and the resampled words.

    side: rate(c, r), volume(c, v), put(rows, counts) -> counts out, get(c, n) -> what was popped,
    state(c) -> (level, correction, fill average, ppm), and tap(c, k) -> the k words of receiver c's last put, or
    None when the side has no tap: then the words are read through the queue, which every put is followed by a get
    of the whole level for (silence, and nothing popped, while the sink is still starting up; the words then come
    with a later get)."""

    def __init__(self, side, rates, volumes, stereo):
        self.side, self.C, self.stereo = side, len(rates), stereo
        for c in range(self.C):
            side.rate(c, rates[c])
            side.volume(c, volumes[c])
        self.rates, self.volumes = list(rates), list(volumes)
        self.at = [0] * self.C
        self.log = [[] for _ in range(self.C)]
        self.pending = [[] for _ in range(self.C)]            # records whose words still sit in the queue

    def put(self, streams, counts):
        """the next counts[c] samples of every receiver's stream"""
        xs = [np.asarray(streams[c][self.at[c]:self.at[c] + counts[c]]) for c in range(self.C)]
        self.at = [self.at[c] + counts[c] for c in range(self.C)]
        self.put_rows(xs, counts, True)

    def put_rows(self, xs, counts, record):
        C, w = self.C, 2 if self.stereo else 1
        T = max(max(counts), 1)
        rows = np.zeros((C, T, w))
        rate = [self.rates[c] / 48000.0 * (1.0 + self.side.state(c)[1]) for c in range(C)]
        recs = []
        for c in range(C):
            x = xs[c].reshape(counts[c], w)
            rows[c, :counts[c]] = x
            recs.append(dict(rate=rate[c], gain=sink_gain(self.volumes[c]), x=x if self.stereo else x[:, 0],
                             corr=self.side.state(c)[1]))
        rows = (rows[:, :, 0] + 1j * rows[:, :, 1]).astype(np.complex64) if self.stereo else \
            rows[:, :, 0].astype(np.float32)
        k = self.side.put(rows, counts)
        for c in range(C):
            r = recs[c]
            r["k"] = int(k[c])
            r["words"] = self.side.tap(c, r["k"])
            if r["words"] is None:
                self.pending[c].append(r)
            self.drain(c)
            r["state"] = self.side.state(c)
            if record:
                self.log[c].append(r)

    def drain(self, c):
        L = self.side.state(c)[0]
        got = self.side.get(c, L)
        if L > 0 and self.side.state(c)[0] == L:              # start-up: silence, the words stay queued
            assert not got.any()
            return
        if self.pending[c]:
            n = sum(r["k"] for r in self.pending[c])
            assert L >= n, "a queue overflowed: the plan must keep every queue below its size"
            at = L - n
            for r in self.pending[c]:
                r["words"] = got[at:at + r["k"]].copy()
                at += r["k"]
            self.pending[c] = []

    def get(self, c, n):
        self.side.get(c, n)
        self.drain(c)

    def run(self, streams, events):
        for e in events:
            if e[0] == "put":
                self.put(streams, e[1])
            else:
                self.get(e[1], e[2])
        return self

    def flush(self):
        """silence, kept out of the log, until every queue has given out its pending words (a sink that never left
        its start-up)"""
        w = 2 if self.stereo else 1
        for _ in range(8):
            if not any(self.pending):
                return self
            counts = [int(min(8192, 6000 * self.rates[c] / 48000.0 + 1)) if self.pending[c] else 0
                      for c in range(self.C)]
            self.put_rows([np.zeros((counts[c], w)) for c in range(self.C)], counts, False)
        raise AssertionError("queues still hold words")


def sink_reference(log):
    """y, S of every put of one receiver's log (the rates, gains and inputs the oracle's run recorded)"""
    r = Resampler()
    out = []
    for rec in log:
        if len(rec["x"]) == 0:                                # no samples: the sink touches nothing
            out.append((np.zeros((0,) + rec["x"].shape[1:]),) * 2)
            continue
        out.append(r.resample(rec["x"], rec["rate"]))
    return out


class OracleSinks:
    """one oracle CSoundOut per receiver behind the SinkDriver's side interface"""

    def __init__(self, oracle, C, stereo):
        self.s = [oracle.CSoundOut(stereo) for _ in range(C)]

    def rate(self, c, r):
        self.s[c].ChangeUserDataRate(r)

    def volume(self, c, v):
        self.s[c].SetVolume(v)

    def put(self, rows, counts):
        return [self.s[c].PutOutQueue(rows[c, :counts[c]].astype(np.complex128 if np.iscomplexobj(rows) else np.float64))
                if counts[c] else 0 for c in range(len(self.s))]

    def get(self, c, n):
        return self.s[c].GetOutQueue(n)

    def state(self, c):
        s = self.s[c]
        return (s.level(), s.rate_correction(), s.ave_level(), s.ppm_error())

    def tap(self, c, k):
        return None


@functools.lru_cache(maxsize=None)
def oracle_sink_run(oracle, stereo, clip=False):
    """the sound-sink plan (or the clip plan) on the oracle's sinks: the log (rates, gains, counts, states, the
    oracle's words) and the fp64 reference of every put.  Computed once per form, shared by every test that needs
    it, never changed."""
    if clip:
        d = SinkDriver(OracleSinks(oracle, 3, stereo), CLIP_SINK_RATES, CLIP_SINK_VOLUMES, stereo)
        d.run(clip_sink_rows(stereo), clip_sink_plan())
    else:
        d = SinkDriver(OracleSinks(oracle, 6, stereo), SINK_RATES, SINK_VOLUMES, stereo)
        d.run(sink_rows(stereo), sink_plan())
    assert not any(d.pending)
    return d.log, [sink_reference(log) for log in d.log]
