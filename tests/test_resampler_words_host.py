"""The K5 word rule (tests/resampler_ref.py) on the CPU: the fp64 helper against the oracle's CFractResampler, a
numpy fp32 model of the kernels' arithmetic that passes the rule, six wrong models that fail it -- four of which the
old "+-1 LSB" rule lets through -- and the cap (at most 2 % undecided words) on every low-level row that
tests/test_resampler_words_gpu.py uses, from the reference alone."""
import numpy as np
import pytest

import resampler_ref as R


# --------------------------------------------------------------------------------------------------------------
# the helper against the oracle

@pytest.mark.parametrize("rate", [1.0, 0.7312, 62500.0 / 48000.0, 0.23, 2.5])
def test_helper_matches_the_oracle(oracle, rate):
    """Counts equal, float outputs within 1e-12 S (libm differences in the table), the oracle's own fp64 words under
    the int16 rule, all four overloads, a ragged call sequence with n = 0, 1, 27, 28, 29."""
    calls = (300, 0, 1, 27, 28, 29, 1, 1, 0, 700, 28, 513)
    rng = np.random.default_rng(5)
    x = R.f32(3000.0 * rng.standard_normal(sum(calls)))
    xc = x + 1j * R.f32(3000.0 * rng.standard_normal(sum(calls)))
    for data, gain in ((x, None), (xc, None), (x, 0.64), (xc, 1.7)):
        o, h = oracle.CFractResampler(), R.Resampler()
        o.Init(4096)
        t = R.Tally("helper vs oracle, rate %g" % rate)
        worst = 0.0
        for part in R.split(data, calls):
            want = o.Resample(part, rate, gain)
            y, S = h.resample(part, rate)
            assert len(want) == len(y)
            if gain is None:
                w = np.stack([want.real, want.imag], axis=1) if np.iscomplexobj(want) else want
                if len(y):
                    assert (np.abs(w - y) <= 1e-12 * S).all()
                    worst = max(worst, float((np.abs(w - y) / np.maximum(S, 1e-300)).max()))
            else:
                t.words(want, y, S, gain)
        if gain is None:
            print("helper vs oracle, rate %g, %s: largest |diff| / S = %.2e" % (rate, data.dtype, worst))
        else:
            print(t)
            assert t.ok and t.nw > 500


def test_the_impulse_trains_reach_into_the_history():
    x, at = R.impulse_train(4096), 0
    for n in R.IMPULSE_CALLS[:2]:
        at += n
        assert x[at - R.PERIODS:at].any()                      # the next call reads this impulse from the history
    assert sum(R.IMPULSE_CALLS) == 4096 and np.count_nonzero(x) == 142


def test_the_batch_calls_cross_the_block_edge_in_both_forms():
    """float on even calls, int16 on odd ones: 256 outputs as float and as int16, 257 likewise"""
    for rate in R.BATCH_RATES:
        calls = R.dense_calls(rate, R.BATCH_EXTRA)
        t, counts = 0.0, []
        for n in calls:
            times, t = R.time_chain(t, n, rate)
            counts.append(len(times))
        assert len(calls) == 13 and calls[7] == calls[10] == 2048
        if rate >= 1.0:
            assert counts[8:10] == [256, 257] and counts[11:13] == [256, 257]
        else:
            assert 256 <= min(counts[8], counts[11]) and max(counts[9], counts[12]) <= 263


def test_helper_table_and_anchor():
    tab = R.table()
    assert len(tab) == 280001 and tab[140000] == 1.0 and abs(tab[150000]) < 1e-15 and tab[0] == pytest.approx(0.0, abs=1e-9)
    h = R.Resampler()
    y, _ = h.resample(np.ones(4096), 1.6276)
    assert len(y) == 2517                                       # the reference's own anchor for 4096 samples


# --------------------------------------------------------------------------------------------------------------
# the fp32 model of the kernels and its faults

class Model:
    """resample_kernel / resample_batch_kernel / soundsink_batch_kernel in numpy: fp32 table, the index in fp64, a
    sequential fp32 sum, fp32 gain, clip, truncate.  fault: None or one of FAULTS."""

    def __init__(self, fault=None):
        self.fault, self.t = fault, 0.0
        self.hist = np.zeros((R.PERIODS, 2), dtype=np.float32)
        self.tab = R.table().astype(np.float32)

    def resample(self, x, rate, gain=None):
        x = np.asarray(x)
        cpx = np.iscomplexobj(x)
        x = (np.stack([x.real, x.imag], axis=1) if cpx else x.reshape(-1, 1)).astype(np.float32)
        n = len(x)
        buf = np.zeros((R.PERIODS + n, 2), dtype=np.float32)
        buf[:R.PERIODS] = self.hist
        buf[R.PERIODS:, :x.shape[1]] = x
        times, self.t = R.time_chain(self.t, n, rate)
        if self.fault == "chunk restart":                       # every chunk after the first starts the chain again
            for s in range(R.CHUNK, len(times), R.CHUNK):       # from the first chunk's first entry
                m = len(times[s:s + R.CHUNK])
                times[s:s + m] = times[:m]
        self.hist = buf[n:n + R.PERIODS].copy()
        if not len(times):
            return np.zeros((0, 2) if cpx else 0, dtype=np.float32 if gain is None else np.int16)
        j, k = R.taps(times)
        if self.fault == "index + 1":
            k = np.minimum(k + 1, R.LEN - 1)
        if self.fault == "history off by one":
            j = np.where(j < R.PERIODS, np.minimum(j + 1, R.PERIODS - 1), j)
        acc = np.zeros((len(times), 2), dtype=np.float32)
        for i in range(R.PERIODS):
            acc = acc + buf[j[:, i]] * self.tab[k[:, i]][:, None]
        assert acc.dtype == np.float32
        if gain is None:
            return acc if cpx else acc[:, 0]
        g = np.float32(gain * {"gain 1e-4": 1.0 + 1e-4, "gain 1e-5": 1.0 + 1e-5}.get(self.fault, 1.0))
        v = np.clip(acc * g, np.float32(-R.MAXV), np.float32(R.MAXV))
        assert v.dtype == np.float32
        w = (np.rint(v) if self.fault == "rounds" else np.trunc(v)).astype(np.int16)
        return w if cpx else w[:, 0]


def run_model(fault, kind, rate, gain, peak, seed=1, cpx=False, extra=()):
    """one dense row through the model, float and int16 form: the tally, and whether the old rule would pass"""
    calls, parts = R.dense_row(kind, peak, seed, rate, extra)
    if cpx:
        parts = [p + 1j * q for p, q in zip(parts, R.dense_row(kind, peak, seed + 50, rate, extra)[1])]
    mf, mi, h = Model(fault), Model(fault), R.Resampler()
    t = R.Tally("%s model, %s rate %g gain %g peak %g%s" % (fault or "right", kind, rate, gain, peak, " complex" if cpx else ""))
    old = True
    for p in parts:
        y, S = h.resample(p, rate)
        t.floats(mf.resample(p, rate), y, S)
        w = mi.resample(p, rate, gain)
        t.words(w, y, S, gain)
        old &= R.old_rule_ok(w, y, gain)
    return t, old


@pytest.mark.parametrize("cpx", [False, True], ids=["real", "complex"])
def test_right_model_passes_both_rules(cpx):
    worst = 0.0
    for kind, rate, gain, peak in R.DENSE:
        t, old = run_model(None, kind, rate, gain, peak, cpx=cpx)
        print(t)
        assert t.ok and old, str(t)
        worst = max(worst, t.ratio)
    print("right model: largest err / (30 u S) = %.3f" % worst)
    x = R.impulse_train(4096)
    for rate in R.IMPULSE_RATES:                                # the impulse train: model == fp32(fp64) on every word
        m, h = Model(), R.Resampler()
        for p in R.split(x, R.IMPULSE_CALLS):
            y, _ = h.resample(p, rate)
            assert np.array_equal(m.resample(p, rate), y.astype(np.float32)), rate


# fault -> the row it is asserted on (kind, rate, gain, peak, extra calls), chosen here on the CPU so that decided words
# differ, and whether the old +-1 LSB rule lets it through on that row
FAULTS = {
    "rounds": (("gauss", 0.7312, 0.64, 1500.0, ()), True),
    "index + 1": (("sine", 62500.0 / 48000.0, 1.0, 1000.0, ()), True),
    "gain 1e-4": (("gauss", 0.7312, 0.64, 1500.0, ()), True),
    "gain 1e-5": (("uniform", 2.5, 0.1, 10000.0, (4096,)), True),
    "history off by one": (("gauss", 0.7312, 0.64, 1500.0, ()), None),
    "chunk restart": (("gauss", 0.7312, 0.64, 1500.0, ()), None),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_wrong_models_fail(fault):
    """Each fault breaks decided words on its row; the plain ones pass the rule the suite had before.  The first
    four are arithmetic faults (the float form sees only the table index); the last two are addressing faults
    (the history branch j < 28 of the short calls; the 2048-sample call's second and third chunk of times)."""
    (kind, rate, gain, peak, extra), old_passes = FAULTS[fault]
    right, _ = run_model(None, kind, rate, gain, peak, extra=extra)
    t, old = run_model(fault, kind, rate, gain, peak, extra=extra)
    print(t)
    print("%s: decided words that differ %d of %d, float samples over the bound %d, old rule passes: %s" %
          (fault, t.bad_decided, t.nw - t.undecided, t.bad_float, old))
    assert right.ok
    assert t.bad_decided >= 3, str(t)
    if fault in ("index + 1", "history off by one", "chunk restart"):
        assert t.bad_float > 0 and t.ratio > 100.0
    else:
        assert t.bad_float == 0                                 # the gain and the conversion are not in the float form
    if old_passes is not None:
        assert old == old_passes


def test_chunk_restart_needs_a_row_longer_than_a_chunk():
    """why the sink rows go past 1024 outputs: the fault is invisible on shorter calls"""
    h, m = R.Resampler(), Model("chunk restart")
    x = R.row("gauss", 700, 1000.0, 3)
    y, S = h.resample(x, 0.7312)
    assert len(y) < R.CHUNK and R.Tally("short").words(m.resample(x, 0.7312, 1.0), y, S, 1.0).ok


# --------------------------------------------------------------------------------------------------------------
# the cap, from the reference alone, on every low-level row of the GPU tests

def test_cap_on_the_dense_rows():
    for kind, rate, gain, peak in R.DENSE:
        for seed in (1, 51):                                    # the real rows / re parts, the im parts
            calls, parts = R.dense_row(kind, peak, seed, rate)
            h = R.Resampler()
            out = [h.resample(p, rate) for p in parts]
            y, S = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
            share = R.undecided_share(y, S, gain)
            print("%s rate %g gain %g peak %g seed %d: %d words, undecided %.3f %%" % (kind, rate, gain, peak, seed, len(y), 100 * share))
            if kind != "clip":
                assert gain * peak <= 1000.0 and share <= R.CAP
            else:
                lo, hi = R.word_bounds(y, S, gain)
                assert ((lo == hi) & (np.abs(lo) == 32767)).mean() >= 0.10


def test_cap_on_the_batch_rows():
    for rate in R.BATCH_RATES:
        for c, (kind, peak) in enumerate(R.BATCH_ROWS):
            calls, parts = R.dense_row(kind, peak, 300 + c, rate, extra=R.BATCH_EXTRA)
            h = R.Resampler()
            out = [h.resample(p, rate) for p in parts]
            y, S = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
            share = R.undecided_share(y, S, R.BATCH_GAIN)
            print("batch row %d (%s) rate %g: %d words, undecided %.3f %%" % (c, kind, rate, len(y), 100 * share))
            if kind != "clip":
                assert R.BATCH_GAIN * peak <= 1000.0 and share <= R.CAP
            else:
                lo, hi = R.word_bounds(y, S, R.BATCH_GAIN)
                assert ((lo == hi) & (np.abs(lo) == 32767)).mean() >= 0.10


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_sink_plan_and_cap(oracle, stereo):
    """The plan does what it is for -- helper counts equal the oracle's at every put, the oracle's own words pass the
    rule, receiver 3's counts are whole chunks, receiver 5 crosses 15 chunk boundaries in a put and runs under a
    non-zero correction for at least two puts -- and every receiver's undecided share is within the cap."""
    log, ref = R.oracle_sink_run(oracle, stereo)
    for c in range(6):
        t = R.Tally("oracle sink, receiver %d" % c)
        for rec, (y, S) in zip(log[c], ref[c]):
            assert rec["k"] == len(y), (c, rec["k"], len(y))
            t.words(rec["words"], y, S, rec["gain"])
        print(t)
        assert t.ok and t.share <= R.CAP and t.nw > 10000
    assert {len(r["x"]) for r in log[0]} >= {0, 1, 27, 28, 29, 1500}
    k3 = [(len(r["x"]), r["k"]) for r in log[3] if len(r["x"]) in (1024, 2048)]
    assert [n for n, _ in k3] == [1024, 2048, 1024] and all(n == k for n, k in k3)
    assert max(r["k"] for r in log[5]) > 15 * R.CHUNK
    corr = [r["corr"] for r in log[5] if r["corr"] != 0.0 and len(r["x"])]
    assert len(corr) >= 2 and len(set(corr)) >= 2, corr
    assert all(r["corr"] == 0.0 for c in range(5) for r in log[c])
    assert not np.concatenate([r["words"].ravel() for r in log[2]]).any()       # the muted receiver


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_sink_clip_plan(oracle, stereo):
    """The clip rows of the sinks: the oracle's own words pass the rule with no cap, at least 10 % of every receiver's
    words are decided and clipped, both signs, and no queue overflowed (the single sink's words come through it)."""
    log, ref = R.oracle_sink_run(oracle, stereo, clip=True)
    for c in range(3):
        t = R.Tally("oracle sink, clip receiver %d" % c)
        for rec, (y, S) in zip(log[c], ref[c]):
            assert rec["k"] == len(y)
            t.words(rec["words"], y, S, rec["gain"])
        print(t)
        assert t.ok and t.decided_clipped >= 0.10 * t.nw and t.nw > 5000
        w = np.concatenate([r["words"].ravel() for r in log[c]])
        assert (w == 32767).any() and (w == -32767).any() and np.abs(w.astype(np.int32)).max() == 32767
        assert R.sink_gain(R.CLIP_SINK_VOLUMES[c]) * R.CLIP_SINK_PEAKS[c] > 1.4 * 32767
