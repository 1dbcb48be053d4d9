"""The batch signal generator on the device (csdr_testgen_batch, K9) against the restatement of the reference's test
bench in testgen_ref.py: parity with the noise off, cut invariance, the noise source, and the generated rows as input
of the display FFT and of the batch chain.

Run with -s for the per-receiver figures; HISTORY.md has them and the timing table of tools/bench_testgen.py."""
import json
import math
import os

import numpy as np
import pytest

import testgen_ref as R
from util_signals import FULL_SCALE

pytestmark = pytest.mark.gpu

K2_TOL = 1e-5 * FULL_SCALE               # the input-rate stage these rows feed
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_anchors.json")))


def pattern(torch, shape, dtype):
    """rows pre-filled with distinct words (compared as integers: some are NaNs)"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    w = t.view(torch.float32).view(torch.int32)
    w.copy_((torch.arange(w.numel(), device="cuda", dtype=torch.int64) * 2654435761 % 2147483647).to(torch.int32).view(w.shape))
    return t


def words(t):
    import torch
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def batch(ca, noise_db=None, seed=None, channels=16):
    g = ca.TestGenBatch(channels)
    for c in range(channels):
        R.configure(g, R.RECEIVERS[c], channel=c, noise_db=noise_db)
    if seed is not None:
        g.SetSeed(seed)
    return g


def run_cuts(g, rows, cuts, rates, events=None):
    pos = 0
    for k, n in enumerate(cuts):
        for rc, name, v in (events or {}).get(k, ()):
            R.slot(g, name, v, channel=rc)
        g.CreateGeneratorSamples(rows, n, rates[k], offset=pos)
        pos += n
    return pos


# ------------------------------------------------------------------------------------------------- 6 parity
def test_parity_with_restatement_noise_off():
    """16 receivers with different parameters in one object, 2^21 samples each in uneven calls (2, 2^20, odd multiples
    of 2), slots between calls, a rate change in mid-stream, against the restatement driven in 256-sample calls: every
    sample within 1e-5 of full scale; rows and samples the generator does not own stay bit for bit.
    Measured on an MI355X: maximum 0.0019 counts = 5.9e-8 of full scale (receiver 1; the others about 0.0010 counts),
    which is what fp32 rounding of amp * cos alone allows (2e-3 counts): a margin of 170 to the tolerance."""
    import torch
    import cutesdr_amd as ca
    n, pad = sum(R.CUTS), 8
    rows = pattern(torch, (16, n + pad), torch.complex64)
    before = words(rows).clone()
    g = batch(ca)
    assert run_cuts(g, rows, R.CUTS, R.RATES, R.EVENTS) == n
    torch.cuda.synchronize()
    after = words(rows)
    assert torch.equal(after[:, n:], before[:, n:])                            # sample counts: nothing behind n
    assert torch.equal(after[9], before[9])                                     # the receiver that is off
    worst = 0.0
    for c in range(16):
        if c == 9:
            continue
        ref = R.ref_stream(c)
        dev = rows[c, :n].cpu().numpy().astype(np.complex128)
        off = np.isnan(ref.real)                                                # receiver 15 is off for one call
        assert off.any() == (c == 15)
        assert np.array_equal(after[c, :n].cpu().numpy()[off], before[c, :n].cpu().numpy()[off])
        d = dev[~off] - ref[~off]
        err = max(np.abs(d.real).max(), np.abs(d.imag).max())
        print("receiver %2d: max error %.3g counts = %.3g of full scale" % (c, err, err / FULL_SCALE))
        worst = max(worst, err)
        assert err <= K2_TOL, (c, err)
    print("parity, noise off: max error %.3g counts = %.3g of full scale (tolerance %.3g)" % (worst, worst / FULL_SCALE, 1e-5))


def test_parity_real_overload():
    """the TYPEREAL overload (3 * amp * cos, same state machine) over 2^18 samples of every receiver"""
    import torch
    import cutesdr_amd as ca
    cuts = [4, 1 << 17, 12, 1020, 65532, (1 << 18) - (4 + (1 << 17) + 12 + 1020 + 65532)]
    n = sum(cuts)
    rows = pattern(torch, (16, n + 8), torch.float32)
    before = words(rows).clone()
    g = batch(ca)
    run_cuts(g, rows, cuts, [R.FS1] * len(cuts))
    torch.cuda.synchronize()
    assert torch.equal(words(rows)[:, n:], before[:, n:]) and torch.equal(words(rows)[9], before[9])
    for c in range(16):
        if c == 9:
            continue
        ref = R.ref_stream(c, real=True, cuts=cuts, rates=[R.FS1] * len(cuts), events={})
        err = np.abs(rows[c, :n].cpu().numpy().astype(np.float64) - ref).max()
        assert err <= 3.0 * K2_TOL, (c, err)                                    # the real form's full scale is 3 x 32767


# ------------------------------------------------------------------------------------------------- 7 cut invariance
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_cut_invariance_noise_on(real):
    """one call of 2^20 = 4096 calls of 256 = a ragged cut, word for word, all 16 receivers with noise at -40 dB"""
    import torch
    import cutesdr_amd as ca
    n = 1 << 20
    q = 4 if real else 2
    ragged = [q, 3 * q, 511 * q, 32767 * q, 131073 * q]
    ragged.append(n - sum(ragged))
    outs = []
    for cuts in ([n], [256] * (n // 256), ragged):
        g = batch(ca, noise_db=-40.0, seed=7)
        g.OnGenOn(True, channel=9)
        rows = torch.zeros((16, n), dtype=torch.float32 if real else torch.complex64, device="cuda")
        run_cuts(g, rows, cuts, [R.FS1] * len(cuts))
        torch.cuda.synchronize()
        outs.append(rows)
    assert torch.equal(words(outs[0]), words(outs[1]))
    assert torch.equal(words(outs[0]), words(outs[2]))
    assert float(outs[0].abs().max()) > 1000.0


# ------------------------------------------------------------------------------------------------- 8 noise
def test_noise_against_restatement_and_moments():
    """signal -160 dB (3.3e-4 counts, kept in the restatement), noise -70 / -20 dB.  ln and sqrt run in fp64 on the
    device, so every sample is within 1e-5 * noise amplitude * max(1, |value| / noise amplitude) of the numpy
    restatement (a sample that took another attempt than the restatement is off by the order of the amplitude)."""
    import torch
    import cutesdr_amd as ca
    n, fs = R.NOISE_N, R.FS1
    outs = {}
    for seed in R.NOISE_SEEDS + (R.NOISE_SEEDS[0],):
        g = ca.TestGenBatch(4)
        g.OnGenOn(True); g.OnPulseWidth(0.0); g.OnSweepStart(10000.0); g.OnSweepStop(10000.0); g.OnSignalPwr(-160.0)
        for c, db in enumerate((-70.0, -20.0, -160.0, -20.0)):
            g.OnNoisePwr(db, channel=c)
        g.SetSeed(seed)
        rows = torch.zeros((4, n), dtype=torch.complex64, device="cuda")
        g.CreateGeneratorSamples(rows, n // 2, fs)
        g.CreateGeneratorSamples(rows, n // 2, fs, offset=n // 2)
        torch.cuda.synchronize()
        if seed in outs:                                                        # the same seed twice: the same words
            assert torch.equal(words(rows), words(outs[seed]))
            continue
        outs[seed] = rows
        for c, db in enumerate((-70.0, -20.0, -160.0, -20.0)):
            r = R.RefTestBench(seed=seed, channel=c)
            r.OnGenOn(True); r.OnPulseWidth(0.0); r.OnSweepStart(10000.0); r.OnSweepStop(10000.0); r.OnSignalPwr(-160.0)
            r.OnNoisePwr(db)
            ref = np.concatenate([r.create(256, fs) for _ in range(n // 256)])
            dev = rows[c].cpu().numpy().astype(np.complex128)
            namp = FULL_SCALE * 10.0 ** (db / 20.0)
            for d, v in ((dev.real - ref.real, ref.real), (dev.imag - ref.imag, ref.imag)):
                assert (np.abs(d) <= 1e-5 * namp * np.maximum(1.0, np.abs(v) / namp)).all(), (seed, c)
            if db == -160.0:                                                    # exactly -160 dB adds nothing (:433)
                assert np.abs(dev).max() <= FULL_SCALE * 1e-8 * 1.0001
                continue
            for k, (v, bound) in R.moments_ok(dev.real, dev.imag, namp).items():
                assert v <= bound, (seed, c, k, v, bound)
    lim = 6.0 / math.sqrt(n)
    a, b = (outs[s].cpu().numpy() for s in R.NOISE_SEEDS)
    assert abs(np.corrcoef(a[1].real, a[3].real)[0, 1]) <= lim                  # different receivers
    assert abs(np.corrcoef(a[0].real, a[1].imag)[0, 1]) <= lim
    assert abs(np.corrcoef(a[1].real, b[1].real)[0, 1]) <= lim                  # different seeds
    assert abs(np.corrcoef(a[3].imag, b[3].imag)[0, 1]) <= lim


# ------------------------------------------------------------------------------------------------- 9 through the product
def test_display_anchor_c1_from_generated_rows():
    """a -20 dB tone at +250 kHz, Fs 2 MHz, generated on the device, into the batch display FFT
    (4096 points, ave 1, dB compensation 0): index 2560, -1.3982 bels within K3's 0.01 dB"""
    import torch
    import cutesdr_amd as ca
    i, e = GOLDEN["display_fft_c1"]["input"], GOLDEN["display_fft_c1"]["expect"]
    g = ca.TestGenBatch(1)
    g.OnGenOn(True); g.OnPulseWidth(0.0); g.OnSweepStart(i["tone_hz"]); g.OnSweepStop(i["tone_hz"]); g.OnSweepRate(0.0)
    g.OnSignalPwr(-20.0); g.OnNoisePwr(-160.0)
    rows = torch.zeros((1, i["n"]), dtype=torch.complex64, device="cuda")
    g.CreateGeneratorSamples(rows, i["n"], i["fs"])
    f = ca.FftBatch(1)
    f.set_params(i["n"], False, i["db_comp"], i["fs"]); f.set_ave(i["ave"])
    f.put_display_ptr(rows.data_ptr(), rows.stride(0), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a = f.ave_buf(0)
    assert int(np.argmax(a)) == e["peak_index"] == 2560
    assert a[2560] == pytest.approx(e["peak_bels"], abs=0.001)                  # K3: 0.01 dB


def test_generated_rows_are_ordinary_chain_input():
    """the generator's buffer into csdr_demod_batch_process gives, word for word, what a device-to-device copy of it gives"""
    import torch
    import cutesdr_amd as ca
    from test_postchain_gpu import MODES, info
    C, T, fs = 3, 1 << 17, R.FS1
    g = ca.TestGenBatch(C)
    g.OnGenOn(True); g.OnPulseWidth(0.0); g.OnSignalPwr(-10.0); g.OnNoisePwr(-60.0)
    for c, hz in enumerate((100500.0, 101000.0, 99000.0)):
        g.OnSweepStart(hz, channel=c); g.OnSweepStop(hz + 2000.0, channel=c); g.OnSweepRate(20000.0, channel=c)
    rows = torch.zeros((C, T), dtype=torch.complex64, device="cuda")
    g.CreateGeneratorSamples(rows, T, fs)
    copy = rows.clone()
    outs = []
    for x in (rows, copy):
        b = ca.DemodBatch(C, 2048); b.set_input_rate(fs)
        for c, name in enumerate(("FM", "AM", "USB")):
            m, kw = MODES[name]
            b.set_demod(c, m, info(ca, **kw))
        b.commit()
        for c in range(C):
            b.set_freq(c, -100e3)
        cap = T // 8 + 2048 + 4096
        out = torch.zeros((C, cap), dtype=torch.float32, device="cuda")
        b.process_ptr(x.data_ptr(), x.stride(0), T, out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        counts = [b.out_count(c) for c in range(C)]
        outs.append((counts, out))
    assert outs[0][0] == outs[1][0] and min(outs[0][0]) > 0
    assert torch.equal(words(outs[0][1]), words(outs[1][1]))
    assert float(outs[0][1].abs().max()) > 0.0


def test_pulse_through_the_blanker():
    """a pulse-gated receiver through csdr_noiseproc_batch_process: the blanked positions equal those on the
    restatement's samples"""
    import torch
    import cutesdr_amd as ca
    n, fs = 1 << 18, R.FS1
    g = ca.TestGenBatch(1)
    g.OnGenOn(True); g.OnSweepStart(50000.0); g.OnSweepStop(50000.0); g.OnPulseWidth(0.00001); g.OnPulsePeriod(0.02)
    g.OnNoisePwr(-60.0); g.SetSeed(3)
    rows = torch.zeros((1, n), dtype=torch.complex64, device="cuda")
    g.CreateGeneratorSamples(rows, n, fs)
    torch.cuda.synchronize()
    r = R.RefTestBench(seed=3)
    r.OnGenOn(True); r.OnSweepStart(50000.0); r.OnSweepStop(50000.0); r.OnPulseWidth(0.00001); r.OnPulsePeriod(0.02)
    r.OnNoisePwr(-60.0)
    ref = np.concatenate([r.create(256, fs) for _ in range(n // 256)]).astype(np.complex64)
    outs = []
    for x in (rows.cpu().numpy(), ref[None, :]):
        nb = ca.NoiseProcBatch(1); nb.setup(True, 30.0, 50.0, fs)
        outs.append(nb.process(x))
    blank = [np.nonzero(o[0] == 0)[0] for o in outs]                           # the noise leaves no other zeros
    assert (blank[0] > 40000).any() and np.array_equal(blank[0], blank[1])


def test_rejects_misaligned_rows():
    import torch
    import cutesdr_amd as ca
    g = ca.TestGenBatch(2)
    g.OnGenOn(True)
    rows = torch.zeros((2, 1025), dtype=torch.complex64, device="cuda")
    with pytest.raises(ca._capi.CsdrError):
        g.CreateGeneratorSamples(rows, 512, R.FS1)                              # odd stride
    rows = torch.zeros((2, 1024), dtype=torch.complex64, device="cuda")
    with pytest.raises(ca._capi.CsdrError):
        g.CreateGeneratorSamples(rows, 512, R.FS1, offset=1)                    # row start not 16-byte aligned
    with pytest.raises(ca._capi.CsdrError):
        g.generate_ptr(rows.data_ptr(), 1024, 2048, R.FS1)                      # n > stride
    g.CreateGeneratorSamples(rows, 511, R.FS1)                                  # an odd count is fine
    torch.cuda.synchronize()
    assert float(rows[:, 510].abs().min()) > 0 and float(rows[:, 511:].abs().max()) == 0.0
