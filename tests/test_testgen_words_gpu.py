"""The batch signal generator on the device (K9: testgen_kernel<0|1> through csdr_testgen_batch_generate / _generate_real)
under the K9 word rule of tests/k9_words.py: every receiver, the complex and the real form, three cuts of the same
8192-sample stream (one call per section, 256-sample calls, a ragged cut with odd counts and gaps in the row), slots
and a rate change between the calls, and the noise rows at two seeds.

  words       a decided word (fp32(y - delta) == fp32(y + delta)) equals the device word as a value; an undecided word
              lies in the interval; gate closed and noise off: zero of either sign
  cuts        the three cuts agree word for word
  not owned   a receiver that is off, a receiver's samples while it is off, the gaps between the calls and everything
              behind the last call keep their words bit for bit

The only tolerances are delta and the cap, both from k9_words.py, derived there; tests/test_testgen_words_host.py checks
the cap, the paths the streams take and what the rule catches.  Every test prints its figures per row."""
import numpy as np
import pytest

import k9_words as K
import testgen_ref as R
from test_testgen_gpu import pattern, words

pytestmark = pytest.mark.gpu


def generate(plan, cut, real):
    """the plan's stream through one TestGenBatch in the calls of a cut: (the stream's words as float64 (C, n, 1 | 2),
    the row words before, the row words after, a mask of the row words the calls own)"""
    import torch
    import cutesdr_amd as ca
    q = 4 if real else 2
    cs, width = K.calls(plan, cut, q)
    Cn = len(plan.receivers)
    rows = pattern(torch, (Cn, width + 8), torch.float32 if real else torch.complex64)
    before = words(rows).clone().cpu().numpy()
    g = ca.TestGenBatch(Cn)
    for c in range(Cn):
        R.configure(g, plan.receivers[c], channel=c, noise_db=plan.noise[c])
    g.SetSeed(plan.seed)
    for events, m, fs, _, off, _ in cs:
        for rc, name, v in events:
            R.slot(g, name, v, channel=rc)
        g.CreateGeneratorSamples(rows, m, fs, offset=off)
    torch.cuda.synchronize()
    after = words(rows).cpu().numpy()
    where, _ = K.positions(plan, cut, q)
    w = 1 if real else 2
    with np.errstate(invalid="ignore"):                                 # words nobody wrote are the pattern's, NaNs among them
        vals = after.view(np.float32).reshape(Cn, -1, w)[:, where, :].astype(np.float64)
    owned = np.zeros((Cn, after.reshape(Cn, -1, w).shape[1]), dtype=bool)
    for c in range(Cn):
        owned[c, where[K.reference(plan, c)["on"]]] = True
    return vals, before.reshape(Cn, -1, w), after.reshape(Cn, -1, w), owned


def check(plan, real):
    form = "real" if real else "complex"
    first = None
    for cut in K.CUTS:
        vals, before, after, owned = generate(plan, cut, real)
        assert np.array_equal(after[~owned], before[~owned]), (plan.name, form, cut)      # bit for bit
        assert owned.any(axis=1).sum() == sum(1 for r in plan.receivers if r[6])
        for c in range(len(plan.receivers)):
            d = K.reference(plan, c)
            if not d["on"].any():
                assert np.array_equal(after[c], before[c])
                continue
            t = K.Tally("%s receiver %d %s, cut %s" % (plan.name, c, form, cut), d, real, vals[c])
            print(t)
            assert t.ok, str(t)
            assert t.share <= K.CAP
        on = np.stack([K.reference(plan, c)["on"] for c in range(len(plan.receivers))])
        bits = vals.astype(np.float32).view(np.int32)[on]               # compared as words: the sign of a zero included
        if first is None:
            first = bits
        assert np.array_equal(bits, first), (plan.name, form, cut)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_every_receiver_three_cuts(real):
    check(K.MAIN, real)


@pytest.mark.parametrize("seed", K.NOISE_SEEDS)
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_noise_rows(real, seed):
    """signal -160 dB under noise at -70 and -20 dB, a full-scale tone and a gated one under noise at -40 dB: nearly
    every word is decided, so this compares bit for bit with fp32 of the reference"""
    check(K.NOISE[seed], real)
    for c in (0, 1):
        d = K.reference(K.NOISE[seed], c)
        assert max(K.undecided_share(d, real)) <= 0.001
