"""The batch chain behind the 16384-point band-pass filter -- fastfir_os2_kernel<14> on real gains -- against the fp64
oracle, with receivers that move between plan groups.  The chain is the one caller of that kernel with staged input (a
fill that is never empty here), channel strides unequal to the call length, hop counts that change from call to call
(1 to 4 hops of 8192: 262144 input samples each at / 32) and csdr__fastfir_batch_copy_row, which has to take the
overlap, both orders of the complex response AND the gains along.

The rig, the taps check and the Track rules are tests/test_batch_control_combinations_gpu.py's, on bursts of 8192
samples: an allowance given there as a count of 1024-sample bursts keeps its length in samples (rounded up to whole
bursts), and the first burst of a stream has the bound startup_bounds.first_burst_16k derives on the oracle alone.

What differs from the 2048-point scenarios, and why: a receiver goes into a muted row only where the staging fills
agree (batch_move_row).  At 2048 points those tests keep every fill empty; here a group that decimates by 64 holds
312 W mod 8192 samples after W windows and one that decimates by 32 holds 624 W mod 8192 -- equal only when W is a
multiple of 1024 -- so AM -> USB opens a group although the USB group has a muted row (asserted from the fills), and the
move INTO a muted row is the one by rate: a USB receiver in the FM group's row has had that group's decimation, hence
its fill, all along."""
import numpy as np
import pytest
from test_postchain_gpu import info
from test_batch_control_combinations_gpu import Rig, _signal, _check_taps, _info_kw, _form, FS, FS_ALT, LIM, KIND_OF
from test_set_demod_many_gpu import _many, NEW_EDGES

pytestmark = pytest.mark.gpu

NFFT, HOP = 16384, 8192
#         0      1      2      3      4      5      6      7      8     9     10    11
NAMES = ["USB", "LSB", "USB", "LSB", "USB", "LSB", "USB", "LSB", "FM", "FM", "AM", "SAM"]
WINDOWS = [32, 16, 16, 32, 16, 32, 32, 48, 16]          # call lengths in m_InBufLimit windows: {16, 32, 48} x LIM


def _fills(windows, per_window):
    """(hops, staging fill behind the call) of every call for a group that gets per_window samples per window"""
    tot = done = 0
    out = []
    for w in windows:
        tot += per_window * w
        out.append((tot // HOP - done, tot % HOP))
        done = tot // HOP
    return out


def test_call_lengths_give_one_to_four_hops_and_fills_that_never_empty_or_agree():
    by32, by64 = _fills(WINDOWS, LIM // 32), _fills(WINDOWS, LIM // 64)
    assert {h for h, _ in by32} == {1, 2, 3, 4}
    assert all(f > 0 for _, f in by32) and all(f > 0 for _, f in by64)
    assert all(a[1] != b[1] for a, b in zip(by32, by64))


def test_chain_at_16384_points_with_receivers_that_move(oracle):
    """Strict mode, set_taps(7), 2 MSPS, twelve receivers: the eight SSB ones are one plan group of eight rows (the kernels'
    (channels & 7) == 0 index mapping; it keeps eight rows when receivers leave), two FM, and AM + SAM (/ 64).  Events, each
    in front of the call named:
      2  USB -> AM for receiver 2: a group of its own;
      3  AM -> USB for receiver 10: the USB group's muted row has another fill -- a group of its own;
      4  new edges for receiver 4 through set_demod_many (designed on the device, never flushed) and, in the same gap,
         USB -> AM: copy_row has to fetch a response that exists on the device only;
      5  FM -> USB for receiver 9, in place (the same decimation at 2 MSPS);
      6  new edges for 8 and 9 through set_demod_many, then 2 -> 3.2 MSPS in the same gap: FM now decimates by 64, receiver
         9 does not and moves into the muted row receiver 2 left -- SetInputSampleRate designs nothing, so the response
         and the gains the row runs on from here are the ones copy_row brought, fetched from the device;
      7  back to 2 MSPS;
      8  FM -> AM for receiver 8: a group of its own, and the FM group, all rows muted, is dropped.
    After every call every receiver's taps 1-3 and its audio against its own oracle CDemodulator(16384).

    Every row is ONE stream cut into the calls, not a signal started again with every call as in the 2048-point tests:
    a carrier that jumps in phase at a call boundary rings through the 8193 taps for a whole burst with the AGC behind it,
    and there the reference itself spreads by 7.2e-5 / 3.0e-5 of full scale in the two bursts behind the jump under an
    fp32 filter's floor (AM and SAM, measured like startup_bounds.py's lists) -- above the steady bound, which holds for a
    stream."""
    import cutesdr_amd as ca
    rig = Rig(ca, oracle, NAMES, taps=7, oracle_taps=True, nfft=NFFT)
    b = rig.b
    g0 = b.group_count()
    assert g0 == (3, 12)
    expect = g0
    fills32 = _fills(WINDOWS, LIM // 32)
    total, pos = sum(WINDOWS) * LIM, 0
    rows = {}                                               # (kind, rate) -> the row's whole stream (not kept in _signal's cache)
    for k, w in enumerate(WINDOWS):
        changed = set()
        if k == 2:
            rig.set_demod(2, "AM"); changed.add(2)
            expect = (expect[0] + 1, expect[1] + 1)
        if k == 3:
            rig.set_demod(10, "USB"); changed.add(10)
            expect = (expect[0] + 1, expect[1] + 1)
        if k == 4:
            (st,) = _many(rig, [(4, "USB", NEW_EDGES["USB"])])
            assert (st == 0).all(), st
            rig.set_demod(4, "AM"); changed.add(4)
            expect = (expect[0] + 1, expect[1] + 1)
        if k == 5:
            rig.set_demod(9, "USB"); changed.add(9)
        if k == 6:
            (st,) = _many(rig, [(8, "FM", NEW_EDGES["FM"]), (9, "USB", NEW_EDGES["USB"])])
            assert (st == 0).all(), st
            rig.set_input_rate(FS_ALT); changed.update(range(rig.C))
        if k == 7:
            rig.set_input_rate(FS); changed.update(range(rig.C))
        if k == 8:
            rig.set_demod(8, "AM"); changed.add(8)
            expect = (expect[0] + 1 - 1, expect[1] + 1 - 2)
        assert b.group_count() == expect, (k, b.group_count(), expect)
        n = w * LIM
        for kind in set(rig.kinds):
            if (kind, rig.fs) not in rows:
                rows[(kind, rig.fs)] = _signal.__wrapped__(kind, 0, total, rig.fs)
        x = np.stack([rows[(rig.kinds[c], rig.fs)][pos:pos + n] for c in range(rig.C)])
        pos += n
        for r in rig.refs:
            r.clear_taps()
        got = b.process(x)
        want = rig.oracle_outs(x)
        if k < 6:                                           # (the SSB group has run at / 32 of 2 MSPS throughout)
            assert len(want[0]) == fills32[k][0] * HOP, (k, len(want[0]))
        rig.check(got, want, ("call", k))
        for c in range(rig.C):
            _check_taps(rig, c, k, strict_tap3=k >= 1 and c not in changed)
    assert _form(b) == 0


def test_chained_form_at_16384_points_survives_a_move_and_the_move_back():
    """the chained pipeline and a strict twin, four receivers behind the 16384-point filter: USB -> AM opens a group, AM ->
    USB takes the receiver, alone in its group, back in place -- every output word equals the twin's"""
    import cutesdr_amd as ca
    names = ["USB", "LSB", "FM", "AM"]
    pipe, strict = ca.DemodBatch(len(names), NFFT), ca.DemodBatch(len(names), NFFT)
    for b in (pipe, strict):
        b.set_input_rate(FS)
        for c, name in enumerate(names):
            m, kw = _info_kw(name)
            b.set_demod(c, m, info(ca, **kw))
        b.commit()
        for c in range(len(names)):
            b.set_freq(c, -100e3 - 500.0 * c)
    pipe.set_pipelined(1)
    assert _form(pipe) == 3 and _form(strict) == 0
    g0 = pipe.group_count()
    plan = {2: (0, "AM"), 4: (0, "USB")}
    for k, w in enumerate(WINDOWS[:6]):
        if k in plan:
            c, name = plan[k]
            m, kw = _info_kw(name)
            for b in (pipe, strict):
                b.set_demod(c, m, info(ca, **kw))
            assert _form(pipe) == 3
            assert pipe.group_count() == strict.group_count() == (g0[0] + 1, g0[1] + 1), (k, pipe.group_count())
        x = np.stack([_signal(KIND_OF[m], 0, w * LIM, FS) for m in names])
        gp, gs = pipe.process(x), strict.process(x)
        for c in range(len(names)):
            assert len(gp[c]) == len(gs[c]) and np.array_equal(gp[c].view(np.uint32), gs[c].view(np.uint32)), (k, c)
    assert sum(len(a) for a in gs) > 0
    assert np.array_equal(pipe.smeter_all(), strict.smeter_all())
