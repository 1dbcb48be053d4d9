"""A committed batch whose control-plane features meet: SetDemod that moves a receiver or changes it in place, stage taps,
the pipelined (chained) form, set_input_rate, set_input_rows and the datagram form with the blanker.
The other files check each feature alone.  Here they run together, and every receiver follows its own fp64 oracle
CDemodulator, which gets the same calls at the same stream positions.

Bounds, all existing ones:
  * from a demodulator's start (the stream's, or a mode change's): the chain rule of test_postchain_gpu.py, restarted
    as test_chain_parity_gpu.py::test_live_mode_change_inside_a_batch restarts it;
  * behind a same-mode SetDemod, a retune, a new input row or an input-rate switch: the rule of
    test_control_plane_gpu.py (1e-3 FM / 5e-4 for eight bursts, then the steady bound);
  * stage taps: the bounds of test_chain_taps_gpu.py::test_batch_taps_equal_the_single_receivers;
  * the pipelined form against the strict mode: the same words."""
import concurrent.futures as cf
import ctypes as C
import functools
import numpy as np
import pytest
from util_signals import FULL_SCALE, fm_carrier, am_carrier, tones_plus_noise
from test_postchain_gpu import (MODES, info, burst_errors, STEADY, FROM_ZERO, FM_STARTUP, FM_STEADY, SAM_FIRST,
                                SAM_SECOND)
from test_chain_taps_gpu import K2_TOL, K1_REL, _oracle_post_chain
import startup_bounds as SB

pytestmark = pytest.mark.gpu

FS, FS_ALT, LIM = 2e6, 3.2e6, 19968     # FS_ALT: FM (15 kHz) decimates by 64 there, SSB (20 kHz) by 32 -- rows must move
ESTATE = -4
KIND_OF = {"FM": "FM", "AM": "AM", "SAM": "AM", "USB": "T", "LSB": "T", "CWU": "T"}
# the modes a receiver may take on its input: FM only on an FM carrier, SAM only on an AM carrier
COMPAT = {"FM": ["FM", "USB", "AM"], "AM": ["AM", "SAM", "USB", "LSB"], "T": ["USB", "LSB", "AM", "CWU"]}


@functools.lru_cache(maxsize=None)
def _signal(kind, variant, n, fs):
    """one input row of a kind: the station at 100 kHz; variant 1 adds a carrier at -300 kHz that every receiver's
    filters reject (a receiver switched between the two rows keeps its station)"""
    if kind == "FM":
        x = fm_carrier(n, fs, 100e3, dbfs=-20.0)
    elif kind == "AM":
        x = am_carrier(n, fs, 100e3, dbfs=-20.0)
    else:
        # (tones in the USB, LSB and CW pass bands: no receiver on this row demodulates noise alone under a wide-open AGC)
        x = tones_plus_noise(9, n, fs, [100e3 + 1200.0, 100e3 + 2340.0, 100e3 - 1200.0, 100e3 - 2040.0, 100e3, 100e3 + 300.0])
    if variant:
        x = x + am_carrier(n, fs, -300e3, fmod=700.0, dbfs=-26.0, noise_dbfs=-200.0, channel=7)
    x = x.astype(np.complex64)
    x.flags.writeable = False
    return x


def _form(b):
    """csdr__demod_batch_form: 3 for a pipelined batch (bit 0 pipelined, bit 1 chained), 0 for a strict one"""
    from cutesdr_amd._capi import lib
    L = lib()
    L.csdr__demod_batch_form.restype = C.c_int
    L.csdr__demod_batch_form.argtypes = [C.c_void_p]
    return L.csdr__demod_batch_form(b.h)


def _set_pipelined_rc(b, on):
    from cutesdr_amd._capi import lib
    return lib().csdr_demod_batch_set_pipelined(b.h, int(on))


def _oracle_out(r, x, stereo):
    """the oracle's audio of one call of whole m_InBufLimit windows (stereo: the stereo overload, window by window)"""
    x = np.asarray(x, dtype=np.complex128)
    if not stereo:
        return r.process_append(x)
    lim = r.buf_limit()
    assert len(x) % lim == 0
    w = []
    for i in range(0, len(x), lim):
        k, o = r.ProcessData(x[i:i + lim], True)
        w.append(o[:k].copy())
    return np.concatenate(w) if w else np.zeros(0, dtype=np.complex128)


def _span(bursts, hop):
    """an allowance of `bursts` 1024-sample bursts keeps its length in samples: the whole bursts of `hop` samples it touches"""
    return -(-bursts * 1024 // hop)


def _start_bound(mode, k, errs, first, stereo, late, hop=1024):
    """the chain rule (test_postchain_gpu.check_chain_bursts; a restart as in test_live_mode_change_inside_a_batch) as
    per-burst bounds; k: bursts since the demodulator started, errs: the errors from there.  hop = 8192 (the 16384-point
    filter): a burst's bound is the largest the rule gives any of the eight 1024-sample bursts in it -- every allowance
    keeps its length in samples, rounded up to whole bursts -- except the stream's first burst, which holds the whole
    start-up: startup_bounds.first_burst_16k on this rig's rows (FM: the pull-in, arbitrary), the steady bound behind it"""
    if hop != 1024:
        assert hop == 8192, hop
        r = hop // 1024
        fine = (np.asarray(k)[:, None] * r + np.arange(r)[None, :]).ravel()
        out = _start_bound(mode, fine, np.zeros(0), first, stereo, late).reshape(-1, r).max(axis=1)
        if first:
            b0 = SB.first_burst_16k(mode, stereo, rig=True)
            out = np.where(k == 0, 2.5 * FULL_SCALE if b0 is None else b0 * FULL_SCALE, out)
        return out
    if mode == "FM":
        s = 0
        big = np.nonzero(errs[:3] > 0.2 * FULL_SCALE)[0]
        if len(big):
            s = int(big[0])
        out = np.full(len(k), 2.5 * FULL_SCALE)
        for j in range(1, len(FM_STARTUP)):
            out = np.where(k >= s + j + late, FM_STARTUP[j], out)
        return np.where(k >= s + len(FM_STARTUP) + late, FM_STEADY, out)
    if mode == "SAM" and stereo:
        return np.where(k <= 1, SB.SAM_STEREO_BISTABLE * FULL_SCALE, STEADY)
    if mode == "SAM":
        z = 1e-3 * FULL_SCALE
        first_b, second_b = (max(z, SAM_FIRST), max(z, SAM_SECOND)) if first else (z, z)
        return np.where(k == 0, first_b, np.where(k == 1, second_b, STEADY))
    return np.where(k < 2, FROM_ZERO, STEADY)


class Track:
    """one receiver's per-burst audio errors since its stream began, and the events that set their bounds: every event's
    rule holds from its burst until the demodulator's next start; the bound of a burst is the largest that holds there"""

    def __init__(self, mode, stereo=False, fm_late=0, hop=1024):
        self.mode, self.stereo, self.fm_late, self.hop = mode, stereo, fm_late, hop
        self.errs = []
        self.events = [(0, "start", mode, True)]

    def restart(self, mode):
        self.mode = mode
        self.events.append((len(self.errs), "start", mode, False))

    def control(self):
        self.events.append((len(self.errs), "ctl", self.mode, False))

    def bounds(self):
        e = np.asarray(self.errs, dtype=float)
        n = len(e)
        i = np.arange(n)
        bound = np.zeros(n)
        starts = [p for p, kind, _, _ in self.events if kind == "start"] + [n]
        for pos, kind, mode, first in self.events:
            end = min([s for s in starts if s > pos] + [n])
            on = (i >= pos) & (i < end)
            k = i - pos
            if kind == "ctl":
                b = np.where(k < _span(8, self.hop), (1e-3 if mode == "FM" else 5e-4) * FULL_SCALE, FM_STEADY if mode == "FM" else STEADY)
            else:
                b = _start_bound(mode, k, e[pos:] if pos < n else e[:0], first, self.stereo, self.fm_late if first else 0, self.hop)
            bound = np.where(on, np.maximum(bound, b), bound)
        return bound

    def add(self, got, want, what):
        assert len(got) == len(want), (what, self.mode, len(got), len(want))
        if not len(want):
            return
        if self.mode == "FM" and not self.stereo:                   # identical squelch decisions, burst by burst
            for j in range(0, len(want), self.hop):
                assert (not np.any(got[j:j + self.hop])) == (not np.any(want[j:j + self.hop])), (what, j // self.hop)
        self.errs.extend(burst_errors(np.asarray(got, dtype=want.dtype), want, self.hop))
        e, bd = np.asarray(self.errs), self.bounds()
        assert np.isfinite(e).all(), (what, self.mode)
        bad = np.nonzero(e > bd)[0]
        assert not len(bad), (what, self.mode, "bursts", bad[:6], (e[bad[:6]] / FULL_SCALE), "bounds", bd[bad[:6]] / FULL_SCALE,
                              self.events)


def _info_kw(name, **over):
    m, kw = MODES[name]
    return m, dict(kw, **over)


class Rig:
    """a batch and one oracle CDemodulator per receiver, driven by the same calls"""

    def __init__(self, ca, oracle, names, kinds=None, rows=None, form=0, taps=0, oracle_taps=False, stereo=False,
                 freqs=None, fm_late=0, nfft=2048):
        self.ca, self.oracle, self.stereo = ca, oracle, stereo
        self.nfft = nfft                                   # the band-pass filter's size; a burst of audio is one hop of it
        self.C = len(names)
        self.modes = list(names)
        self.kinds = list(kinds or [KIND_OF[m] for m in names])
        self.freqs = list(freqs or [-100e3] * self.C)
        self.fs = FS
        self.batches = [ca.DemodBatch(self.C, nfft)]
        self.refs = []
        for b in self.batches:
            b.set_input_rate(FS)
            if rows is not None:
                b.set_input_rows(np.asarray(rows, dtype=np.int32))
        for c, name in enumerate(names):
            m, kw = _info_kw(name)
            for b in self.batches:
                b.set_demod(c, m, info(ca, **kw))
            r = oracle.CDemodulator(nfft)
            r.SetInputSampleRate(FS); r.SetDemod(m, info(oracle, **kw)); r.SetDemodFreq(self.freqs[c])
            if oracle_taps:
                r.enable_taps(True)
            self.refs.append(r)
        for b in self.batches:
            b.commit()
            for c in range(self.C):
                b.set_freq(c, self.freqs[c])
        self.b = self.batches[0]
        if taps:
            self.b.set_taps(taps)
        if form:
            self.b.set_pipelined(form)
        self.tracks = [Track(m, stereo, fm_late, nfft // 2) for m in names]
        self.set_demods = [0] * self.C                     # SetDemod calls a receiver has had since commit

    def set_demod(self, c, name, **over):
        m, kw = _info_kw(name, **over)
        for b in self.batches:
            b.set_demod(c, m, info(self.ca, **kw))
        self.refs[c].SetDemod(m, info(self.oracle, **kw))
        if name != self.modes[c]:
            self.tracks[c].restart(name)
        else:
            self.tracks[c].control()
        self.modes[c] = name
        self.set_demods[c] += 1
        assert self.b.output_rate(c) == self.refs[c].GetOutputRate(), (c, name)

    def set_freq(self, c, f):
        self.freqs[c] = f
        for b in self.batches:
            b.set_freq(c, f)
        self.refs[c].SetDemodFreq(f)
        self.tracks[c].control()

    def set_input_rate(self, fs):
        self.fs = fs
        for b in self.batches:
            b.set_input_rate(fs)
        for c, r in enumerate(self.refs):
            r.SetInputSampleRate(fs)
            self.tracks[c].control()
        assert [self.b.output_rate(c) for c in range(self.C)] == [r.GetOutputRate() for r in self.refs]

    def oracle_outs(self, xs):
        """every receiver's oracle audio of one call; xs[c]: receiver c's input"""
        with cf.ThreadPoolExecutor(16) as ex:
            return list(ex.map(lambda c: _oracle_out(self.refs[c], xs[c], self.stereo), range(self.C)))

    def check(self, got, want, what):
        for c in range(self.C):
            self.tracks[c].add(got[c], want[c], (what, c))


NAMES8 = ["FM", "AM", "USB", "SAM", "FM", "AM", "USB", "LSB"]
N64 = 64 * LIM          # whole m_InBufLimit windows, and whole FastFIR hops at /32: a USB group's staging fill stays empty


def _check_taps(rig, c, k, strict_tap3):
    r = rig.refs[c]
    g1, g2, g3 = rig.b.tap(c, 1, cap=1 << 22), rig.b.tap(c, 2, cap=1 << 22), rig.b.tap(c, 3, cap=1 << 22)
    w1, w2, w3 = r.tap(1), r.tap(2), r.tap(3)
    what = (k, c, rig.modes[c])
    assert len(g1) == len(w1) and len(g2) == len(w2) and len(g3) == len(w3), (what, len(g1), len(w1), len(g2), len(w2))
    if len(w1):
        assert np.abs(g1 - w1).max() <= K2_TOL, (what, "tap 1", np.abs(g1 - w1).max() / FULL_SCALE)
    if len(w2):
        assert np.abs(g2 - w2).max() <= K1_REL * np.abs(w1).max() * 1.5, (what, "tap 2")
        if strict_tap3:
            assert np.abs(g3 - w3).max() <= STEADY, (what, "tap 3", np.abs(g3 - w3).max() / FULL_SCALE)


@pytest.mark.parametrize("how", ["mode", "rate"])
def test_taps_follow_receivers_that_move(oracle, how):
    """csdr_demod_batch_set_taps(7) on a strict batch of eight mixed receivers, then receivers that move: "mode" -- USB ->
    AM opens a new plan group, AM -> USB goes into the muted row the first one left, and FM -> AM for both receivers of the
    FM group drops that group (one takes the muted row the AM receiver left, the other opens a group); "rate" -- FM -> USB
    in place (the same decimation at 2 MSPS), then 2 -> 3.2 -> 2 MSPS, where the two no longer decimate alike and one of
    them moves.  Every receiver's taps 1-3 of every call against its oracle's, and its audio."""
    import cutesdr_amd as ca
    rig = Rig(ca, oracle, NAMES8, taps=7, oracle_taps=True)
    b = rig.b
    g0 = b.group_count()
    calls = 8
    for k in range(calls):
        changed = set()
        if how == "mode":
            if k == 2:
                rig.set_demod(2, "AM"); changed.add(2)
                assert b.group_count() == (g0[0] + 1, g0[1] + 1)     # a group of its own
            if k == 4:
                rig.set_demod(5, "USB"); changed.add(5)
                assert b.group_count() == (g0[0] + 1, g0[1] + 1)     # into the muted row receiver 2 left
            if k == 6:
                rig.set_demod(0, "AM"); rig.set_demod(4, "AM"); changed.update((0, 4))
                assert b.group_count() == (g0[0] + 1, g0[1])         # a muted row, a new group, the FM group dropped
        else:
            if k == 2:
                rig.set_demod(0, "USB"); changed.add(0)
                assert b.group_count() == g0                        # in place
            if k == 3:
                rig.set_input_rate(FS_ALT); changed.update(range(rig.C))
                assert b.group_count()[0] > g0[0]                   # somebody moved
            if k == 5:
                rig.set_input_rate(FS); changed.update(range(rig.C))
        x = np.stack([_signal(rig.kinds[c], 0, N64, rig.fs) for c in range(rig.C)])
        for r in rig.refs:
            r.clear_taps()
        got = b.process(x)
        want = rig.oracle_outs(x)
        rig.check(got, want, ("call", k))
        for c in range(rig.C):
            _check_taps(rig, c, k, strict_tap3=k >= 1 and c not in changed)


def test_set_pipelined_is_refused_while_taps_are_on(oracle):
    """the other order of the check set_taps makes: set_pipelined(1 | 2 | 3) on a batch with stage taps returns ESTATE and
    changes nothing -- the batch keeps running strict, its taps readable; after set_taps(0) it goes through"""
    import cutesdr_amd as ca
    names = ["FM", "AM", "USB", "SAM"]
    rig = Rig(ca, oracle, names, taps=7, oracle_taps=True)
    b = rig.b
    n = 8 * LIM
    for on in (1, 2, 3):
        assert _set_pipelined_rc(b, on) == ESTATE, on
        assert _form(b) == 0, on
    for k in range(2):
        x = np.stack([_signal(rig.kinds[c], 0, n, FS) for c in range(rig.C)])
        for r in rig.refs:
            r.clear_taps()
        got = b.process(x)
        rig.check(got, rig.oracle_outs(x), ("strict", k))
        for c in range(rig.C):
            _check_taps(rig, c, k, strict_tap3=False)
    b.set_taps(0)
    assert _set_pipelined_rc(b, 1) == 0
    assert _form(b) == 3
    x = np.stack([_signal(rig.kinds[c], 0, n, FS) for c in range(rig.C)])
    rig.check(b.process(x), rig.oracle_outs(x), ("chained", 2))


@pytest.mark.parametrize("form", [1], ids=["chained"])
def test_pipelined_form_survives_moves(form):
    """A pipelined batch and a strict twin fed the same calls and changes: a move that opens a group (USB -> AM), one into
    the muted row it left (AM -> USB, which drops the group), an in-place change (FM -> USB), an input-rate switch that
    moves a receiver, and back.  The pipelined batch stays pipelined, the strict twin strict, and every output word equals
    the twin's."""
    import cutesdr_amd as ca
    C_ = len(NAMES8)
    groups_before_rate = None
    pipe, strict = ca.DemodBatch(C_, 2048), ca.DemodBatch(C_, 2048)
    for b in (pipe, strict):
        b.set_input_rate(FS)
        for c, name in enumerate(NAMES8):
            m, kw = _info_kw(name)
            b.set_demod(c, m, info(ca, **kw))
        b.commit()
        for c in range(C_):
            b.set_freq(c, -100e3 - 500.0 * c)
    pipe.set_pipelined(form)
    want_form = {0: 0, 1: 3}[form]
    assert _form(pipe) == want_form and _form(strict) == 0
    # (as in test_taps_follow_receivers_that_move: a new group, a muted row, a dropped group; then an in-place change that
    # the switch to 3.2 MSPS turns into a move, and back)
    plan = {2: [("demod", 2, "AM")], 4: [("demod", 5, "USB")], 6: [("demod", 0, "AM"), ("demod", 4, "AM")],
            7: [("demod", 7, "FM")], 8: [("rate", FS_ALT)], 10: [("rate", FS)]}
    fs = FS
    for k in range(12):
        for op in plan.get(k, []):
            for b in (pipe, strict):
                if op[0] == "demod":
                    m, kw = _info_kw(op[2])
                    b.set_demod(op[1], m, info(ca, **kw))
                else:
                    b.set_input_rate(op[1])
            if op[0] == "rate":
                fs = op[1]
            assert _form(pipe) == want_form, (k, op, _form(pipe))
            assert pipe.group_count() == strict.group_count(), (k, op)
        if k == 8:
            assert pipe.group_count() != groups_before_rate             # the rate switch moved receiver 7
        groups_before_rate = pipe.group_count()
        x = np.stack([_signal(KIND_OF[m], 0, N64, fs) for m in NAMES8])      # (each row keeps its first station)
        gp, gs = pipe.process(x), strict.process(x)
        for c in range(C_):
            assert len(gp[c]) == len(gs[c]) and np.array_equal(gp[c].view(np.uint32), gs[c].view(np.uint32)), (k, c)
    assert _form(pipe) == want_form
    assert np.array_equal(pipe.smeter_all(), strict.smeter_all())


@pytest.mark.parametrize("case", ["AM-SAM", "USB-LSB", "FM-USB"])
@pytest.mark.parametrize("form", [0, 1], ids=["strict", "chained"])
def test_in_place_changes_while_a_call_is_in_flight(oracle, form, case):
    """64 receivers, calls of 64 windows (1.28 M samples) issued with process_ptr and never waited for.  Right after call 1
    returns -- its launches still on the device in the pipelined form -- three receivers get a same-mode SetDemod with
    another AGC knee and decay, then a mode change that keeps their row: AM -> SAM, USB -> LSB, or FM -> USB (a new
    decimator plan of the same stage count: its histories are reset).  Call 1 must be the oracle's with the OLD
    parameters, call 2 with the new ones, and every other receiver untouched.  The strict mode is the control."""
    import cutesdr_amd as ca
    src, dst = case.split("-")
    kinds4 = ["AM", "T", "FM", "AM"]
    names = [("AM", "USB", "FM", "SAM")[c % 4] for c in range(64)]
    C_ = len(names)
    rows = [c % 4 for c in range(C_)]
    freqs = [-100e3] * C_                                   # (on the carrier: the SAM loop pulls in from the stream's start)
    calls, n = 3, N64
    rig = Rig(ca, oracle, names, kinds=[kinds4[c % 4] for c in range(C_)], rows=rows, form=form, freqs=freqs)
    b = rig.b
    xin = np.stack([_signal(kinds4[r], 0, calls * n, FS) for r in range(4)])
    din = ca.DeviceBuffer(xin.nbytes)
    din.upload(xin)
    cap = n // 32 + 2048 + 4096
    douts = [ca.DeviceBuffer(C_ * cap * 4) for _ in range(calls)]
    changed = [c for c in range(C_) if names[c] == src][:3]
    # (another knee, decay and slope move AM and SSB audio by 5e3 x the steady bound; FM audio does not depend on the
    # AGC, so its same-mode change also narrows the edges, which moves the squelch high-pass -- a post-chain patch too)
    new_agc = dict(AgcThresh=-40, AgcDecay=1000, AgcSlope=10)
    same_kw = dict(new_agc, **(dict(HiCut=3000, LowCut=-3000) if src == "FM" else {}))
    counts = []
    g0 = b.group_count()
    for k in range(calls):
        b.process_ptr(din.ptr + 8 * k * n, calls * n, n, douts[k].ptr, cap)
        counts.append([b.out_count(c) for c in range(C_)])
        if k == 1:                                           # call 1 is in flight: same-mode changes first, then the modes
            for c in changed:
                m, kw = _info_kw(src, **same_kw)
                b.set_demod(c, m, info(ca, **kw))
            for c in changed:
                m, kw = _info_kw(dst, **new_agc)
                b.set_demod(c, m, info(ca, **kw))
            assert b.group_count() == g0                     # nobody moved
    b.flush()
    ca.sync()
    assert _form(b) == {0: 0, 1: 3}[form]
    # the oracle side, call by call, the changes between calls 1 and 2
    ghost = {}
    for k in range(calls):
        if k == 2:
            for c in changed:
                m, kw = _info_kw(src, **same_kw)
                rig.refs[c].SetDemod(m, info(oracle, **kw)); rig.tracks[c].control()
            for c in changed:
                m, kw = _info_kw(dst, **new_agc)
                rig.refs[c].SetDemod(m, info(oracle, **kw)); rig.tracks[c].restart(dst)
                rig.modes[c] = dst
        xs = [xin[rows[c], k * n:(k + 1) * n] for c in range(C_)]
        if k == 1:                                           # what a change landing inside call 1 would give: it has to show
            for c in changed:
                g = oracle.CDemodulator(2048)
                g.SetInputSampleRate(FS)
                m, kw = _info_kw(src)
                g.SetDemod(m, info(oracle, **kw)); g.SetDemodFreq(freqs[c])
                g.process_append(xin[rows[c], :n].astype(np.complex128))
                m, kw = _info_kw(src, **same_kw)
                g.SetDemod(m, info(oracle, **kw))
                ghost[c] = g.process_append(xs[c].astype(np.complex128))
        want = rig.oracle_outs(xs)
        out = douts[k].download(np.float32, C_ * cap).reshape(C_, cap)
        got = [out[c, :counts[k][c]] for c in range(C_)]
        for c in ghost if k == 1 else ():
            assert np.abs(ghost[c] - want[c]).max() > 100 * STEADY, (c, "the new AGC constants must change call 1's audio")
        rig.check(got, want, (case, "call", k))


def _sweep(ca, oracle, seed, form, stereo, packets=False):
    """16 receivers of three kinds of input on six rows (two per kind), 8 calls; between the calls random control
    operations on receivers 0-11: same-mode SetDemod (edges, AGC), mode changes (in place or moving), retunes, another
    input row of the same station; one input-rate switch 2 -> 3.2 -> 2 MSPS.  packets: through
    csdr_demod_batch_process_packets with the blanker on (every receiver its own datagrams)."""
    from test_frontend_gpu import _pack16
    rng = np.random.default_rng(1000 + seed)
    C_, calls, n = 16, 8, 8 * LIM
    kinds = [("FM", "AM", "T")[c % 3] for c in range(C_)]
    names = [str(rng.choice(COMPAT[kd])) for kd in kinds]
    variant = [0] * C_
    rows = [2 * ("FM", "AM", "T").index(kinds[c]) + variant[c] for c in range(C_)]
    freqs = [-100e3] * C_
    taps = 2 if (form == 0 and not packets) else 0
    rig = Rig(ca, oracle, names, kinds=kinds, rows=None if packets else rows, form=form, stereo=stereo, freqs=freqs,
              taps=taps, fm_late=1 if packets else 0)
    b = rig.b
    nb, rnb = None, None
    if packets:
        nb = ca.NoiseProcBatch(C_); nb.setup(True, 30.0, 10.0, FS)
        rnb = []
        for c in range(C_):
            q = oracle.CNoiseProc(); q.SetupBlanker(True, 30.0, 10.0, FS); rnb.append(q)
    # the loop-only check (test_chain_taps_gpu.py): the oracle's AGC and demodulator on the GPU's own filter output (tap 2),
    # for receivers whose post-chain no SetDemod has touched
    posts = [_oracle_post_chain(oracle, names[c], stereo, rig.refs[c].GetOutputRate()) for c in range(C_)] if taps else None
    loop_bursts = [0] * C_
    rate_at = int(rng.integers(2, 6))
    pos = 0                                                  # the stream position of every row, in samples
    for k in range(calls):
        if k == rate_at:
            rig.set_input_rate(FS_ALT)
        elif k == rate_at + 1:
            rig.set_input_rate(FS)
        if k >= 1:
            for c in rng.choice(12, size=3, replace=False):
                c = int(c)
                ops = ["freq", "rows"] if (k in (rate_at, rate_at + 1) or packets) else ["same", "mode", "freq", "rows"]
                if packets:
                    ops = ["freq"] if k in (rate_at, rate_at + 1) else ["same", "mode", "freq"]
                op = ops[int(rng.integers(len(ops)))]
                if op == "same":
                    m = rig.modes[c]
                    over = dict(AgcThresh=int(rng.choice([-100, -80, -60])), AgcDecay=int(rng.choice([200, 500, 1000])))
                    if m in ("AM", "SAM", "FM"):
                        h = int(rng.choice([3000, 4000, 5000])); over.update(HiCut=h, LowCut=-h)
                    elif m == "USB":
                        over.update(HiCut=int(rng.choice([2400, 2800])), LowCut=int(rng.choice([100, 300])))
                    elif m == "LSB":
                        over.update(HiCut=-int(rng.choice([100, 300])), LowCut=-int(rng.choice([2400, 2800])))
                    rig.set_demod(c, m, **over)
                elif op == "mode":
                    choices = [m for m in COMPAT[kinds[c]] if m != rig.modes[c]]
                    rig.set_demod(c, choices[int(rng.integers(len(choices)))])
                elif op == "freq":
                    # (receivers on an AM carrier stay on it: SAM can start there, and its loop pulls in on the carrier)
                    rig.set_freq(c, -100e3 - (0.0 if kinds[c] == "AM" else float(rng.choice([0.0, 150.0, -200.0]))))
                else:
                    variant[c] ^= 1
                    rows[c] = 2 * ("FM", "AM", "T").index(kinds[c]) + variant[c]
                    b.set_input_rows(np.asarray(rows, dtype=np.int32))
                    rig.tracks[c].control()
        kinds3 = ("FM", "AM", "T")
        src = [_signal(kinds3[r // 2], r % 2, calls * n, rig.fs) for r in range(6)]
        xs = [src[rows[c]][pos:pos + n] for c in range(C_)]
        what = (seed, form, "stereo" if stereo else "mono", "call", k)
        if packets:
            raw = np.stack([_pack16(x.astype(np.complex128)) for x in xs])
            got = b.process_packets(raw, 1028, nb)
            xs = [rnb[c].ProcessBlanker(oracle.unpack_packets(raw[c], 1028)) for c in range(C_)]
        else:
            x6 = np.stack([s[pos:pos + n] for s in src])
            x6 = np.concatenate([x6, np.zeros((C_ - 6, n), dtype=np.complex64)])
            got = b.process(x6, stereo=stereo)
        want = rig.oracle_outs(xs)
        rig.check(got, want, what)
        if taps:
            for c in range(C_):
                if rig.set_demods[c] or not len(got[c]):
                    continue
                g2 = b.tap(c, 2, cap=1 << 22)
                assert len(g2) == len(got[c]), (what, c)
                _, w4 = posts[c](g2)
                e = burst_errors(np.asarray(got[c], dtype=w4.dtype), w4)
                idx = loop_bursts[c] + np.arange(len(e))
                if rig.modes[c] == "FM":
                    bound = np.where(idx < 3, 1e-4 * FULL_SCALE, 3e-5 * FULL_SCALE)
                else:
                    bound = np.full(len(e), STEADY)
                assert (e <= bound).all(), (what, c, rig.modes[c], "loop-only", e[:6] / FULL_SCALE)
                loop_bursts[c] += len(e)
        pos += n
    if not packets:
        sm = b.smeter_all()
        for c in range(C_):
            assert float(sm[c]) == pytest.approx(rig.refs[c].GetSMeterAve(), abs=0.02), c


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("form", [0, 1], ids=["strict", "chained"])
@pytest.mark.parametrize("seed", range(6))
def test_seeded_control_sequences(oracle, seed, form, stereo):
    import cutesdr_amd as ca
    _sweep(ca, oracle, seed, form, stereo)


@pytest.mark.parametrize("form", [0, 1], ids=["strict", "chained"])
def test_seeded_control_sequence_on_datagrams_with_the_blanker(oracle, form):
    import cutesdr_amd as ca
    _sweep(ca, oracle, 6, form, False, packets=True)
