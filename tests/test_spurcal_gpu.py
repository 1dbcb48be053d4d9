"""GPU checks of the batch NCO-spur calibration (csdr_spurcal_batch_*, K13): CSdrInterface::ProcessIQData calibrates on
the samples its in-place blanker handed over (reference interface/sdrinterface.cpp:884, :886-887) while the bookkeeping
of :791-848 says so.  The checker is made of the fp64 checker's pieces, per receiver and per datagram: unpack_packets ->
CNoiseProc.ProcessBlanker (state kept across datagrams) -> spurcal, under the literal bookkeeping of tests/spurcal_ref.py.

Common shape: four receivers on one feed (tones + noise + DC + impulses of 30000) -- blanker on with an odd delay_n + 1
(51), on with an even one (152), off, and on for a receiver whose calibration is never started -- about 2600 datagrams per
receiver, so that a calibration ends inside the feed; puts vary in length and are multiples of 512 samples (the chain's
rule: 2 datagrams of 1028 bytes, 32 of 1444); starts are staggered."""
import ctypes as C
import functools
import numpy as np
import pytest
from spurcal_ref import RefSpurCal
from test_display_stream_gpu import make_packets, OracleDisplay, rate_for_skip, feed_signal
from test_display_blanked_gpu import THRESH, IMPULSE, PATTERN, CHAIN_FS, ESTATE, EINVAL, audio_cap
from test_fft_resampler_gpu import assert_spectrum_close

pytestmark = pytest.mark.gpu

CN = 4
WIDTH_N = (100, 302, 100, 100)       # m_WidthSamples: delay_n + 1 = 51 (odd) / 152 (even) / (off) / 51
ON = (True, True, False, True)
FS = rate_for_skip(2048, 1)
FEED_DC = (150.0, -6.0)              # x (1 + 0.2 c): every I beyond the STARTCAL clamp of 10, every |Q| inside it
SET3 = (7.5, -2.25)                  # receiver 3: SET, never started
NPK = 2600
PER = {1444: 240, 1028: 256}


def width_us(c):
    return (WIDTH_N[c] + 0.5) / FS * 1e6                     # (int)(width * 1e-6 * fs) = WIDTH_N[c], noiseproc.cpp:89


def put_sizes(pkt_len):
    """datagrams per put: varying, each put a multiple of 512 samples"""
    out, k = [], 0
    while sum(out) < NPK:
        out.append(PATTERN[k % len(PATTERN)] * 32 if pkt_len == 1444 else (PATTERN[k % len(PATTERN)] * 16 + k % 2) * 2)
        k += 1
    return out


def commands(k):
    """what is commanded before put k: (receiver, command, arguments)"""
    return {0: [(0, "start_cal", ()), (3, "set", SET3)],
            1: [(2, "set", (50.0, -3.0)), (2, "start_cal", ())],              # -> I = 0, Q = -3, active
            3: [(1, "start_cal", ())]}.get(k, [])


def command_device(s, c, name, args):
    if name == "set":
        s.set(args[0], args[1], c)
    else:
        s.start_cal(c)


@functools.lru_cache(maxsize=None)
def feed(pkt_len):
    """-> (datagrams uint8 [CN, npk, pkt_len], puts, max |sample|)"""
    per = PER[pkt_len]
    puts = put_sizes(pkt_len)
    calls = [p * per for p in puts]
    assert all(n % 512 == 0 for n in calls)
    tot = sum(calls)
    x = feed_signal(CN, tot, FS, seed=pkt_len, dc=FEED_DC)
    edge = np.cumsum(calls)
    pos = {f * 4096 + 200 + (37 * f * f) % 3000 for f in range(tot // 4096)}
    pos |= {int(e) + 5 for e in edge[:-1]} | {int(e) - 20 for e in edge}
    pos = np.array(sorted(p for p in pos if p < tot))
    # the cases the blanked forms must meet, in this very feed
    assert any(min(WIDTH_N) // 2 > p - e >= 0 for e in edge[:-1] for p in pos)     # inside the first delay_n of a call
    assert any(0 < e - p < min(WIDTH_N) for e in edge for p in pos)                # a blank window across two calls
    assert any(0 < p % per < per - 1 for p in pos)                                 # a datagram blanked in part
    x[:, pos] += IMPULSE
    raw = make_packets(x, pkt_len)
    return raw, puts, float(max(np.abs(x.real).max(), np.abs(x.imag).max()))


def make_blankers(ca, count):
    out = []
    for _ in range(count):
        nb = ca.NoiseProcBatch(CN)
        for c in range(CN):
            nb.setup(ON[c], THRESH, width_us(c), FS, channel=c)
        out.append(nb)
    return out


def make_chain(ca, pipelined=False, channels=CN):
    import test_postchain_gpu as T
    b = ca.DemodBatch(channels, 2048); b.set_input_rate(CHAIN_FS)
    for c in range(channels):
        m, kw = T.MODES[("FM", "AM", "USB", "LSB", "CWU")[c]]
        b.set_demod(c, m, T.info(ca, **kw))
    b.commit()
    for c in range(channels):
        b.set_freq(c, -(100e3 + 900.0 * c))
    if pipelined:
        b.set_pipelined(True)
    return b


def chain_call(L, b, nb, dp, npk, pkt_len, dout, cap):
    return L.csdr_demod_batch_process_packets(b.h, C.c_void_p(dp.ptr), npk, pkt_len, nb.h, C.c_void_p(dout.ptr), cap, None)


@functools.lru_cache(maxsize=None)
def check_states(oracle, pkt_len, blank):
    """the checker: per put, per receiver (offset_i, offset_q, count, active)"""
    raw, puts, _ = feed(pkt_len)
    per = PER[pkt_len]
    refs = [RefSpurCal(lambda off, s: oracle.spurcal(np.array(off), s)) for _ in range(CN)]
    nbs = []
    for c in range(CN):
        q = oracle.CNoiseProc(); q.SetupBlanker(ON[c] and blank, THRESH, width_us(c), FS); nbs.append(q)
    out, p0 = [], 0
    for k, npk in enumerate(puts):
        for c, name, args in commands(k):
            getattr(refs[c], name)(*args)
        for c in range(CN):
            x = oracle.unpack_packets(raw[c, p0:p0 + npk], pkt_len)
            for p in range(npk):                                                   # one ProcessIQData call per datagram
                refs[c].call(per, nbs[c].ProcessBlanker(x[p * per:(p + 1) * per]))  # :884, :886-887
        p0 += npk
        out.append([r.state() for r in refs])
    return out


@functools.lru_cache(maxsize=None)
def run_forms(pkt_len, pipelined):
    """The same puts through
      blanked   the fused chain call + put_packets_blanked
      plain     put_packets
      unpacked  csdr_ingest_unpack (no DC) + put_stream(call_len = per)
      two_pass  a second blanker with the same set-up into fp32 rows + put_stream(call_len = per)
    -> {name: per put [per receiver get_state]}.  pipelined: the chain in pipelined mode, two input buffers alternating, no
    device synchronisation between the calls -- blanked only."""
    import cutesdr_amd as ca
    L = ca.lib()
    raw, puts, _ = feed(pkt_len)
    per = PER[pkt_len]
    b, (nb, nb2) = make_chain(ca, pipelined), make_blankers(ca, 2)
    names = ("blanked",) if pipelined else ("blanked", "plain", "unpacked", "two_pass")
    objs = {k: ca.SpurCalBatch(CN) for k in names}
    cap = audio_cap([p * per for p in puts])
    dout = ca.DeviceBuffer(4 * CN * cap)
    pmax = max(puts)
    bufs = [ca.DeviceBuffer(CN * pmax * pkt_len) for _ in range(2)]
    rows, blanked = ca.DeviceBuffer(CN * pmax * per * 8), ca.DeviceBuffer(CN * pmax * per * 8)
    states = {k: [] for k in names}
    p0 = 0
    for k, npk in enumerate(puts):
        n = npk * per
        for c, name, args in commands(k):
            for s in objs.values():
                command_device(s, c, name, args)
        din = bufs[k % 2]
        din.upload(np.ascontiguousarray(raw[:, p0:p0 + npk])); p0 += npk
        assert chain_call(L, b, nb, din, npk, pkt_len, dout, cap) == 0
        objs["blanked"].put_packets_blanked_ptr(b, din.ptr, npk, pkt_len)
        if not pipelined:
            objs["plain"].put_packets_ptr(din.ptr, npk, pkt_len)
            assert L.csdr_ingest_unpack(0, C.c_void_p(din.ptr), CN, npk, pkt_len, C.c_void_p(rows.ptr), n, None, None) == n
            objs["unpacked"].put_stream_ptr(rows.ptr, n, n, per)
            nb2.process_ptr(rows.ptr, n, n, blanked.ptr, n)
            objs["two_pass"].put_stream_ptr(blanked.ptr, n, n, per)
        for name in names:                                     # (waits for the object's own last launch only)
            states[name].append([objs[name].get_state(c) for c in range(CN)])
    b.flush()
    ca.sync()
    for o in bufs + [rows, blanked, dout]:
        o.free()
    return states


def bits(v):
    return np.array([v], dtype=np.float64).view(np.uint64)[0]


def same_words(a, b):
    """two per-put state lists, no tolerance"""
    assert len(a) == len(b)
    for k, (sa, sb) in enumerate(zip(a, b)):
        for c in range(CN):
            assert sa[c][2:] == sb[c][2:], (k, c)
            assert bits(sa[c][0]) == bits(sb[c][0]) and bits(sa[c][1]) == bits(sb[c][1]), (k, c, sa[c], sb[c])


# ---- 1. against the checker --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pkt_len", [1444, 1028])
@pytest.mark.parametrize("form", ["plain", "blanked"])
def test_states_match_the_checker_after_every_put(oracle, pkt_len, form):
    """count and active equal, offsets within 1e-9 x max |sample of the feed| (the bound tests/test_frontend_gpu.py and
    tests/test_display_stream_gpu.py hold this recurrence to) after EVERY put; the never-started receiver's offsets are
    the words SET left; and the blanker matters: the blanked and the plain checker differ by far more than the bound."""
    _, puts, top = feed(pkt_len)
    got = run_forms(pkt_len, False)[form]
    want = check_states(oracle, pkt_len, form == "blanked")
    tol = 1e-9 * top
    assert len(got) == len(want) == len(puts)
    for k in range(len(puts)):
        for c in range(CN):
            assert got[k][c][2] == want[k][c][2] and got[k][c][3] == want[k][c][3], (k, c, got[k][c], want[k][c])
            assert abs(got[k][c][0] - want[k][c][0]) <= tol and abs(got[k][c][1] - want[k][c][1]) <= tol, (k, c, got[k][c], want[k][c])
        assert bits(got[k][3][0]) == bits(SET3[0]) and bits(got[k][3][1]) == bits(SET3[1])
        assert got[k][3][2:] == (0, False)
    assert got[0][0][3] and not got[-1][0][3]                  # receiver 0: started before put 0, done inside the feed
    assert not got[2][1][3] and got[3][1][3]                   # receiver 1: started before put 3
    assert got[0][2][:2] == (0.0, 0.0) and got[1][2][3] and abs(got[1][2][1] + 3.0) < 1.0     # receiver 2: SET, STARTCAL
    other = check_states(oracle, pkt_len, form != "blanked")
    assert abs(other[-1][0][0] - want[-1][0][0]) > 100 * tol   # receivers 0, 1: blanker on
    assert abs(other[-1][1][0] - want[-1][1][0]) > 100 * tol
    assert other[-1][2] == want[-1][2]                         # receiver 2: off


# ---- 2. the end of a calibration -----------------------------------------------------------------------------------------
def test_calibration_that_ends_with_a_put_stays_active_until_the_next_datagram():
    """24 bit: 2500 datagrams end on the limit exactly"""
    import cutesdr_amd as ca
    raw, _, _ = feed(1444)
    s = ca.SpurCalBatch(CN)
    s.start_cal(-1)
    s.put_packets(raw[:, :2000]); s.put_packets(raw[:, 2000:2500])
    at_limit = [s.get_state(c) for c in range(CN)]
    assert all(st[2:] == (300000, True) for st in at_limit)
    s.put_packets(raw[:, 2500:2501])                           # the next put's first datagram clears it, nothing else
    after = [s.get_state(c) for c in range(CN)]
    for c in range(CN):
        assert after[c][2:] == (300000, False)
        assert bits(after[c][0]) == bits(at_limit[c][0]) and bits(after[c][1]) == bits(at_limit[c][1])
    # a second STARTCAL: the feed's DC of 150 has converged to 150 (1 - e^-6) = 149.6, plus the impulses' share of the
    # mean: beyond 10, and zeroed; |Q| < 10 is kept
    assert after[0][0] > 149.0 and 0.0 < abs(after[0][1]) < 10.0
    s.start_cal(0)
    again = s.get_state(0)
    assert again[0] == 0.0 and bits(again[1]) == bits(after[0][1]) and again[2:] == (0, True)
    assert s.get_state(1) == after[1]


def test_calibration_overshoots_at_16_bit(oracle):
    """300000 / 128 = 2343.75: datagram 2343 still runs, the count ends at 300032 -- in one put and in the cut feed"""
    import cutesdr_amd as ca
    raw, _, _ = feed(1028)
    s = ca.SpurCalBatch(CN)
    s.start_cal(1)
    s.put_packets(raw)
    assert s.get_state(1)[2:] == (300032, False) and s.get_state(0)[2:] == (0, False)
    for form in ("plain", "blanked"):
        assert run_forms(1028, False)[form][-1][0][2:] == (300032, False)
        assert run_forms(1444, False)[form][-1][0][2:] == (300000, False)
    # one put of 2600 datagrams against the same datagrams in 29 puts: the same calibration within the bound
    i, q = s.get_state(1)[:2]
    r = RefSpurCal(lambda off, x: oracle.spurcal(np.array(off), x)); r.start_cal()
    x = oracle.unpack_packets(raw[1], 1028)
    for p in range(raw.shape[1]):
        r.call(256, x[p * 256:(p + 1) * 256])
    tol = 1e-9 * feed(1028)[2]
    assert abs(i - r.off[0]) <= tol and abs(q - r.off[1]) <= tol and r.count == 300032


# ---- 3. word for word ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pkt_len", [1444, 1028])
def test_the_forms_give_the_same_words(pkt_len):
    r = run_forms(pkt_len, False)
    same_words(r["blanked"], r["two_pass"])                    # the blanked put = a blanker pass into rows + put_stream
    same_words(r["plain"], r["unpacked"])                      # put_packets = unpack + put_stream
    for k in range(len(r["plain"])):                           # blanker off: the blanked put = the unblanked one
        assert r["blanked"][k][2][2:] == r["plain"][k][2][2:]
        assert bits(r["blanked"][k][2][0]) == bits(r["plain"][k][2][0]) and bits(r["blanked"][k][2][1]) == bits(r["plain"][k][2][1])
    assert bits(r["blanked"][-1][0][0]) != bits(r["plain"][-1][0][0])       # ... blanker on: other samples


# ---- 4. commands ---------------------------------------------------------------------------------------------------------
def test_commands():
    import cutesdr_amd as ca
    L = ca.lib()
    raw, _, _ = feed(1444)
    s = ca.SpurCalBatch(CN)
    assert [s.get_state(c) for c in range(CN)] == [(0.0, 0.0, 0, False)] * CN
    s.start_cal(-1)                                            # channel -1: every receiver
    assert all(s.get_state(c)[2:] == (0, True) for c in range(CN))
    s.put_packets(raw[:, :40])
    mid = [s.get_state(c) for c in range(CN)]
    assert all(st[2:] == (40 * 120, True) and st[0] != 0.0 for st in mid)
    assert s.read(1) == mid[1][:2]                             # READ in mid-calibration stops it (:793) ...
    assert s.get_state(1) == mid[1][:3] + (False,)
    s.put_packets(raw[:, 40:80])                               # ... and the next put changes nothing of receiver 1
    assert s.get_state(1) == mid[1][:3] + (False,)
    assert s.get_state(0)[2:] == (80 * 120, True) and s.get_state(0)[0] != mid[0][0]
    # order between puts
    s.set(50.0, -3.0, 2); s.start_cal(2)
    assert s.get_state(2) == (0.0, -3.0, 0, True)
    s.start_cal(3); s.set(50.0, -3.0, 3)
    assert s.get_state(3) == (50.0, -3.0, 0, False)
    s.set(1.5, -2.5, -1)
    assert [s.get_state(c) for c in range(CN)] == [(1.5, -2.5, 80 * 120, False), (1.5, -2.5, 40 * 120, False),
                                                   (1.5, -2.5, 0, False), (1.5, -2.5, 0, False)]
    # an empty put applies pending commands: what was commanded stands in front of the put's stream afterwards
    part = np.ascontiguousarray(raw[:, :4])
    dp, do = ca.DeviceBuffer(part.nbytes), ca.DeviceBuffer(CN * 4 * 240 * 8)
    dp.upload(part)
    plain = ca.unpack_packets_batch(part, 1444)
    s.set(250.0, -125.0, 1)
    s.put_packets_ptr(dp.ptr, 0, 1444)
    assert L.csdr_ingest_unpack(0, C.c_void_p(dp.ptr), CN, 4, 1444, C.c_void_p(do.ptr), 4 * 240, C.c_void_p(s.dc_ptr), None) == 4 * 240
    ca.sync()
    got = do.download(np.complex64, CN * 4 * 240).reshape(CN, -1)
    for c, (i, q) in enumerate([(1.5, -2.5), (250.0, -125.0), (1.5, -2.5), (1.5, -2.5)]):
        want = ((plain[c].real.astype(np.float64) - i).astype(np.float32) + 1j * (plain[c].imag.astype(np.float64) - q).astype(np.float32))
        assert np.array_equal(got[c], want.astype(np.complex64)), c
    assert s.get_state(1) == (250.0, -125.0, 40 * 120, False)
    dp.free(); do.free()


def test_row_form_with_odd_call_lengths(oracle):
    """put_stream with a call length that divides nothing and a short last call, runs that begin inside a tile: count by
    the rule, offsets against the per-call loop"""
    import cutesdr_amd as ca
    raw, _, top = feed(1028)
    x = ca.unpack_packets_batch(np.ascontiguousarray(raw[:, :70]), 1028)      # 17920 samples: more than one tile
    s = ca.SpurCalBatch(CN)
    s.set(3.0, -4.0, -1); s.start_cal(-1)
    refs = [RefSpurCal(lambda off, v: oracle.spurcal(np.array(off), v)) for _ in range(CN)]
    for r in refs:
        r.set(3.0, -4.0); r.start_cal()
    for a, b, call_len in ((0, 1, 7), (1, 17001, 1001), (17001, 17920, 100)):
        s.put_stream(x[:, a:b], call_len)
        for c in range(CN):
            for p in range(a, b, call_len):
                v = x[c, p:min(p + call_len, b)].astype(np.complex128)
                refs[c].call(len(v), v)
            got = s.get_state(c)
            assert got[2:] == refs[c].state()[2:], (a, b, c)
            assert abs(got[0] - refs[c].off[0]) <= 1e-9 * top and abs(got[1] - refs[c].off[1]) <= 1e-9 * top


# ---- 5. with the display ---------------------------------------------------------------------------------------------------
def test_offsets_feed_the_blanked_display(oracle):
    """dc() handed to put_display_packets_blanked behind the put: the spectrum of the checker's display loop with the
    offsets as they stand after each put (the display stream's rule for a put's samples)"""
    import cutesdr_amd as ca
    L = ca.lib()
    N, pkt_len, per, ave = 2048, 1444, 240, 3
    raw, puts, _ = feed(pkt_len)
    puts = puts[:6]
    b, (nb,) = make_chain(ca), make_blankers(ca, 1)
    s = ca.SpurCalBatch(CN)
    f = ca.FftBatch(CN)
    f.set_params(N, False, 0.0, FS); f.set_ave(ave); f.set_display_rate(FS, 10, False)
    want_states = check_states(oracle, pkt_len, True)
    disp = [OracleDisplay(oracle, N, ave, FS, 1, False) for _ in range(CN)]
    nbs = []
    for c in range(CN):
        q = oracle.CNoiseProc(); q.SetupBlanker(ON[c], THRESH, width_us(c), FS); nbs.append(q)
    cap = audio_cap([p * per for p in puts])
    dout = ca.DeviceBuffer(4 * CN * cap)
    p0, frames = 0, 0
    for k, npk in enumerate(puts):
        for c, name, args in commands(k):
            command_device(s, c, name, args)
        part = np.ascontiguousarray(raw[:, p0:p0 + npk]); p0 += npk
        dp = ca.DeviceBuffer(part.nbytes); dp.upload(part)
        assert chain_call(L, b, nb, dp, npk, pkt_len, dout, cap) == 0
        s.put_packets_blanked_ptr(b, dp.ptr, npk, pkt_len)
        got = f.put_display_packets_blanked_ptr(b, dp.ptr, npk, pkt_len, s.dc_ptr)
        ca.sync()
        dp.free()
        want = []
        for c in range(CN):
            disp[c].dc = np.array(want_states[k][c][:2])
            want.append(disp[c].process(nbs[c].ProcessBlanker(oracle.unpack_packets(part[c], pkt_len)), False))
        assert got == want[0] == want[1] == want[2] == want[3]
        frames += got
    assert frames >= 4
    for c in range(CN):
        assert f.total_count(c) == disp[c].total
        assert_spectrum_close(f.ave_buf(c).astype(np.float64), disp[c].fft.ave_buf())
    dout.free()


# ---- 6. pipelined chain --------------------------------------------------------------------------------------------------
def test_pipelined_chain_gives_the_strict_mode_words():
    same_words(run_forms(1444, True)["blanked"], run_forms(1444, False)["blanked"])


# ---- 7. the contract's refusals --------------------------------------------------------------------------------------------
def test_contract_refusals_leave_the_state_alone():
    """CSDR_ESTATE without a blanked call to stand behind, CSDR_EINVAL for another input, form or width; the state after
    every refusal is the state before it, to the bit"""
    import cutesdr_amd as ca
    L = ca.lib()
    pkt_len, per, npk = 1444, 240, 64
    n = npk * per
    raw, _, _ = feed(pkt_len)
    b, (nb,) = make_chain(ca), make_blankers(ca, 1)
    s, wide = ca.SpurCalBatch(CN), ca.SpurCalBatch(CN + 1)
    s.set(2.0, -1.0, -1); s.start_cal(-1); wide.start_cal(-1)
    cap = audio_cap([n])
    dout = ca.DeviceBuffer(4 * CN * cap)
    dps = []
    for k in range(3):
        dp = ca.DeviceBuffer(CN * npk * pkt_len); dp.upload(np.ascontiguousarray(raw[:, k * npk:(k + 1) * npk])); dps.append(dp)
    drows = ca.DeviceBuffer(CN * n * 8); drows.upload(np.zeros((CN, n), dtype=np.complex64))

    def state(o=s, channels=CN):
        return [o.get_state(c) for c in range(channels)]

    def packets(o, dp, count=npk, length=pkt_len):
        return L.csdr_spurcal_batch_put_packets_blanked(o.h, b.h, C.c_void_p(dp.ptr), count, length, None)

    def rows(o):
        return L.csdr_spurcal_batch_put_stream_blanked(o.h, b.h, C.c_void_p(drows.ptr), n, n, per, None)

    def refused(rc, want):
        before = state()
        assert rc() == want
        assert state() == before

    refused(lambda: packets(s, dps[0]), ESTATE)                # no blanked call yet
    assert chain_call(L, b, nb, dps[0], npk, pkt_len, dout, cap) == 0
    refused(lambda: packets(s, dps[0], npk - 32), EINVAL)      # another count
    refused(lambda: packets(s, dps[1]), EINVAL)                # another buffer
    refused(lambda: packets(s, dps[0], npk, 1028), EINVAL)     # another packet length
    refused(lambda: rows(s), EINVAL)                           # rows behind a datagram call
    assert packets(wide, dps[0]) == EINVAL                     # another width
    assert state(wide, CN + 1) == [(0.0, 0.0, 0, True)] * (CN + 1)
    assert packets(s, dps[0]) == 0
    assert all(st[2:] == (npk * 120, True) for st in state())
    assert L.csdr_demod_batch_process(b.h, C.c_void_p(drows.ptr), n, n, C.c_void_p(dout.ptr), cap, None) == 0
    refused(lambda: packets(s, dps[0]), ESTATE)                # an unblanked call since
    refused(lambda: rows(s), ESTATE)
    assert chain_call(L, b, nb, dps[1], npk, pkt_len, dout, cap) == 0
    assert packets(s, dps[1]) == 0
    assert all(st[2:] == (2 * npk * 120, True) for st in state())
    ca.sync()
    for o in dps + [drows, dout]:
        o.free()
