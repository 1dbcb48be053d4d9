"""GPU checks of the row form of the spectrum batch (csdr_fft_batch_*_row, csdr_fft_batch_get_emits,
csdr_plotter_batch_draw_emitted): averaging length, display rate, screen gate and acknowledge per row, the frame
position shared.  Each row against its own fp64 display loop (OracleDisplay, one per row); the bin-resolving rule of
k3_bins.py with frame groups; word for word against the uniform object that carries the row's settings; equal settings
through the row form; independence of how the stream is cut; row isolation of the setters; behind a blanked chain call;
the plotter's draw of the rows that emitted; the refusals.

One sample rate serves every row: fs = 60 N + 1, where display rates 60 / 30 / 20 / 12 / 10 / 1 give the skip values
1 / 2 / 3 / 5 / 6 / 60 (and 61 gives 0).  Calls stay below 16 used frames per row wherever words are compared: from 16
frames on a row's frames are cut into frame groups and the running mean rounds as the groups fall."""
import ctypes as C
import functools
import numpy as np
import pytest

import k3_bins as K
import test_display_blanked_gpu as B
from test_display_stream_gpu import make_packets, OracleDisplay, feed_signal
from test_fft_resampler_gpu import assert_spectrum_close
from test_plotter_gpu import Pair, frame, own_screen

pytestmark = pytest.mark.gpu

EINVAL = -1
RATE = {0: 61, 1: 60, 2: 30, 3: 20, 5: 12, 6: 10, 60: 1}
#        ave, skip, gated
FIVE = [(1, 1, False),      # every frame
        (3, 3, True),       # acknowledged at random
        (2, 5, False),
        (4, 1, True),       # never acknowledged: exactly one frame ever
        (2, 60, False)]     # no frame in most calls


def fs_of(N):
    return float(60 * N + 1)


def dc_of(c):
    return np.array([150.0, -90.0]) * (1 + 0.2 * c)             # the offsets feed_signal adds


def row_object(ca, N, settings):
    b = ca.FftBatch(len(settings))
    b.set_params(N, False, 0.0, fs_of(N))
    b.set_display_rate(fs_of(N), 60)                            # the object's sample rate
    for r, (ave, skip, gated) in enumerate(settings):
        b.set_ave_row(r, ave)
        b.set_display_rate_row(r, RATE[skip], gated)
    assert b.row_form()
    return b


def uniform_object(ca, N, channels, ave, skip, gated):
    u = ca.FftBatch(channels)
    u.set_params(N, False, 0.0, fs_of(N)); u.set_ave(ave)
    u.set_display_rate(fs_of(N), RATE[skip], gated)
    assert not u.row_form()
    return u


def row_state(ca, b, row):
    """(bels, running sum, [ave_count, total_count]) of one row, as words"""
    L = ca.lib()
    L.csdr__fft_batch_row_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    sm = np.zeros(b.size(), dtype=np.float32); cnt = np.zeros(2, dtype=np.int32)
    assert L.csdr__fft_batch_row_state(b.h, row, sm.ctypes.data, cnt.ctypes.data) == 0
    return b.ave_buf(row).view(np.uint32).copy(), sm.view(np.uint32).copy(), cnt.copy()


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def overloads(b):
    return [bool(v) for v in b.screen_all(1, 1, 0.0, -160.0, -1000, 1000)[0]]


def ragged_calls(rng, N, unit, need, top_frames):
    """call lengths in units (packets, or samples for unit 1): ragged, some completing no frame, until `need` samples.
    The first call ends inside frame 2: frame 1 is the last one it completes."""
    per_frame = max(N // unit, 1)
    calls = [(2 * N + N // 4) // unit + 1]
    tot, k = calls[0] * unit, 0
    while tot < need:
        if k % 7 == 3:
            c = int(rng.integers(1, max(per_frame // 3, 2)))    # completes no frame, twice in a row
            calls += [c, c]; tot += 2 * c * unit
        c = int(rng.integers(1, top_frames * per_frame))
        calls.append(c); tot += c * unit
        k += 1
    return calls


# ---- 1. each row against its own fp64 display loop -------------------------------------------------------------------
@pytest.mark.parametrize("N,pkt_len", [(2048, 1028), (4096, 1444), (8192, 1444), (16384, 1028), (1024, 1444),
                                       (32768, 1444), (4096, 0)])
def test_rows_match_their_own_display_loop(oracle, N, pkt_len):
    """pkt_len 0: fp32 rows with d_dc.  Per call get_emits equals the five loops' counts and the return value their
    maximum; at the end total_count, bels (K3 tolerance), the screen (one pixel) and the overload flags."""
    import cutesdr_amd as ca
    fs, Cn = fs_of(N), len(FIVE)
    per = {1444: 240, 1028: 256, 0: 1}[pkt_len]
    rng = np.random.default_rng(N + pkt_len)
    calls = ragged_calls(rng, N, per, 62 * N, 3 if N <= 8192 else 14)
    tot = sum(calls) * per
    x = feed_signal(Cn, tot, fs, seed=N + 1)
    for c in (0, 2):
        x[c, N + N // 3] = 32700.0 + 0j                         # frame 1: row 0 uses it, row 2 (skip 5) does not
    data = make_packets(x, pkt_len) if pkt_len else x.astype(np.complex64)
    dc = np.stack([dc_of(c) for c in range(Cn)])
    b = row_object(ca, N, FIVE)
    refs = [OracleDisplay(oracle, N, ave, fs, skip, gated) for ave, skip, gated in FIVE]
    for c, r in enumerate(refs):
        r.dc = dc[c]
    p0 = 0
    for ci, k in enumerate(calls):
        part = np.ascontiguousarray(data[:, p0:p0 + k]); p0 += k
        got = b.put_display_packets(part, pkt_len, dc) if pkt_len else b.put_display_stream(part, dc)
        rows = [oracle.unpack_packets(part[c], pkt_len) if pkt_len else part[c].astype(np.complex128) for c in range(Cn)]
        want = [r.process(rows[c], False) for c, r in enumerate(refs)]
        assert list(b.emits()) == want, ci
        assert got == max(want), ci
        if ci < 3:                                               # around the spike: the flag is the row's last used frame's
            ov = overloads(b)
            assert ov == [bool(r.fft.GetScreenIntegerFFTData(1, 1, 0.0, -160.0, -1000, 1000)[0]) for r in refs], ci
            if ci == 0:
                assert ov == [True, False, False, False, False]  # frame 1 is this call's last: it flags row 0 only
        if rng.random() < 0.5:
            b.screen_update_done_row(1); refs[1].finished = True
    assert refs[3].total == 1 and refs[4].total >= 1 and refs[0].total >= 62
    for c in range(Cn):
        assert b.total_count(c) == refs[c].total, c
        assert_spectrum_close(b.ave_buf(c).astype(np.float64), refs[c].fft.ave_buf())
    ov, pix = b.screen_all(255, 700, 0.0, -160.0, -int(fs / 2), int(fs / 2))
    for c in range(Cn):
        want_ov, want = refs[c].fft.GetScreenIntegerFFTData(255, 700, 0.0, -160.0, -int(fs / 2), int(fs / 2))
        assert ov[c] == want_ov
        touched = pix[c] >= 0
        assert np.abs(pix[c][touched] - want[touched]).max() <= 1


def test_overload_flag_is_the_rows_own_last_used_frame():
    """a spike in frame 1, which row 0 uses and row 1 (skip 5) skips, on both rows' input: it flags row 0 only, and only
    until row 0's next used frame; a row that uses no frame keeps its word"""
    import cutesdr_amd as ca
    N = 2048
    b = row_object(ca, N, [(1, 1, False), (2, 5, False), (1, 1, False)])
    x = feed_signal(3, 6 * N, fs_of(N), seed=2, dc=(0.0, 0.0)).astype(np.complex64)
    x[0, N + 7] = x[1, N + 7] = 32700.0
    x[2, 4 * N + 9] = 32700.0
    assert b.put_display_stream(x[:, :2 * N + 100]) == 2 and list(b.emits()) == [2, 0, 2]
    assert overloads(b) == [True, False, False]
    assert b.put_display_stream(x[:, 2 * N + 100:3 * N + 50]) == 1 and list(b.emits()) == [1, 0, 1]
    assert overloads(b) == [False, False, False]
    assert b.put_display_stream(x[:, 3 * N + 50:5 * N]) == 2 and list(b.emits()) == [2, 1, 2]     # frames 3, 4
    assert overloads(b) == [False, False, True]
    b.set_display_rate_row(2, RATE[60])
    assert b.put_display_stream(x[:, 5 * N:]) == 1 and list(b.emits()) == [1, 0, 0]
    assert overloads(b) == [False, False, True]                  # row 2 used no frame: its word stays


# ---- 2. the bin-resolving bound, with frame groups -------------------------------------------------------------------
@pytest.mark.parametrize("n", [2048, 4096])
def test_bin_resolving_bound_with_frame_groups(oracle, n):
    """three rows of 40 frames in one call: row 0 uses 40 (ave 2), row 1 every third, 13 (ave 5), row 2 is gated and not
    ready.  40 frames on two active rows are five frame groups for row 0; row 1, below 16 frames, runs as one."""
    import cutesdr_amd as ca
    x = K.frames(n, 3, 41)
    b = row_object(ca, n, [(2, 1, False), (5, 3, False), (3, 1, True)])
    assert b.put_display_stream(x[:, 0]) == 1                    # row 2 takes a frame: its gate is closed from here on
    for r, (ave, skip) in enumerate([(2, 1), (5, 3)]):           # rows 0 and 1 from scratch: spectrum, counter
        b.set_ave_row(r, ave); b.set_display_rate_row(r, RATE[skip])
    before = row_state(ca, b, 2)
    assert before[0].any() and before[1].any() and list(before[2]) == [1, 1]
    assert b.put_display_stream(x[:, 1:].reshape(3, 40 * n)) == 40
    assert list(b.emits()) == [40, 13, 0]
    assert same_state(row_state(ca, b, 2), before)
    assert b.total_count(0) == 40 and b.total_count(1) == 13
    ref, e_y = K.reference(oracle, x[0, 1:], 2)
    K.check(b.ave_buf(0), ref, e_y, n, "row 0, five frame groups")
    ref, e_y = K.reference(oracle, x[1, 1:][2::3], 5)
    K.check(b.ave_buf(1), ref, e_y, n, "row 1, one group")


# ---- 3. the words of the uniform path --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_against_uniform(N, pkt_len):
    """the row-form object with the settings FIVE, and one uniform object of the same width per setting, on the same
    calls (at most 15 frames each) -> per call and object (counts, per-row words, totals, overload flags)"""
    import cutesdr_amd as ca
    fs, Cn = fs_of(N), len(FIVE)
    per = {1444: 240, 1028: 256, 0: 1}[pkt_len]
    rng = np.random.default_rng(3 * N + pkt_len)
    calls = ragged_calls(rng, N, per, 61 * N, 14)
    x = feed_signal(Cn, sum(calls) * per, fs, seed=N + 5)
    x[:, N + 11] = 32700.0 + 0j
    data = make_packets(x, pkt_len) if pkt_len else x.astype(np.complex64)
    dc = np.stack([dc_of(c) for c in range(Cn)])
    b = row_object(ca, N, FIVE)
    us = [uniform_object(ca, N, Cn, *s) for s in FIVE]
    out, p0 = [], 0
    for ci, k in enumerate(calls):
        part = np.ascontiguousarray(data[:, p0:p0 + k]); p0 += k
        put = (lambda o: o.put_display_packets(part, pkt_len, dc)) if pkt_len else (lambda o: o.put_display_stream(part, dc))
        got = put(b)
        counts = [put(u) for u in us]
        rec = {"ret": got, "emits": list(b.emits()), "counts": counts, "uemits": [list(u.emits()) for u in us]}
        rec["over"] = (overloads(b), [overloads(u)[r] for r, u in enumerate(us)])
        if ci % 5 == 0 or ci == len(calls) - 1:
            rec["rows"] = [(b.ave_buf(r).view(np.uint32).copy(), b.total_count(r)) for r in range(Cn)]
            rec["uni"] = [(u.ave_buf(r).view(np.uint32).copy(), u.total_count(r)) for r, u in enumerate(us)]
        out.append(rec)
        if rng.random() < 0.5:
            b.screen_update_done_row(1); us[1].screen_update_done()
    return out


@pytest.mark.parametrize("N", [2048, 4096, 16384])
@pytest.mark.parametrize("pkt_len", [1444, 0])
def test_row_equals_uniform_object_with_its_settings(N, pkt_len):
    out = rows_against_uniform(N, pkt_len)
    assert max(max(r["counts"]) for r in out) < 16
    compared = 0
    for ci, rec in enumerate(out):
        assert rec["emits"] == rec["counts"] and rec["ret"] == max(rec["counts"]), ci
        for r, e in enumerate(rec["uemits"]):
            assert e == [rec["counts"][r]] * len(FIVE)           # get_emits of the uniform form: every entry the same
        assert rec["over"][0] == rec["over"][1], ci
        if "rows" in rec:
            for r in range(len(FIVE)):
                assert rec["rows"][r][1] == rec["uni"][r][1], (ci, r)
                assert np.array_equal(rec["rows"][r][0], rec["uni"][r][0]), (ci, r)
            compared += 1
    assert compared >= 3 and out[-1]["rows"][4][1] >= 1 and out[-1]["rows"][3][1] == 1
    assert out[0]["over"][0] == [True, False, False, False, False]       # the spike in frame 1: row 0's last used frame


# ---- 4. equal settings through the row form --------------------------------------------------------------------------
@pytest.mark.parametrize("N,pkt_len", [(4096, 1444), (2048, 0), (1024, 1028)])
def test_equal_settings_through_the_row_form(N, pkt_len):
    import cutesdr_amd as ca
    fs, Cn = fs_of(N), 4
    per = {1444: 240, 1028: 256, 0: 1}[pkt_len]
    rng = np.random.default_rng(N)
    calls = ragged_calls(rng, N, per, 30 * N, 10)
    data = feed_signal(Cn, sum(calls) * per, fs, seed=N + 9)
    data = make_packets(data, pkt_len) if pkt_len else data.astype(np.complex64)
    u = uniform_object(ca, N, Cn, 3, 3, True)
    b = ca.FftBatch(Cn)
    b.set_params(N, False, 0.0, fs); b.set_display_rate(fs, 60)
    b.set_ave_row(2, 7)                                          # into the row form ...
    b.set_ave_row(-1, 3); b.set_display_rate_row(-1, RATE[3], True)      # ... and every row the same settings
    assert b.row_form()
    p0, frames = 0, 0
    for ci, k in enumerate(calls):
        part = np.ascontiguousarray(data[:, p0:p0 + k]); p0 += k
        put = (lambda o: o.put_display_packets(part, pkt_len)) if pkt_len else (lambda o: o.put_display_stream(part))
        got = put(b)
        assert got == put(u) and list(b.emits()) == [got] * Cn, ci
        frames += got
        for r in range(Cn):
            assert b.total_count(r) == u.total_count(r)
            assert np.array_equal(b.ave_buf(r).view(np.uint32), u.ave_buf(r).view(np.uint32)), (ci, r)
        if rng.random() < 0.5:
            b.screen_update_done(); u.screen_update_done()      # object-wide: every row ready
    assert frames >= 3 and b.row_form()


# ---- 5. cutting ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dc", [(4096, True), (2048, False), (16384, False), (1024, True)])
def test_call_cutting_does_not_matter(N, dc):
    """one call of 40 N + 777 samples gives the words of the same samples cut into ragged calls; every row stays below
    16 frames (skips 3, 5, 6, a closed gate, 60), so no row is cut into frame groups on either side"""
    import cutesdr_amd as ca
    settings = [(4, 3, False), (2, 5, False), (3, 6, False), (2, 1, True), (2, 60, False)]
    Cn, fs, n = len(settings), fs_of(N), 40 * N + 777
    x = feed_signal(Cn, n, fs, seed=5).astype(np.complex64)
    d = np.array([[12.5, -3.25]] * Cn) if dc else None
    a, b = row_object(ca, N, settings), row_object(ca, N, settings)
    assert a.put_display_stream(x, d) == 13 and list(a.emits()) == [13, 8, 6, 1, 0]
    rng = np.random.default_rng(N)
    tot, p = np.zeros(Cn, dtype=np.int64), 0
    while p < n:
        k = int(min(n - p, rng.integers(1, 3 * N)))
        b.put_display_stream(x[:, p:p + k], d)
        tot += b.emits()
        p += k
    assert list(tot) == [13, 8, 6, 1, 0]
    for c in range(Cn):
        assert same_state(row_state(ca, a, c), row_state(ca, b, c)), c
    tail = feed_signal(Cn, N, fs, seed=6).astype(np.complex64)   # the carry is the same: one more frame completes alike
    for o in (a, b):
        o.set_display_rate_row(-1, RATE[0])
    assert a.put_display_stream(tail, d) == b.put_display_stream(tail, d) == 1
    for c in range(Cn):
        assert a.total_count(c) == int(tot[c]) + 1
        assert same_state(row_state(ca, a, c), row_state(ca, b, c)), c


# ---- 6. row isolation ------------------------------------------------------------------------------------------------
def test_setters_touch_their_row_only():
    import cutesdr_amd as ca
    N, Cn = 2048, 4
    fs = fs_of(N)
    x = feed_signal(Cn, 12 * N, fs, seed=8).astype(np.complex64)
    b = row_object(ca, N, [(2, 1, False), (3, 2, True), (4, 1, True), (2, 3, False)])
    assert b.put_display_stream(x[:, :4 * N]) == 4 and list(b.emits()) == [4, 1, 1, 1]
    st = [row_state(ca, b, r) for r in range(Cn)]
    assert all(s[0].any() and s[1].any() for s in st)
    b.set_ave_row(1, 5)                                          # SetFFTAve of row 1: that row is reset, nobody else
    got = [row_state(ca, b, r) for r in range(Cn)]
    assert not got[1][0].any() and not got[1][1].any() and list(got[1][2]) == [0, 0]
    assert all(same_state(got[r], st[r]) for r in (0, 2, 3))
    b.reset_row(3)
    got = [row_state(ca, b, r) for r in range(Cn)]
    assert not got[3][1].any() and list(got[3][2]) == [0, 0] and all(same_state(got[r], st[r]) for r in (0, 2))
    # rows 1 and 2 are gated and have had their frame: only the acknowledged one gets the next
    # (row 3, skip 3, selects frames 2 and 5: reset_row cleared its spectrum, not its skip counter)
    assert b.put_display_stream(x[:, 4 * N:6 * N]) == 2 and list(b.emits()) == [2, 0, 0, 1]
    b.screen_update_done_row(2)
    assert b.put_display_stream(x[:, 6 * N:8 * N]) == 2 and list(b.emits()) == [2, 0, 1, 0]
    # set_params: every row's skip from its own stored rate, counters 0 -- twice the size at the same sample rate:
    # (int)((60 N + 1) / (2 N rate)) = 2 / 1 / 0 / 1 for the rates 12 / 30 / 60 / 20
    b.set_display_rate_row(0, RATE[5])
    b.set_params(2 * N, False, 0.0, fs)
    b.screen_update_done()
    skips = [int(fs / (2 * N * RATE[s])) for s in (5, 2, 1, 3)]
    assert skips == [2, 1, 0, 1]
    y = feed_signal(Cn, 12 * N, fs, seed=9).astype(np.complex64)   # six frames of 2 N
    assert b.put_display_stream(y) == 6
    assert list(b.emits()) == [3, 1, 1, 6]                       # rows 1 and 2 are gated: one frame
    # the object-wide setters write every row and end the row form
    b.set_display_rate(fs, RATE[2])                              # skip 1 at this size, no gate
    assert b.row_form()                                          # the averaging lengths are still per row
    b.set_ave(2)
    assert not b.row_form()
    assert b.put_display_stream(y[:, :8 * N]) == 4 and list(b.emits()) == [4] * Cn


def test_display_rate_object_wide_returns_to_the_uniform_words():
    """after set_ave and set_display_rate (object-wide) a former row-form object gives the words of one that never left"""
    import cutesdr_amd as ca
    N, Cn = 4096, 3
    fs = fs_of(N)
    x = feed_signal(Cn, 9 * N + 300, fs, seed=12).astype(np.complex64)
    b = row_object(ca, N, [(2, 1, False), (3, 2, True), (4, 5, False)])
    b.put_display_stream(x[:, :N + 5])
    b.stream_reset()
    b.set_ave(3); b.set_display_rate(fs, RATE[2])
    u = uniform_object(ca, N, Cn, 3, 2, False)
    assert not b.row_form()
    assert b.put_display_stream(x) == u.put_display_stream(x) == 4
    for r in range(Cn):
        assert same_state(row_state(ca, b, r), row_state(ca, u, r))


# ---- 7. behind a blanked chain call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N", [(1444, 4096), ("rows", 2048), (1028, 16384)])
def test_blanked_rows_equal_uniform_blanked_objects(form, N):
    """mixed rows behind process_packets with a blanker / process_blanked: each row equals the uniform blanked object
    with that row's settings, bit for bit (calls of at most 14 frames)"""
    import cutesdr_amd as ca
    L = ca.lib()
    pkt_len = form if form != "rows" else 0
    per = 240 if pkt_len == 1444 else 256
    unit = 7680 if pkt_len == 1444 else 512
    fs = fs_of(N)
    settings = [(2, 1, False), (3, 3, True), (1, 2, False)]
    calls = B.call_lengths(N, unit, 9.5 * N, max_frames=14)
    x = B.make_feed(N, fs, calls, seed=N + pkt_len + 1)
    x[2, N + N // 4] = 32700.0                                   # receiver 2 (blanker off: the sample stays) overloads in frame 1
    data = make_packets(x, pkt_len) if pkt_len else x.astype(np.complex64)
    chain, (nb,) = B.make_chain(ca), B.make_blankers(ca, fs)
    b = row_object(ca, N, settings)
    us = [uniform_object(ca, N, B.CN, *s) for s in settings]
    ddc = ca.DeviceBuffer(B.CN * 16); ddc.upload(np.stack([B.dc_of(c) for c in range(B.CN)]))
    cap = B.audio_cap(calls)
    dout = ca.DeviceBuffer(4 * B.CN * cap)
    p0, frames = 0, np.zeros(B.CN, dtype=np.int64)
    for k, n in enumerate(calls):
        cnt = n // per if pkt_len else n
        part = np.ascontiguousarray(data[:, p0:p0 + cnt]); p0 += cnt
        din = ca.DeviceBuffer(part.nbytes); din.upload(part)
        if pkt_len:
            assert L.csdr_demod_batch_process_packets(chain.h, C.c_void_p(din.ptr), cnt, pkt_len, nb.h, C.c_void_p(dout.ptr), cap, None) == 0
            put = lambda o: o.put_display_packets_blanked_ptr(chain, din.ptr, cnt, pkt_len, ddc.ptr)
        else:
            assert L.csdr_demod_batch_process_blanked(chain.h, C.c_void_p(din.ptr), n, n, nb.h, C.c_void_p(dout.ptr), cap, None) == 0
            put = lambda o: o.put_display_stream_blanked_ptr(chain, din.ptr, n, n, ddc.ptr)
        got = put(b)
        counts = [put(u) for u in us]
        ca.sync()
        din.free()
        assert list(b.emits()) == counts and got == max(counts) and max(counts) < 16, k
        frames += counts
        assert overloads(b) == [overloads(u)[r] for r, u in enumerate(us)], k
        for r, u in enumerate(us):
            assert b.total_count(r) == u.total_count(r)
            assert np.array_equal(b.ave_buf(r).view(np.uint32), u.ave_buf(r).view(np.uint32)), (k, r)
        if k % 2 == 0:
            b.screen_update_done_row(1); us[1].screen_update_done()
    chain.flush()
    assert frames[0] >= 9 and frames[1] >= 1 and frames[2] >= 4
    for o in (ddc, dout):
        o.free()


# ---- 8. the plotter draws the rows that emitted ----------------------------------------------------------------------
def test_draw_emitted_draws_the_rows_that_emitted():
    import cutesdr_amd as ca
    n, rows = 2048, 4
    fs = 1000.0 * n
    b = ca.FftBatch(rows)
    b.set_params(n, False, 0.0, fs); b.set_display_rate(fs, 100000)       # skip 0
    for r in range(rows):
        b.set_ave_row(r, 1); b.set_display_rate_row(r, 100000, gated=(r % 2 == 1))
    q = Pair(ca, 6, [0, 1, 2, 3, 2, 0])                          # views 0 and 5 on row 0, 2 and 4 on row 2; view 5 stopped
    for v in range(6):
        q.slot("SetPercent2DScreen", 40 + 5 * v, view=v)
        q.slot("SetSpanFreq", int(0.5 * fs) // (v + 1), view=v)
        q.slot("resizeEvent", 150 + 30 * v, 90 + 10 * v, view=v)
        q.slot("SetRunningState", v != 5, view=v)
    assert b.put_display_stream(frame(1, n, fs, rows=rows, hot=(1,))) == 1 and list(b.emits()) == [1, 1, 1, 1]
    assert q.draw(b) == 5                                        # every running view once: trace, line and pen are real words
    q.check("first draw")
    before = {v: (q.p.trace(v)[0].copy(), q.p.trace(v)[1], q.p.waterfall(v).copy()) for v in (1, 3, 5)}
    assert before[1][1] and not before[3][1]                     # row 1 overloaded: view 1's pen is red
    # rows 1 and 3 are gated and not acknowledged: the next frame reaches rows 0 and 2 only
    assert b.put_display_stream(frame(2, n, fs, rows=rows, hot=(2,))) == 1 and list(b.emits()) == [1, 0, 1, 0]
    assert q.p.draw_emitted(b) == 3                              # views 0, 2, 4
    for v in (0, 2, 4):
        mapping, over = own_screen(ca, b, q.rows[v])
        q.refs[v].draw(mapping, over)
    q.check("after draw_emitted")                                # views 1, 3, 5: their reference was not drawn either
    for v in (1, 3, 5):
        y, red = q.p.trace(v)
        assert np.array_equal(y, before[v][0]) and red == before[v][1], v
        assert np.array_equal(q.p.waterfall(v), before[v][2]), v
    assert q.p.trace(2)[1] and q.p.trace(4)[1] and not q.p.trace(0)[1]     # row 2's pen went red with this frame
    # a call that uses no frame: nothing is drawn
    assert b.put_display_stream(frame(3, n, fs, rows=rows)[:, :100]) == 0
    assert q.p.draw_emitted(b) == 0
    q.check("no frame, no draw")


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_rows_out_of_range_are_refused_and_change_nothing():
    import cutesdr_amd as ca
    L = ca.lib()
    N, Cn = 2048, 3
    b = row_object(ca, N, [(2, 1, False), (3, 2, True), (1, 3, False)])
    x = feed_signal(Cn, 5 * N, fs_of(N), seed=4).astype(np.complex64)
    assert b.put_display_stream(x) == 5
    st, em = [row_state(ca, b, r) for r in range(Cn)], list(b.emits())
    for row in (Cn, Cn + 5, 1 << 20):
        assert L.csdr_fft_batch_set_ave_row(b.h, row, 9) == EINVAL
        assert L.csdr_fft_batch_reset_row(b.h, row) == EINVAL
        assert L.csdr_fft_batch_set_display_rate_row(b.h, row, 10, 1) == EINVAL
        assert L.csdr_fft_batch_screen_update_done_row(b.h, row) == EINVAL
    assert L.csdr_fft_batch_set_display_rate_row(b.h, 0, 0, 0) == EINVAL       # a display rate below 1
    assert L.csdr_fft_batch_get_emits(b.h, None) == EINVAL
    assert list(b.emits()) == em and all(same_state(row_state(ca, b, r), st[r]) for r in range(Cn))
    # ... and the settings: the same next call as an object that was never asked
    c = row_object(ca, N, [(2, 1, False), (3, 2, True), (1, 3, False)])
    c.put_display_stream(x)
    assert b.put_display_stream(x) == c.put_display_stream(x) and list(b.emits()) == list(c.emits())
    for r in range(Cn):
        assert same_state(row_state(ca, b, r), row_state(ca, c, r))
    u = ca.FftBatch(Cn)                                          # a refusal does not move an object into the row form
    assert L.csdr_fft_batch_set_ave_row(u.h, Cn, 2) == EINVAL and not u.row_form()
