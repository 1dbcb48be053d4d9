"""Every decimator plan of the NCO + decimator cascade kernel (K2), in its compiled and its run-time-plan form, against
the fp64 reference of tests/dc_ref.py under the tap-resolving tolerance tol = K * rms(reference) (DESIGN.md, K2 parity
rule; K and the condition that gives it meaning are proven on the CPU in test_downconvert_ref_host.py), plus impulse
cases that pin every tap of every stage kind sample by sample, and stream cuts, segments, NCO edges and a late stream
against the same reference.  Needs only indep_ref, dc_ref, _build and the library.

Every comparison prints its figure before it asserts (pytest -s shows them)."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import dc_ref as D
from cutesdr_amd import _build

pytestmark = pytest.mark.gpu

PLANS = _build.all_dc_plans()
NINE = (3, 3, 11, 11, 11, 11, 15, 23, 47)        # nine stages, CICs and short and long half bands
assert NINE in PLANS
FM = (11, 11, 15, 19, 31)                       # 2 MS/s, 15 kHz
_id = lambda p: "-".join(map(str, p)) or "mixer"


def _pair(plan):
    return PLANS[plan] if plan else (2e6, 1e9)           # no stage fits a 1 GHz bandwidth: the pure mixer


def _lib():
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__downconv_force_dynamic.restype = C.c_int
    L.csdr__downconv_force_dynamic.argtypes = [C.c_int]
    L.csdr__downconvert_batch_set_wgs.restype = C.c_int
    L.csdr__downconvert_batch_set_wgs.argtypes = [C.c_void_p, C.c_long]
    return L


@contextlib.contextmanager
def kernel_form(dyn):
    """dyn = 1: every launch takes the run-time-plan kernel; 0: the compiled plan where the library has one"""
    L = _lib()
    L.csdr__downconv_force_dynamic(dyn)
    try:
        yield
    finally:
        L.csdr__downconv_force_dynamic(0)


def run_host_form(plan, freq, x, calls, retunes=None, pair=None):
    """x through a fresh CDownConvert in the given calls; retunes = {call index: frequency set in front of that call}"""
    import cutesdr_amd as ca
    rate, bw = pair or _pair(plan)
    dc = ca.CDownConvert()
    try:
        dc.SetDataRate(rate, bw)
        assert tuple(dc.stages()) == tuple(plan), (rate, bw)
        dc.SetFrequency(freq)
        out, pos = [], 0
        for i, n in enumerate(calls):
            if retunes and i in retunes:
                dc.SetFrequency(retunes[i])
            y = dc.ProcessData(x[pos:pos + n]); pos += n
            assert len(y) == n >> len(plan)                      # output counts exact, call by call
            out.append(y)
        assert pos == len(x)
        return np.concatenate(out)
    finally:
        dc.close()


def assert_parity(got, ref, what, skip=1):
    """every output behind the first `skip` within K rms(reference) of the reference"""
    assert len(got) == len(ref)
    tol = D.tolerance(ref)
    err = float(np.abs(got - ref)[skip:].max())
    print("DCPAR %s: max|err| %.4g = %.3f tol (%.3g of the rms; tol %.4g)" % (what, err, err / tol, err / D.rms(ref), tol))
    assert err <= tol, what


# ------------------------------------------------------------------------------------------------ B: every plan
def _parity_case(plan, dyn):
    rate, _ = _pair(plan)
    x, calls, f = D.parity_input(plan), D.parity_calls(plan), D.parity_freq(rate)
    assert calls[0] % 512 == 0 and calls[2] % 512 == 0 and calls[1] == 2048 + 3 * (1 << len(plan))
    with kernel_form(dyn):
        got = run_host_form(plan, f, x, calls)
    assert len(got) == sum(calls) >> len(plan)
    assert_parity(got, D.dc_reference(plan, f, rate, x), "%s %s" % ("run-time" if dyn else "compiled", _id(plan)))


@pytest.mark.parametrize("plan", sorted(PLANS, key=lambda p: (len(p), p)), ids=_id)
def test_runtime_plan_kernel_matches_fp64(plan):
    """all 164 stage sequences SetDataRate can produce, through the run-time-plan kernel"""
    _parity_case(plan, 1)


@pytest.mark.parametrize("plan", _build.DC_PLANS, ids=_id)
def test_compiled_plan_kernel_matches_fp64(plan):
    """every plan the library was compiled for, through its own kernel"""
    assert _lib().csdr__downconv_force_dynamic(-1) == len(_build.DC_PLANS)
    _parity_case(plan, 0)


def test_case_counts():
    assert len(PLANS) == 164 and len(_build.DC_PLANS) >= 40 and set(_build.DC_PLANS) <= set(PLANS)


# ------------------------------------------------------------------------------------------------ B: impulses
IMPULSE_REL = 8 * 2.0 ** -24        # a_inf, the mix, the fp32 tap and the product round once each (4 x 2^-24 at most);
                                    # the sum adds zeros.  Measured worst on the MI355X: HISTORY.md.


@pytest.mark.parametrize("form", ["whole", "ragged"])
@pytest.mark.parametrize("dyn", [0, 1], ids=["library", "runtime"])
@pytest.mark.parametrize("kind", D.KINDS)
def test_impulse_response_is_the_tap_vector(kind, dyn, form):
    """One stage, NCO at 0 Hz, full-scale impulses at an even and an odd input index behind the envelope: the output is
    the tap vector times the settled amplitude, tap by tap.  `whole`: the impulses lie in a complete tile (a compiled
    plan runs dc_stage_full there), `ragged`: in a short last tile (dc_stage in both kernels).  dyn = 0 takes whatever
    the library holds for (kind,): its compiled kernel if there is one."""
    n = 2048 if form == "whole" else 1936                    # 3 tiles + 400 samples: the impulses sit at 1560 and 1701
    assert all(1536 <= m and m + D.hist_of(kind) < n for m in D.IMPULSE_AT)
    want = D.impulse_expected(kind, n)
    with kernel_form(dyn):
        got = run_host_form((kind,), 0.0, D.impulse_input(n), [n])
    nz = want != 0
    assert nz.sum() == (4 if kind == 3 else 2 * D.n_pairs(kind) + 1)
    rel = max(np.abs(got.real[nz] / want.real[nz] - 1).max(), np.abs(got.imag[nz] / want.imag[nz] - 1).max())
    print("DCIMP kind %d %s %s: worst relative error %.3g = %.2f x 2^-24; compiled %s" %
          (kind, "runtime" if dyn else "library", form, rel, rel * 2.0 ** 24, (kind,) in _build.DC_PLANS))
    bad = np.flatnonzero(nz & ((np.abs(got.real - want.real) > IMPULSE_REL * np.abs(want.real)) |
                               (np.abs(got.imag - want.imag) > IMPULSE_REL * np.abs(want.imag))))
    assert len(bad) == 0, "outputs %s (taps reached from the impulses at %s)" % (bad.tolist(), D.IMPULSE_AT)
    assert np.all(got[~nz] == 0), "outputs %s must be exactly zero" % np.flatnonzero((got != 0) & ~nz).tolist()


# ------------------------------------------------------------------------------------------------ C: cuts
def cut_lengths(plan):
    """the call lengths of the issue's set that the plan can take: multiples of 2^ns, and of the kernel's own sample
    pair for the pure mixer and the single stage (n must be even)"""
    u, W = max(2, 1 << len(plan)), D.warmup_len(plan)
    cand = [u, 3 * u, W - u, W, W + u, 512 - u, 512 + u, 5 * 512 + u, 19968]
    return sorted({n for n in cand if n > 0 and n % u == 0})


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("plan", [(), (3,), (51,), FM, NINE], ids=_id)
def test_any_cutting_of_a_stream_matches_fp64(plan, seed):
    """48 calls from age 0, the first eight short (so the end of the start-up envelope at sample 512 and the n_in < W
    tail copy fall into short tiles several calls in a row), against ONE run of the reference over the whole stream"""
    rate, _ = _pair(plan)
    lens = cut_lengths(plan)
    short = [n for n in lens if n <= 1024] or lens[:2]
    rng = np.random.Generator(np.random.PCG64(1000 * seed + len(plan)))
    calls = [int(rng.choice(short)) for _ in range(8)] + [int(rng.choice(lens)) for _ in range(40)]
    assert len(calls) >= 40 and all(n % (1 << len(plan)) == 0 and n % 2 == 0 for n in calls)
    x = D.white(77 + seed, sum(calls))
    f = 0.0617 * rate
    got = run_host_form(plan, f, x, calls)
    assert_parity(got, D.dc_reference(plan, f, rate, x), "cuts %s seed %d (%d calls, %d samples)" % (_id(plan), seed, len(calls), len(x)),
                  skip=0 if not plan else 1)


# ------------------------------------------------------------------------------------------------ C: segments
def segment_geometry(n, W, nchan=1, wgs=1 << 20):
    """the host's segment rule (capi_downconv.hip), recomputed: (segments, segment length, length of the last one)"""
    min_seg = max(512, W)
    nseg = max(1, min(wgs // nchan, n // min_seg))
    seg_len = ((n + nseg - 1) // nseg + 511) // 512 * 512
    nseg = (n + seg_len - 1) // seg_len
    return nseg, seg_len, n - (nseg - 1) * seg_len


def _find_n(W, unit, want, start=8192):
    """smallest call length from `start` (multiple of `unit`) whose last segment satisfies want(nseg, last)"""
    for n in range(start, start + 200000, unit):
        nseg, _, last = segment_geometry(n, W)
        if nseg >= 3 and want(last):
            return n
    raise AssertionError("no such call length")


@pytest.mark.parametrize("plans", [[FM], [FM, (11, 11, 11, 15, 23, 51), (3, 3, 11, 11, 11, 11, 15)]], ids=["one", "three"])
def test_maximum_segments_with_ragged_and_short_last_segments(plans):
    """The most segments the host rule allows (one per warm-up length), call lengths that leave, channel by channel,
    the last segment (a) a single ragged tile and (b) ragged, longer than a tile and shorter than W; then a whole-tile
    call.  Every channel of every call against the reference."""
    import cutesdr_amd as ca
    rate = 2e6
    bws = {FM: 15000.0, (11, 11, 11, 15, 23, 51): 10000.0, (3, 3, 11, 11, 11, 11, 15): 1000.0}
    unit = 1 << max(len(p) for p in plans)
    calls = []
    for p in plans:
        W = D.warmup_len(p)
        na = _find_n(W, unit, lambda last: last < 512)
        nb = _find_n(W, unit, lambda last: 512 < last < W and last % 512)
        assert segment_geometry(na, W)[2] < 512 <= W and 512 < segment_geometry(nb, W)[2] < W
        calls += [na, nb]
    calls.append(16384)
    L = _lib()
    b = ca.DownConvertBatch(len(plans))
    try:
        freqs = [(-0.11 + 0.09 * c) * rate for c in range(len(plans))]
        for c, p in enumerate(plans):
            assert b.set_data_rate(rate, bws[p], channel=c) == rate / (1 << len(p))
            assert tuple(b.stages(c)) == p
            b.set_frequency(freqs[c], channel=c)
        assert L.csdr__downconvert_batch_set_wgs(b.h, 1 << 20) == 0
        x = np.stack([D.white(300 + c, sum(calls)) for c in range(len(plans))])
        outs, pos = [[] for _ in plans], 0
        for n in calls:
            got = b.process(x[:, pos:pos + n]); pos += n
            for c, p in enumerate(plans):
                assert len(got[c]) == n >> len(p)
                outs[c].append(got[c])
        for c, p in enumerate(plans):
            geo = [segment_geometry(n, D.warmup_len(p)) for n in calls]
            assert_parity(np.concatenate(outs[c]), D.dc_reference(p, freqs[c], rate, x[c]),
                          "segments ch %d %s (nseg, seg_len, last) %s" % (c, _id(p), geo))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ C: blanker in front
class _DcBlank(C.Structure):
    """DcBlank of downconv_kernels.h: what csdr__noiseproc_batch_mask leaves for the down-converter"""
    _fields_ = [("mask", C.c_void_p), ("mask_stride", C.c_long), ("state", C.c_void_p), ("hist", C.c_void_p)]


@pytest.mark.parametrize("dyn", [0, 1], ids=["compiled", "runtime"])
@pytest.mark.parametrize("fs,width", [(2e6, 20.0), (2000200.0, 21.0)], ids=["odd-delay", "even-delay"])
@pytest.mark.parametrize("src", ["rows", 1028, 1444])
def test_blanked_down_converter_matches_fp64(oracle, src, fs, width, dyn):
    """The down-converter that applies the noise blanker's mask in its own loads (sample i = mask bit ? 0 :
    raw[i - delay_n - 1]), on its own: one FM channel, float rows and both datagram formats, D1 = delay_n + 1 = 21 and
    22 (behind an odd delay the datagram form fetches aligned pairs one sample early, rotates them across the wave and
    decodes one trailing sample), three calls of 64, 4 and 130 datagrams (or 256-sample rows) cut into as many segments
    as the host rule allows -- the first reaches into the blanker's history, the second is no longer than the warm-up.
    Expected: the fp64 cascade over the oracle blanker's output on the oracle's unpacked samples (mask + delay give
    that stream word for word: test_frontend_gpu.py::test_blank_mask_is_bit_exact).  Input: white I/Q of amplitude
    1500 with +25000 impulses at rate 2e-4, as there; dc_ref.dc_reference_fp32 of the six blanked streams (6 % of the
    samples zeroed) stays within 0.16 .. 0.22 tol of the fp64 reference, as it does for white input."""
    import cutesdr_amd as ca
    from test_frontend_gpu import _pack16, _pack24
    L = _lib()
    L.csdr__noiseproc_batch_mask.restype = C.c_int
    L.csdr__noiseproc_batch_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_longlong, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
    L.csdr__downconvert_batch_process_rows.restype = C.c_int
    L.csdr__downconvert_batch_process_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p,
                                                       C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_DcBlank)]
    per = 240 if src == 1444 else 256
    counts = [64, 4, 130]
    tot = sum(counts) * per
    assert all(npk * per % 32 == 0 for npk in counts) and counts[1] * per <= D.warmup_len(FM) < counts[0] * per
    rng = np.random.default_rng(17)
    x = 1500.0 * (rng.standard_normal(tot) + 1j * rng.standard_normal(tot))
    x[rng.random(tot) < 2e-4] += 25000.0
    if src == "rows":
        xs = x.astype(np.complex64)
    else:
        raw = (_pack24 if src == 1444 else _pack16)(x)
        xs = oracle.unpack_packets(raw, src).astype(np.complex64)
    delay1 = int(width * 1e-6 * fs) // 2 + 1
    assert delay1 == (21 if width == 20.0 else 22)
    freq = D.parity_freq(fs)
    nb, b = ca.NoiseProcBatch(1), ca.DownConvertBatch(1)
    q = oracle.CNoiseProc(); q.SetupBlanker(True, 25.0, width, fs)
    bufs, got, blanked = [], [], []
    try:
        nb.setup(True, 25.0, width, fs)
        assert b.set_data_rate(fs, 15000.0) == fs / 32 and tuple(b.stages(0)) == FM
        b.set_frequency(freq)
        assert L.csdr__downconvert_batch_set_wgs(b.h, 1 << 20) == 0
        k0 = 0
        with kernel_form(dyn):
            for npk in counts:
                n, a0 = npk * per, k0 * per
                words = (n + 31) // 32 + 64
                part = np.ascontiguousarray(xs[a0:a0 + n] if src == "rows" else raw[k0:k0 + npk])
                dp, dm, do = ca.DeviceBuffer(part.nbytes), ca.DeviceBuffer(words * 4), ca.DeviceBuffer(8 * (n >> 5))
                bufs += [dp, dm, do]
                dp.upload(part)
                rows, pk, npk_arg, fmt = (C.c_void_p(dp.ptr), None, 0, 0) if src == "rows" else (None, C.c_void_p(dp.ptr), npk, src)
                st, hi = C.c_void_p(), C.c_void_p()
                assert L.csdr__noiseproc_batch_mask(nb.h, rows, n, pk, npk_arg, fmt, n, C.c_void_p(dm.ptr), words,
                                                    C.byref(st), C.byref(hi), None) == 0
                blank = _DcBlank(dm.ptr, words, st.value, hi.value)
                assert L.csdr__downconvert_batch_process_rows(b.h, rows, n, None, n, C.c_void_p(do.ptr), n >> 5, None, pk, fmt,
                                                              C.byref(blank)) == 0
                ca.sync()
                got.append(do.download(np.complex64, n >> 5).astype(np.complex128))
                blanked.append(q.ProcessBlanker(xs[a0:a0 + n].astype(np.complex128)))
                k0 += npk
    finally:
        b.close(); nb.close()
        for d in bufs:
            d.free()
    blanked = np.concatenate(blanked)
    zeros = int((blanked == 0).sum()) - delay1                # (the delay line starts with delay1 zeros of its own)
    print("DCBLK %s D1 %d: %d of %d samples blanked" % (src, delay1, zeros, tot))
    assert 0 < zeros < tot                                    # the case blanks, and not everything
    assert_parity(np.concatenate(got), D.dc_reference(FM, freq, fs, blanked),
                  "blanked %s D1 %d %s" % (src, delay1, "run-time" if dyn else "compiled"))


# ------------------------------------------------------------------------------------------------ C: NCO edges
NCO_RATE = 2e6
NCO_FREQS = [("zero", 0.0), ("+rate/2", NCO_RATE / 2), ("-rate/2", -NCO_RATE / 2), ("rate/2 - 1 Hz", NCO_RATE / 2 - 1.0),
             ("1.3 rate", 1.3 * NCO_RATE), ("smallest increment", NCO_RATE * 2.0 ** -63)]


@pytest.mark.parametrize("plan", [(), FM], ids=_id)
@pytest.mark.parametrize("i", range(len(NCO_FREQS)), ids=[n for n, _ in NCO_FREQS])
def test_nco_edge_frequencies_and_retune(oracle, plan, i):
    """two calls with a retune between them (to the next frequency of the list): the phasor stays, the increment changes"""
    import cutesdr_amd as ca
    (name, f1), (_, f2) = NCO_FREQS[i], NCO_FREQS[(i + 1) % len(NCO_FREQS)]
    calls = [8192 + 96, 8192]
    x = D.white(500 + i, sum(calls))
    got = run_host_form(plan, f1, x, calls, retunes={1: f2}, pair=(NCO_RATE, 15000.0 if plan else 1e9))
    r = D.DcRef(plan, f1, NCO_RATE)
    a = r.run(x[:calls[0]]); r.set_frequency(f2); ref = np.concatenate([a, r.run(x[calls[0]:])])
    assert_parity(got, ref, "nco %s then retune, %s" % (name, _id(plan)), skip=0 if not plan else 1)
    # nco_freq() is the request as given (the wrap is the host's business), as in the oracle
    dc, oc = ca.CDownConvert(), oracle.CDownConvert()
    for f in (f1, f2):
        dc.SetFrequency(f); oc.SetFrequency(f)
        assert dc.nco_freq() == oc.nco_freq() == f
    dc.close()
    if name == "1.3 rate":          # a request outside +-rate/2 IS the wrapped one
        r = D.DcRef(plan, 0.3 * NCO_RATE, NCO_RATE)
        a = r.run(x[:calls[0]]); r.set_frequency(f2); ref = np.concatenate([a, r.run(x[calls[0]:])])
        assert_parity(got, ref, "nco 1.3 rate against 0.3 rate, %s" % _id(plan), skip=0 if not plan else 1)
    if name == "smallest increment":
        assert 0.5 <= f1 / NCO_RATE * 2.0 ** 63 < 1.5           # the host's llround(turns 2^63) gives 1: increment 2 of 2^64


# ------------------------------------------------------------------------------------------------ C: late stream
LATE_RATE = 2.0 ** 21                                           # a power of two: freq / rate below is exact in fp64
LATE_TURNS = 0.3125 + 2.0 ** -33 + 2.0 ** -45                   # 2^32 samples of it are NOT a whole number of turns


@pytest.mark.parametrize("log2_age", [31, 32])
@pytest.mark.parametrize("decimating", [False, True], ids=["mixer", "decimating"])
def test_late_stream_straddling_a_power_of_two(decimating, log2_age):
    """One channel advanced to 8192 samples below 2^31 / 2^32 input samples by process calls on one resident device
    buffer, then two compared calls, the first of which straddles the power of two (a 32-bit age, phase or sample index
    would turn the phasor by half a turn there), against dc_reference(first_sample = age)."""
    import cutesdr_amd as ca
    from cutesdr_amd.host import DeviceBuffer, sync
    bw = 15000.0 if decimating else 1e9
    plan = _build.dc_plan(LATE_RATE, bw)
    assert bool(plan) == decimating
    ns, W = len(plan), D.warmup_len(plan)
    N, back = 1 << 22, 8192
    target = (1 << log2_age) - back
    x = D.white(900 + log2_age, N)
    freq = LATE_RATE * LATE_TURNS
    assert freq / LATE_RATE == LATE_TURNS
    din, dout = DeviceBuffer(8 * N), DeviceBuffer(8 * N)
    b = ca.DownConvertBatch(1)
    try:
        din.upload(x)
        b.set_data_rate(LATE_RATE, bw)
        assert tuple(b.stages(0)) == plan
        b.set_frequency(freq)
        t0 = time.time()
        full, rem = divmod(target, N)
        for _ in range(full):
            b.process_ptr(din.ptr, N, N, dout.ptr, N)
        assert rem > 0 and rem % 512 == 0
        b.process_ptr(din.ptr, N, rem, dout.ptr, N)
        sync()
        wall = time.time() - t0
        P = max(4096, W)
        assert W <= P <= rem
        o1, n1, n2 = 65536, back + 4096, 8192                  # the first compared call runs from 2^k - 8192 to 2^k + 4096
        got = []
        for o, n in ((o1, n1), (o1 + n1, n2)):
            b.process_ptr(din.ptr + 8 * o, N, n, dout.ptr, N)
            sync()
            got.append(dout.download(np.complex64, n >> ns).astype(np.complex128))
        stream = np.concatenate([x[rem - P:rem], x[o1:o1 + n1 + n2]])
        ref = D.dc_reference(plan, freq, LATE_RATE, stream, first_sample=target - P)[P >> ns:]
        print("DCLATE advance to 2^%d - %d (%d calls): %.3f s wall" % (log2_age, back, full + 1, wall))
        assert_parity(np.concatenate(got), ref, "late 2^%d %s" % (log2_age, _id(plan)), skip=0)
    finally:
        b.close(); din.free(); dout.free()


# ------------------------------------------------------------------------------------------------ C: refusals
def test_arguments_that_would_break_the_pair_loads_are_refused_before_any_launch():
    """The kernel reads sample PAIRS with 16-byte loads and walks 2^ns-sample units: odd n, n not a multiple of 2^ns,
    an input stride below n, an odd stride and an input pointer 8 bytes off a 16-byte boundary must each return
    CSDR_EINVAL -- by the host code, with nothing launched: the output buffer keeps its sentinel and the stream has not
    advanced (the next valid call gives the stream's FIRST outputs)."""
    import cutesdr_amd as ca
    from cutesdr_amd import _capi
    from cutesdr_amd.host import DeviceBuffer, sync
    L = _lib()
    n = 4096
    x = D.white(4242, 2 * n)
    sentinel = np.full(2 * n, -7.0 - 7.0j, dtype=np.complex64)
    din, dout = DeviceBuffer(8 * 2 * n), DeviceBuffer(8 * 2 * n)
    b = ca.DownConvertBatch(1)
    try:
        din.upload(x); dout.upload(sentinel)
        b.set_data_rate(2e6, 15000.0)
        assert tuple(b.stages(0)) == FM
        b.set_frequency(123456.0)
        call = lambda ptr, stride, cnt: L.csdr_downconvert_batch_process(b.h, C.c_void_p(ptr), stride, cnt, C.c_void_p(dout.ptr), 2 * n, None)
        bad = {"odd n": (din.ptr, 2 * n, n + 1), "n not a multiple of 2^ns": (din.ptr, 2 * n, n + 16),
               "zero n": (din.ptr, 2 * n, 0), "stride below n": (din.ptr, n - 2, n), "odd stride": (din.ptr, n + 1, n),
               "pointer 8 bytes off": (din.ptr + 8, 2 * n, n)}
        for what, args in bad.items():
            assert call(*args) == _capi.CSDR_EINVAL, what
        sync()
        assert np.array_equal(dout.download(np.complex64, 2 * n), sentinel)
        assert call(din.ptr, 2 * n, n) == _capi.CSDR_OK
        sync()
        got = dout.download(np.complex64, n >> 5).astype(np.complex128)
        assert_parity(got, D.dc_reference(FM, 123456.0, 2e6, x[:n]), "first valid call after the refusals")
    finally:
        b.close(); din.free(); dout.free()
