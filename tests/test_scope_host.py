"""CPU checks of the batch test-bench scope: the restatement of the reference's time view in scope_ref.py has the
window property the kernel is built on, and the library's host-side pieces (cutesdr_amd/csrc/scope_host.hpp through
the csdr__host_scope_* hooks, the functions the kernel evaluates) equal the restatement's loops.  All comparisons are
on integers and exact."""
import ctypes as C

import numpy as np
import pytest

import scope_ref as R

SYMBOLS = ["csdr_scope_batch_" + s for s in (
    "create", "destroy", "set_screen", "set_horz_span", "set_display_rate", "set_trigger_mode", "set_trig_level",
    "set_vert_range", "reset", "put_real", "put_cpx", "time_plot_done", "get_emits", "get_screen", "get_state",
    "get_screens_all")]


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_scope_emissions.restype = C.c_longlong
    lib.csdr__host_scope_emissions.argtypes = [C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_int, C.c_longlong,
                                               C.c_longlong, C.c_void_p, C.c_void_p]
    lib.csdr__host_scope_settings.restype = None
    lib.csdr__host_scope_settings.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.csdr__host_scope_free_run.restype = None
    lib.csdr__host_scope_free_run.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_void_p]
    lib.csdr__host_scope_sat_int.restype = C.c_int
    lib.csdr__host_scope_sat_int.argtypes = [C.c_double]
    return lib


def hook_emissions(L, inpos, pos, pix, sr, w, n):
    cap = 8 * w + 8 * n // max(1, int(sr * pix)) + 64
    out, end = np.zeros(cap, dtype=np.int64), np.zeros(3, dtype=np.int64)
    e = L.csdr__host_scope_emissions(inpos, pos, pix, sr, w, n, cap, out.ctypes.data, end.ctypes.data)
    assert e == end[0] and e <= cap, (e, cap)
    return out[:e].tolist(), int(end[1]), int(end[2])


def sweep_len(w, span, sr):
    return R.emission_sequence(0, 0, .001 * (float(span) / float(w)), sr, w, int(span * sr / 1000.0) + 8)[0][w - 1] + 1


def test_symbols_exported_and_bound(L):
    from cutesdr_amd import _capi
    names = _capi.declared_symbols()
    for s in SYMBOLS:
        assert s in names, s
        assert getattr(L, s).argtypes is not None, s
    import cutesdr_amd
    for slot in ("OnHorzSpan", "OnDisplayRate", "OnTriggerMode", "OnTrigLevel", "OnVertRange", "Reset", "DisplayData",
                 "DrawTimePlot", "time_plot_done", "resizeEvent", "get_emits", "get_screen", "get_screens_all"):
        assert hasattr(cutesdr_amd.ScopeBatch, slot), slot


@pytest.mark.parametrize("w,span,sr", R.CONFIGS)
def test_restatement_window_property(w, span, sr):
    """in the triggered modes a trigger found at emission q_t displays at q_d = q_t + Post, Post = (7*w)/10, and the
    screen is emissions q_d-w .. q_d-1 in order, zeros before the reset: the trigger pixel sits at screen index w - Post"""
    post = (7 * w) // 10
    n = max(20000, 5 * sweep_len(w, span, sr))
    rng = np.random.default_rng(5)
    for mode in (R.TRIG_PNORM, R.TRIG_NNORM):
        r = R.RefScope()
        r.resizeEvent(w, 100); r.OnHorzSpan(span); r.OnTriggerMode(mode)
        x = R.signal(0, n, cpx=True)
        r.DisplayData([], [], sr)                        # the first call's rate differs from 1: dropped, :587-592
        pos, shown = 0, 0
        while pos < n:
            k = min(int(rng.choice([1, 7, 256, 513, 1000])), n - pos)
            before = len(r.display_at)
            r.DisplayData(x.real[pos:pos + k], x.imag[pos:pos + k], sr)
            pos += k
            if len(r.display_at) > before:
                assert len(r.display_at) == before + 1 == len(r.trigger_at)
                qt, qd = r.trigger_at[-1], r.display_at[-1]
                assert qd == qt + post
                window = [(0, 0)] * max(0, w - qd) + r.log[max(0, qd - w):qd]
                re, im = r.screen()
                assert re == [v[0] for v in window] and im == [v[1] for v in window]
                lvl = r.m_TrigLevel
                cur, prv = re[w - post], (re[w - post - 1] if w - post - 1 >= 0 else None)
                if qd >= w and prv is not None:
                    assert (cur >= lvl > prv) if mode == R.TRIG_PNORM else (cur <= lvl < prv)
                shown += 1
                r.time_plot_done()
        assert shown >= 3, shown


def test_restatement_free_run_screen_is_rotated():
    """TRIG_OFF: decided at screen position 0, the screen is the sweep before it read from ring slot Post"""
    w, span, sr = 64, 10, 48000.0
    post = (7 * w) // 10
    r = R.RefScope()
    r.resizeEvent(w, 100); r.OnHorzSpan(span)
    x = R.signal(0, 20000)
    r.DisplayData([], None, sr)
    r.DisplayData(x, None, sr)
    assert r.emits >= 2
    qd = r.display_at[-1]
    assert qd % w == 0
    sweep = [v[0] for v in r.log[qd - w:qd]]
    assert r.screen()[0] == sweep[post:] + sweep[:post]


@pytest.mark.parametrize("w,span,sr", R.CONFIGS)
def test_emission_hook_equals_restatement(L, w, span, sr):
    """the library's emission sequence, from the start of a sweep, from a mid-sweep state, and with the span changed
    in mid-sweep (shorter and longer), over calls that end inside the entered sweep and calls that span several"""
    pix = .001 * (float(span) / float(w))
    ln = sweep_len(w, span, sr)
    for n in (0, 1, ln - 1, ln, ln + 1, int(2.5 * ln) + 3):
        assert hook_emissions(L, 0, 0, pix, sr, w, n) == R.emission_sequence(0, 0, pix, sr, w, n)
    for frac in (0.11, 0.5, 0.93):
        _, pos, inpos = R.emission_sequence(0, 0, pix, sr, w, max(1, int(frac * ln)))
        for n in (1, 7, max(1, ln // 3), ln, int(2.2 * ln) + 1):
            assert hook_emissions(L, inpos, pos, pix, sr, w, n) == R.emission_sequence(inpos, pos, pix, sr, w, n), (frac, n)
            for span2 in (max(1, span // 3), span * 2 + 1):
                pix2 = .001 * (float(span2) / float(w))
                n2 = min(n, 3 * sweep_len(w, span2, sr))
                assert hook_emissions(L, inpos, pos, pix2, sr, w, n2) == R.emission_sequence(inpos, pos, pix2, sr, w, n2), (frac, n, span2)


def test_settings_free_run_and_conversion_hooks(L):
    for w, span, sr in R.CONFIGS:
        for rate in (1, 7, 10, 15):
            r = R.RefScope()
            r.resizeEvent(w, 100); r.DisplayData([], None, sr); r.OnHorzSpan(span); r.OnDisplayRate(rate)
            pix, skip = C.c_double(), C.c_int()
            L.csdr__host_scope_settings(span, rate, sr, w, C.byref(pix), C.byref(skip))
            assert pix.value == r.m_TimeScrnPixel and skip.value == r.m_DisplaySkipValue
    out = np.zeros(3, dtype=np.int64)
    for skip in (0, 1, 2, 3, 4, 14, 100):
        for cnt in (-2, -1, 0, 2, 3, 5, 99, 120):
            for m in (0, 1, 2, 3, 4, 5, 13, 14, 15, 29, 250):
                c, shown, last = cnt, 0, 0
                for k in range(1, m + 1):                # :826-831
                    c += 1
                    if c >= skip and c > 2:
                        c, shown, last = 0, shown + 1, k
                L.csdr__host_scope_free_run(cnt, skip, m, out.ctypes.data)
                assert out.tolist() == [shown, last, c], (skip, cnt, m)
    for x in (0.0, -0.0, 0.999, -0.999, 1.5, -1.5, 2999.7, -32768.9, 2147483520.0, 2147483647.0, 2147483648.0, 3e9, -2147483648.0,
              -2147483904.0, -1e30, 1e30, float("inf"), float("-inf"), float("nan")):
        assert L.csdr__host_scope_sat_int(x) == R.c_int(x), x


def test_create_needs_a_gpu(L):
    """no CPU fallback: NULL and the reason without a HIP device, an object with one"""
    s = L.csdr_scope_batch_create(0, 4)
    if L.csdr_device_count() > 0:
        assert s
        L.csdr_scope_batch_destroy(s)
    else:
        assert not s and b"no HIP device" in L.csdr_last_error()


# ------------------------------------------------------------------ the whole receiver on the CPU
class HookBatch:
    """16 receivers of the library's host-side scope (csdr__host_scope_*: the host's settings as capi_scope.hip keeps
    them and the put with the functions the kernel calls) behind the batch's interface"""
    WHAT = {"OnHorzSpan": 1, "OnDisplayRate": 2, "OnTriggerMode": 3, "OnTrigLevel": 4, "OnVertRange": 5, "Reset": 6,
            "time_plot_done": 7}

    def __init__(self, L, channels=16):
        L.csdr__host_scope_create.restype = C.c_void_p
        L.csdr__host_scope_destroy.argtypes = [C.c_void_p]
        L.csdr__host_scope_slot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.csdr__host_scope_put.restype = C.c_longlong
        L.csdr__host_scope_put.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
        L.csdr__host_scope_get.argtypes = [C.c_void_p] * 4
        self.L, self.w = L, 100
        self.h = [L.csdr__host_scope_create() for _ in range(channels)]
        self.total = [0] * channels

    def __del__(self):
        for h in self.h:
            self.L.csdr__host_scope_destroy(h)

    def resizeEvent(self, w, h):
        self.w = w
        for x in self.h:
            self.L.csdr__host_scope_slot(x, 0, w, h)

    def __getattr__(self, name):
        k = self.WHAT[name]

        def slot(v=0, channel=-1):
            if k in (6, 7):                              # Reset(channel), time_plot_done(channel)
                v, channel = 0, v
            for x in (self.h if channel < 0 else [self.h[channel]]):
                self.L.csdr__host_scope_slot(x, k, v, 0)
        return slot

    def put(self, rows, pos, n, rates):
        for c, x in enumerate(self.h):                   # n[c] = 0: only what the setters left pending
            a = rows[c, pos:pos + n[c]]
            if rows.dtype.kind == "c":
                re, im = np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
                self.total[c] = self.L.csdr__host_scope_put(x, re.ctypes.data, im.ctypes.data, n[c], rates[c])
            else:
                re = np.ascontiguousarray(a)
                self.total[c] = self.L.csdr__host_scope_put(x, re.ctypes.data, None, n[c], rates[c])

    def totals(self):
        return list(self.total)

    def _get(self, c):
        st, re, im = np.zeros(7, dtype=np.int64), np.zeros(self.w, dtype=np.int32), np.zeros(self.w, dtype=np.int32)
        self.L.csdr__host_scope_get(self.h[c], st.ctypes.data, re.ctypes.data, im.ctypes.data)
        return st.tolist(), (re.tolist(), im.tolist())

    def screen(self, c):
        return self._get(c)[1]

    def state(self, c):
        return self._get(c)[0]


@pytest.mark.parametrize("cpx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("k", range(5))
def test_host_scope_parity(L, k, cpx):
    """the functions the kernel evaluates, run on the CPU over the scenario of the GPU test: emits, screens and states
    equal the restatement's after every call"""
    R.check_counts(k, R.check(HookBatch(L), k, cpx))


@pytest.mark.parametrize("k", [0, 3])
def test_host_scope_slots_in_mid_stream(L, k):
    R.check(HookBatch(L), k, False, "mid", R.mid_stream_events(k))


@pytest.mark.parametrize("k", [3, 4])
def test_host_scope_cut_does_not_matter(L, k):
    """TRIG_OFF (k = 3) and PSINGLE (k = 4): one call of 20000 samples gives the screen and emit count of the uneven calls"""
    rows, calls, states, totals, screens = R.trace(k, False)
    one = HookBatch(L)
    R.configure(one, k)
    first = R.cuts()[0]                                  # the first call is dropped (its rate differs from 1), as in the cuts
    R.run(one, rows, k, [first, R.N_SAMPLES - first])
    assert one.totals()[k] == totals[k] and one.screen(k) == screens[k]
