"""ctypes binding of the REFERENCE's own dsp/ code, compiled unmodified -- TEST INFRASTRUCTURE ONLY.

oracle/oracle.py binds an fp64 restatement of the reference that this project wrote; this module binds the reference's
classes themselves, through oracle/ref/ref_shim.cpp, with the same class names and method signatures, so a test can
take either module as its checker.  build() compiles oracle/_ref/libcutesdr_ref.so from the reference tree (default
/root/reference, or $CSDR_REFERENCE_DIR) with the stand-in Qt headers of oracle/ref/qt; neither the tree nor anything
compiled from it is committed.  Where the tree is absent (the GPU machine) the library that travelled with the working
tree is used as it is.

Differences from the oracle's binding, all of them the reference's own limits:
  * inputs are always private copies: CDownConvert::ProcessData, CFastFIR::ProcessData and CFft::PutInDisplayFFT work
    in place, and no caller's array may change under a checker;
  * a call longer than one of the reference's fixed buffers raises ValueError and is never forwarded (half-band scratch
    of 32768 samples, MAX_INBUFSIZE, MAX_MAGBUFSIZE, MAX_SQBUF_SIZE, the blanker's 4096-entry test-bench buffer and
    32768-entry average, the resampler's Init size, the display transform's size);
  * CFastFIR and CDemodulator exist at 2048 points only (CONV_FFT_SIZE is a constant of dsp/fastfir.cpp);
  * objects are constructed into zeroed storage (see ref_shim.cpp for the members this decides);
  * no sound sink, packet unpacking, spur calibration or plotter: those live outside dsp/ and need more of Qt;
  * the PROFILE_* tap points are recorded as calls (profile, length, rate, first value) on one global test bench:
    tap_calls() / clear_tap_calls().
Nothing under cutesdr_amd/ or include/ may name this module or its library (tests/test_capi_abi.py).
"""
import ctypes as C
import os
import subprocess
import tempfile
import numpy as np

from . import oracle as _o
from .oracle import DemodInfo, fm_defaults, DEMOD_AM, DEMOD_SAM, DEMOD_FM, DEMOD_USB, DEMOD_LSB, DEMOD_CWU, DEMOD_CWL  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_RECIPE = os.path.join(_HERE, "ref")
_OUT = os.path.join(_HERE, "_ref")
_SO = os.path.join(_OUT, "libcutesdr_ref.so")
_STUB = os.path.join(os.path.dirname(_HERE), "tests", "cpp", "stub", "gui", "testbench.h")
DSP_SOURCES = ["agc", "amdemod", "demodulator", "downconvert", "fastfir", "fft", "fir", "fmdemod", "fractresampler", "iir",
               "noiseproc", "samdemod", "smeter", "ssbdemod"]
# the oracle's floating-point contract (oracle/Makefile): no contraction into fused multiply-adds, no fast-math;
# every claim of bit equality between the two depends on it
FLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-std=gnu++11", "-fpermissive", "-w"]


def reference_dir():
    return os.environ.get("CSDR_REFERENCE_DIR", "/root/reference")


def tree_present():
    return os.path.isfile(os.path.join(reference_dir(), "dsp", "demodulator.cpp"))


def _recipe_files():
    files = [os.path.abspath(__file__), _STUB]
    for d, _, names in os.walk(_RECIPE):
        files += [os.path.join(d, n) for n in names]
    return files


def build(force=False):
    """Compile the reference into oracle/_ref/libcutesdr_ref.so when its tree is there and the library is missing or
    older than a recipe file; otherwise leave whatever is there.  Returns the library's path, or None without one."""
    if tree_present():
        stale = force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(f) for f in _recipe_files())
        if stale:
            _compile()
    return _SO if os.path.exists(_SO) else None


def _compile():
    ref = reference_dir()
    inc = ["-I" + _RECIPE, "-I" + os.path.join(_RECIPE, "qt"), "-I" + ref]
    os.makedirs(_OUT, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(os.path.join(ref, "dsp", n + ".cpp"), os.path.join(tmp, n + ".o"), []) for n in DSP_SOURCES]
        jobs.append((os.path.join(_RECIPE, "ref_stubs.cpp"), os.path.join(tmp, "ref_stubs.o"), []))
        jobs.append((os.path.join(_RECIPE, "ref_shim.cpp"), os.path.join(tmp, "ref_shim.o"), ["-fno-access-control"]))
        procs = [subprocess.Popen([cxx] + FLAGS + extra + inc + ["-c", src, "-o", obj]) for src, obj, extra in jobs]
        bad = [j[0] for j, p in zip(jobs, procs) if p.wait() != 0]
        if bad:
            raise RuntimeError("reference build failed: " + ", ".join(bad))
        part = _SO + ".part"
        subprocess.check_call([cxx, "-shared", "-o", part] + [j[1] for j in jobs] +
                              ["-Wl,-Bsymbolic", "-Wl,--version-script=" + os.path.join(_RECIPE, "ref_exports.map"), "-lm"])
        os.replace(part, _SO)


def available():
    return build() is not None


class _Renamed:
    """the reference library with its ref_* entry points under the orc_* names oracle.py's classes call"""

    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        if not name.startswith("orc_"):
            raise AttributeError(name)
        try:
            return getattr(self._cdll, "ref_" + name[4:])
        except AttributeError:
            raise AttributeError("the reference library has no counterpart of " + name) from None


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = build()
        if so is None:
            raise RuntimeError("no reference library: neither %s nor the reference tree at %s exists" % (_SO, reference_dir()))
        L = C.CDLL(so)
        _o._declare(L, prefix="ref_", optional=True)
        for name, res, args in (("ref_limit", C.c_int, [C.c_int]), ("ref_tap_calls", C.c_int, []), ("ref_tap_calls_clear", None, []),
                                ("ref_tap_call", None, [C.c_int] + [C.c_void_p] * 5), ("ref_demod_buf_pos", C.c_int, [C.c_void_p]),
                                ("ref_demod_stages", C.c_int, [C.c_void_p, C.c_void_p]), ("ref_demod_nco_freq", C.c_double, [C.c_void_p]),
                                ("ref_demod_input_rate", C.c_double, [C.c_void_p]), ("ref_demod_max_bw", C.c_double, [C.c_void_p]),
                                ("ref_dc_loop_const", C.c_double, [C.c_int])):
            fn = getattr(L, name); fn.restype = res; fn.argtypes = args
        _lib = _Renamed(L)
    return _lib


def limit(name):
    names = ["MAX_HALF_BAND_BUFSIZE", "MAX_INBUFSIZE", "MAX_MAGBUFSIZE", "MAX_SQBUF_SIZE", "BLANKER_CALL", "BLANKER_MAX_AVE",
             "MAX_FFT_SIZE", "MIN_FFT_SIZE", "MAX_NUMCOEF", "CONV_FFT_SIZE"]
    return lib()._cdll.ref_limit(names.index(name))


def tap_calls():
    """[(profile, n, is_complex, rate, first value)] of every DisplayData call since the last clear, all objects"""
    L = lib()._cdll
    out = []
    for i in range(L.ref_tap_calls()):
        p, n, c = C.c_int(), C.c_int(), C.c_int()
        r, f = C.c_double(), C.c_double()
        L.ref_tap_call(i, C.byref(p), C.byref(n), C.byref(c), C.byref(r), C.byref(f))
        out.append((p.value, n.value, bool(c.value), r.value, f.value))
    return out


def clear_tap_calls():
    lib()._cdll.ref_tap_calls_clear()


def _own(x):
    """a private copy: the reference works in place"""
    return np.array(x, copy=True)


def _refuse(cond, what):
    if cond:
        raise ValueError("refused, the reference's fixed buffer would overrun: " + what)


def _hb_check(stages, n):
    """every half-band stage but the 11-tap one copies its n input samples behind L - 1 kept ones (downconvert.cpp:295);
    ten stages leave m_pDecimatorPtrs[MAX_DECSTAGES] without the null that ends ProcessData's walk (downconvert.cpp:252)"""
    _refuse(len(stages) >= 10, "ten decimation stages, no end of the list")
    for i, code in enumerate(stages):
        if code not in (3, 11):
            _refuse((n >> i) + code - 1 > limit("MAX_HALF_BAND_BUFSIZE"), "%d samples into the %d-tap half band at stage %d" % (n >> i, code, i))


def _stage_count_check(in_rate, max_bw):
    """SetDataRate halves the rate while it is above max_bw / HB51TAP_MAX and above MIN_OUTPUT_RATE, one stage per
    halving, with no bound on their number (downconvert.cpp:127-166): the eleventh is written behind m_pDecimatorPtrs"""
    L = lib()._cdll
    f, n = in_rate, 0
    while f > max_bw / L.ref_dc_loop_const(0) and f > L.ref_dc_loop_const(1) and n <= 10:
        f /= 2.0
        n += 1
    _refuse(n > 10, "SetDataRate(%g, %g) would build more than ten stages" % (in_rate, max_bw))


class _Ref:
    _lib = staticmethod(lib)


class CFft(_Ref, _o.CFft):
    def SetFFTParams(self, size, invert, db_comp, fs):
        _refuse(size & (size - 1) != 0, "transform size %d is no power of two" % size)
        super().SetFFTParams(size, invert, db_comp, fs)

    def _size(self):
        return lib().orc_cfft_size(self.h)

    def PutInDisplayFFT(self, x):
        _refuse(len(x) > self._size(), "%d samples into a %d-point display transform" % (len(x), self._size()))
        return super().PutInDisplayFFT(_own(x))

    def GetScreenIntegerFFTData(self, max_h, max_w, max_db, min_db, start_hz, stop_hz):
        _refuse(max_w > self._size(), "%d pixels from a %d-entry translate table" % (max_w, self._size()))
        return super().GetScreenIntegerFFTData(max_h, max_w, max_db, min_db, start_hz, stop_hz)

    def WaterfallLine(self, *a, **k):
        raise NotImplementedError("gui/plotter.cpp is not part of the reference library")

    def FwdFFT(self, x):
        _refuse(len(x) != self._size(), "%d samples into a %d-point transform" % (len(x), self._size()))
        return super().FwdFFT(x)

    def RevFFT(self, x):
        _refuse(len(x) != self._size(), "%d samples into a %d-point transform" % (len(x), self._size()))
        return super().RevFFT(x)


_plain = {}


def fft(x, sign=+1):
    """CFft::FwdFFT (sign +1) / RevFFT (-1) at len(x) points, 512 ... 65536"""
    n = len(x)
    _refuse(n < limit("MIN_FFT_SIZE") or n > limit("MAX_FFT_SIZE"), "the reference clamps transform sizes to 512 ... 65536")
    if n not in _plain:
        _plain[n] = CFft()
        _plain[n].SetFFTParams(n, False, 0.0, 1.0)
    return _plain[n].FwdFFT(x) if sign > 0 else _plain[n].RevFFT(x)


def _only_2048(n):
    if n != 2048:
        raise ValueError("the reference's overlap-save filter has 2048 points (CONV_FFT_SIZE, dsp/fastfir.cpp:55), not %d" % n)


class CFastFIR(_Ref, _o.CFastFIR):
    def __init__(self, fft_size=2048):
        _only_2048(fft_size)
        super().__init__(fft_size)

    def set_faithful(self, on):
        if not on:
            raise NotImplementedError("the reference is what `faithful` means")

    def ProcessData(self, x):
        return super().ProcessData(_own(x))


class CDownConvert(_Ref, _o.CDownConvert):
    def SetDataRate(self, in_rate, max_bw):
        _stage_count_check(in_rate, max_bw)
        return super().SetDataRate(in_rate, max_bw)

    def ProcessData(self, x):
        _hb_check(self.stages(), len(x))
        return super().ProcessData(_own(x))


class CFir(_Ref, _o.CFir):
    def InitConstFir(self, coef):
        _refuse(len(coef) > limit("MAX_NUMCOEF"), "%d taps" % len(coef))
        super().InitConstFir(coef)

    def ProcessFilter(self, x):
        return super().ProcessFilter(_own(x))


class CIir(_Ref, _o.CIir):
    def ProcessFilter(self, x):
        return super().ProcessFilter(_own(x))


class CAgc(_Ref, _o.CAgc):
    def ProcessData(self, x):
        return super().ProcessData(_own(x))


class CSMeter(_Ref, _o.CSMeter):
    def ProcessData(self, x, fs):
        super().ProcessData(_own(x), fs)


class CNoiseProc(_Ref, _o.CNoiseProc):
    def SetupBlanker(self, On, Threshold, Width, SampleRate):
        if int(0.005 * SampleRate) > limit("BLANKER_MAX_AVE") - 1:      # MAGAVE_TIME, noiseproc.cpp:98 and :146
            raise ValueError("sample rate too high for the reference's 32768-entry average buffer")
        super().SetupBlanker(On, Threshold, Width, SampleRate)

    def ProcessBlanker(self, x):
        _refuse(len(x) > limit("BLANKER_CALL"), "%d samples into the blanker's 4096-entry test-bench buffer" % len(x))
        return super().ProcessBlanker(_own(x))


class CAmDemod(_Ref, _o.CAmDemod):
    def ProcessData(self, x, stereo=False):
        return super().ProcessData(_own(x), stereo)


class CSamDemod(_Ref, _o.CSamDemod):
    def ProcessData(self, x, stereo=False):
        return super().ProcessData(_own(x), stereo)


class CFmDemod(_Ref, _o.CFmDemod):
    def ProcessData(self, x, fm_bw, stereo=False):
        _refuse(len(x) > limit("MAX_SQBUF_SIZE"), "%d samples into CFmDemod" % len(x))
        return super().ProcessData(_own(x), fm_bw, stereo)


def ssb_demod(x, stereo=False):
    a = _o._c128(_own(x))
    if stereo:
        out = np.zeros_like(a); lib().orc_ssbdemod_process_stereo(len(a), _o._ptr(a), _o._ptr(out))
    else:
        out = np.zeros(len(a)); lib().orc_ssbdemod_process_mono(len(a), _o._ptr(a), _o._ptr(out))
    return out


class CFractResampler(_Ref, _o.CFractResampler):
    _max_input = None

    def Init(self, max_input):
        super().Init(max_input)
        self._max_input = max_input

    def Resample(self, x, rate, gain=None):
        _refuse(self._max_input is None or len(x) > self._max_input, "%d samples, Init(%r)" % (len(x), self._max_input))
        return super().Resample(_own(x), rate, gain)


class CDemodulator(_Ref, _o.CDemodulator):
    def __init__(self, fastfir_n=2048):
        _only_2048(fastfir_n)
        super().__init__(fastfir_n)

    def stages(self):
        codes = np.zeros(16, dtype=np.int32)
        n = lib()._cdll.ref_demod_stages(self.h, _o._ptr(codes))
        return list(codes[:n])

    def nco_freq(self):
        return lib()._cdll.ref_demod_nco_freq(self.h)

    def buf_pos(self):
        return lib()._cdll.ref_demod_buf_pos(self.h)

    def SetInputSampleRate(self, r):
        _stage_count_check(r, lib()._cdll.ref_demod_max_bw(self.h))
        super().SetInputSampleRate(r)

    def SetDemod(self, mode, info):
        _stage_count_check(lib()._cdll.ref_demod_input_rate(self.h), -info.LowCutmin if mode in (DEMOD_LSB, DEMOD_CWL) else info.HiCutmax)
        super().SetDemod(mode, info)

    def _check(self):
        lim, st = self.buf_limit(), self.stages()
        _refuse(lim > limit("MAX_INBUFSIZE"), "an input window of %d samples" % lim)
        _hb_check(st, lim)
        _refuse((lim >> len(st)) > min(limit("MAX_MAGBUFSIZE"), limit("MAX_SQBUF_SIZE")), "%d decimated samples per pass" % (lim >> len(st)))

    def ProcessData(self, x, stereo=False, out_cap=None):
        self._check()
        return super().ProcessData(_own(x), stereo, out_cap)

    def process_append(self, x):
        self._check()
        return super().process_append(_own(x))

    def perturb_filter_output(self, *a, **k):
        raise NotImplementedError("a hook of the oracle, not of the reference")

    def enable_taps(self, on=True):
        """the reference's tap points always call the test bench: see tap_calls()"""

    def clear_taps(self):
        clear_tap_calls()

    def tap(self, k):
        raise NotImplementedError("the test bench stub records calls, not buffers: tap_calls()")
