"""The K4 sample rule: an fp32 yardstick of the reference's post-chain stages in numpy, the window rule that holds the HIP
kernels to it, the guards on the test inputs and the yardstick with one thing wrong -- TEST INFRASTRUCTURE.

K4 (cutesdr_amd/csrc/postchain_kernels.hip: S-meter, AGC, AM / SAM / FM demodulators) was compared with the fp64 oracle at
absolute bounds (2e-5 of full scale, 0.01 dB): 30 ... 300 times its own error on strong signals, and no bound at all on weak
ones.  The rule here is relative and resolves what fp32 can do, in the shape of the K1 / K3 rules: with e = got - oracle,

    E = max|e| / rms(oracle output)  over a window of WIN = 1024 samples,        E <= M * E_y,

where E_y is the same figure of the YARDSTICK: the reference's loops restated statement by statement, in the reference's own
order (dsp/smeter.cpp:62-93, agc.cpp:104-296 / 301-401, amdemod.cpp:66-104, fmdemod.cpp:62-236, samdemod.cpp:54-158,
fir.cpp:72-127, iir.cpp:171-201), under a precision contract read from those loops and the product's sample type, not from any
kernel code path:

  * every quantity computed from the current sample is np.float32, each operation rounded: products, magnitudes, log10, sqrt,
    10**x, the sine / cosine of the loop phase as applied to the sample, atan2, FIR products and their running sum (added in
    the order of the reference's circular buffer), the stored output;
  * every quantity carried from one sample to the next is float64: averages, DC estimates, PLL phase and frequency, biquad
    delay words, the hang timer, ring positions.

The yardstick rotates and then takes atan2, as the reference does.  With dt = np.float64 every model here IS the oracle's
operation (tests/test_pc_samples_host.py pins it to oracle.CSMeter / CAgc / CAmDemod / CSamDemod / CFmDemod at 1e-12 of a
window's rms).  Windows are cut from the concatenated stream whatever the calls were; wherever the oracle's output is exactly
zero (a squelched FM burst, the AGC's delay line at the start) the other side must be exactly zero.  The S-meter uses the rule
on |delta dB| of GetAve / GetPeak after each call, largest over the stream's calls.

Filter designs are not restated: they come from the oracle's CFir / CIir (pinned elsewhere to 1e-14), through `Designs`."""
import math
import numpy as np
import pc_paths_ref as P

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                 # unit roundoff of fp32
WIN = 1024
M = 4.0                        # the project's margin for an fp32 kernel against an fp32 restatement (K1, K3)
MIN_RMS = 1e-3                 # counts: no compared window's reference output may lie below this
K_2PI = 2.0 * 3.14159265358979323846           # dsp/datatypes.h:44
FULL_SCALE = 32767.0
OLD_AUDIO, OLD_DB = 2e-5 * FULL_SCALE, 0.01    # the bounds K4 had: tests/test_postchain_gpu.py STEADY, the S-meter's 0.01 dB
PLL_SLIP = 0.25                # turns: a window in which the fp64 loop's phase error goes beyond this is left out
PLL_MAX_LEFT_OUT = 2
SQUELCH_CLEAR = 0.01           # of the threshold: how far the squelch average stays from both hysteresis edges

SM_ATTACK, SM_DECAY, SM_CAL, SM_MAX_PWR = .01, .5, 5.0, 32767.0 * 32767.0           # smeter.cpp:42-47
DC_ALPHA = 0.99                                                                      # amdemod.cpp:44, samdemod.cpp:45
FM_RANGE, FM_VOICE, FM_ZETA, FM_DC, FM_MAX_OUT = 6000.0, 3000.0, .707, 0.01, 25000.0  # fmdemod.cpp:45-53
FM_SQ_MAX, FM_SQ_TC, FM_SQ_HYST = 5000.0, .02, 100.0                                  # fmdemod.cpp:55-57
FM_MAX_SQBUF = 16384                                                                  # fmdemod.h:14 MAX_SQBUF_SIZE
SAM_BW, SAM_ZETA, SAM_LIMIT = 100.0, .707, 1000.0                                     # samdemod.cpp:47-49

FAULTS = ("agc_gain", "agc_slope", "dc_coef", "fm_gain", "fir_tap", "biquad_b0", "atan2", "sam_phase", "sm_coef", "sm_cal")


def f32_values(x):
    """the input as the product takes it: fp32 values, in the oracle's container"""
    x = np.asarray(x)
    return x.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(x) else x.astype(F32).astype(F64)


# ---- the window rule --------------------------------------------------------------------------------------------------------
def _rms(v):
    return math.sqrt(float(np.mean(np.abs(v) ** 2))) if len(v) else 0.0


def window_errors(got, want, win=WIN):
    """per window of the concatenated stream: (max|got - want| / rms(want), rms(want)); inf / 0 where want is all zeros"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    E, R = [], []
    for j in range(0, len(want), win):
        r = _rms(want[j:j + win])
        d = float(np.abs(got[j:j + win] - want[j:j + win]).max())
        E.append(d / r if r > 0 else (0.0 if d == 0 else math.inf)); R.append(r)
    return np.array(E), np.array(R)


class Windows:
    """what check_windows found: per window E, E_y, ratio = E / E_y, rms of the reference, the windows left out, and
    ok[w] (E <= m E_y, zeros equal); `zero_samples`: reference samples that are exactly zero, all equal on the other side"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def worst(self):
        r = self.ratio[self.compared]
        return float(r.max()) if len(r) else 0.0

    @property
    def passed(self):
        return bool(self.ok[self.compared].all()) and self.zeros_equal

    def __repr__(self):
        return "Windows(worst %.3g of m = %g, E_y %.3g ... %.3g, %d zero samples %s, left out %s)" % (
            self.worst, self.m, self.Ey[self.compared].min() if self.compared.any() else 0, self.Ey[self.compared].max() if self.compared.any() else 0,
            self.zero_samples, "equal" if self.zeros_equal else "DIFFER", list(np.nonzero(~self.compared)[0]))


def check_windows(got, want, model_out, m=M, leave_out=(), win=WIN):
    """the rule: E <= m E_y in every window not left out; a reference sample that is exactly zero is exactly zero in `got`
    (so a window of zeros is a window of zeros).  Returns a Windows; asserts nothing."""
    got, want, model_out = np.asarray(got), np.asarray(want), np.asarray(model_out)
    E, R = window_errors(got, want, win)
    Ey, _ = window_errors(model_out, want, win)
    compared = np.ones(len(E), dtype=bool)
    compared[list(leave_out)] = False
    compared &= R > 0                                     # an all-zero window is held by the zero rule alone
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(Ey > 0, E / Ey, np.where(E == 0, 0.0, np.inf))
    zero = want == 0
    return Windows(E=E, Ey=Ey, rms=R, ratio=ratio, m=m, compared=compared, ok=(E <= m * Ey),
                   zero_samples=int(zero.sum()), zero_windows=int((R == 0).sum()), zeros_equal=bool((got[zero] == 0).all()),
                   low=bool((R[compared] < MIN_RMS).any()))


def old_rule_accepts(got, want, bound=OLD_AUDIO):
    return bool(np.abs(np.asarray(got) - np.asarray(want)).max() <= bound)


def db_rule(got, want, model, m=M):
    """the S-meter form: (E, E_y, E / E_y) on the largest |delta dB| over the calls of a stream"""
    E = float(np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64)).max())
    Ey = float(np.abs(np.asarray(model, dtype=F64) - np.asarray(want, dtype=F64)).max())
    return E, Ey, (E / Ey if Ey > 0 else (0.0 if E == 0 else math.inf))


# ---- filter designs, from the oracle ------------------------------------------------------------------------------------------
class Designs:
    """CFir::InitLPFilter / InitHPFilter / GenerateHBFilter and CIir::Init* as the oracle designs them"""

    def __init__(self, oracle):
        self.o, self._c = oracle, {}

    def fir(self, kind, scale, astop, fpass, fstop, fs, hilbert=None):
        """(real-form taps, I taps, Q taps)"""
        key = (kind, scale, astop, fpass, fstop, fs, hilbert)
        if key not in self._c:
            f = self.o.CFir()
            (f.InitLPFilter if kind == "lp" else f.InitHPFilter)(scale, astop, fpass, fstop, fs)
            if hilbert is not None:
                f.GenerateHBFilter(hilbert)
            self._c[key] = tuple(np.array(v) for v in f.taps())
        return self._c[key]

    def iir(self, kind, f0, q, fs):
        """(b0, b1, b2, a1, a2)"""
        key = (kind, f0, q, fs)
        if key not in self._c:
            f = self.o.CIir(); f.Init(kind, f0, q, fs)
            self._c[key] = np.array(f.coefs())
        return self._c[key]


# ---- CFir::ProcessFilter (fir.cpp:72-127) ----------------------------------------------------------------------------------------
class Fir:
    """y[i] = sum_k h[k] x[i-k] with every product and every addition in dt, added in the order of the reference's circular
    buffer: sample i sits at position (-i) mod N and the loop runs over positions 0 .. N-1, so the sum starts at the tap
    k = i mod N and goes round.  The complex form runs the I taps on .re and the Q taps on .im (no cross terms)."""

    def __init__(self, taps, qtaps=None, dt=F32, bad_tap=None):
        self.dt = dt
        self.h = np.array(taps, dtype=F64)
        self.hq = self.h.copy() if qtaps is None else np.array(qtaps, dtype=F64)
        if bad_tap is not None:                                             # the fault model: one tap 1e-3 off
            self.h[bad_tap] *= 1.0 + 1e-3
            self.hq[bad_tap] *= 1.0 + 1e-3
        self.n, self.pos = len(self.h), 0
        self.zr, self.zi = np.zeros(self.n - 1, dtype=dt), np.zeros(self.n - 1, dtype=dt)

    def _one(self, h, x, z, want_s):
        dt, N, n = self.dt, self.n, len(x)
        e = np.concatenate([z, x.astype(dt)])
        if N == 1:
            p = (e * h.astype(dt))[:, None]
        else:
            p = np.lib.stride_tricks.sliding_window_view(e, N)[:, ::-1] * h.astype(dt)[None, :]          # p[i, k] = h[k] x[i-k], rounded
        k = ((self.pos + np.arange(n))[:, None] + np.arange(N)[None, :]) % N
        p = np.take_along_axis(p, k, axis=1)
        acc = p[:, 0].copy()
        s = np.abs(p[:, 0]).astype(F64) if want_s else None
        for j in range(1, N):
            acc = acc + p[:, j]
            if want_s:
                s += np.abs(p[:, j])
        return acc, e[len(e) - (N - 1):], s

    def run(self, x, want_s=False):
        """one call; with want_s also S[i] = sum_k |h[k] x[i-k]| (the derived bound of the leaf filters)"""
        x = np.asarray(x)
        if len(x) == 0:
            return (x.copy(), np.zeros(0)) if want_s else x.copy()
        if np.iscomplexobj(x):
            yr, self.zr, sr = self._one(self.h, x.real, self.zr, want_s)
            yi, self.zi, si = self._one(self.hq, x.imag, self.zi, want_s)
            y, s = yr.astype(F64) + 1j * yi.astype(F64), (np.hypot(sr, si) if want_s else None)
        else:
            y, self.zr, s = self._one(self.h, x, self.zr, want_s)
            y = y.astype(F64)
        self.pos += len(x)
        return (y, s) if want_s else y


# ---- CIir::ProcessFilter (iir.cpp:171-201) -----------------------------------------------------------------------------------------
class Biquad:
    """direct form II: the delay words are carried (float64); the output of a sample is stored in dt"""

    def __init__(self, coefs, dt=F32, b0_off=0.0):
        self.b0, self.b1, self.b2, self.a1, self.a2 = (float(v) for v in coefs)
        self.b0 *= 1.0 + b0_off
        self.dt, self.w = dt, [[0.0, 0.0], [0.0, 0.0]]

    def _one(self, x, w):
        b0, b1, b2, a1, a2 = self.b0, self.b1, self.b2, self.a1, self.a2
        w1, w2 = w
        y = np.empty(len(x))
        for i, v in enumerate(x.tolist()):
            w0 = v - a1 * w1 - a2 * w2
            y[i] = b0 * w0 + b1 * w1 + b2 * w2
            w2 = w1; w1 = w0
        w[0], w[1] = w1, w2
        return y.astype(self.dt).astype(F64)

    def run(self, x):
        x = np.asarray(x)
        if np.iscomplexobj(x):
            return self._one(x.real, self.w[0]) + 1j * self._one(x.imag, self.w[1])
        return self._one(x, self.w[0])


# ---- CSMeter (smeter.cpp:62-112) ------------------------------------------------------------------------------------------------
class SMeter:
    """the dB power of a sample is computed in dt; both averages and the peak are carried.  (1e-50 lies below fp32's range:
    it acts on a sample of zero power only, which it puts at -500 dB.)"""

    def __init__(self, dt=F32, fault=None):
        self.dt, self.fault = dt, fault
        self.att, self.dec, self.ave, self.peak, self.fs = -120.0, -120.0, 0.0, 0.0, 1.0
        self.aa = self.da = 1.0

    def process(self, x, fs):
        dt = self.dt
        if fs != self.fs:
            self.fs = fs
            self.aa = 1.0 - math.exp(-1.0 / (fs * SM_ATTACK))
            self.da = 1.0 - math.exp(-1.0 / (fs * SM_DECAY))
            if self.fault == "sm_coef":
                self.aa *= 1.01
        re, im = np.asarray(x).real.astype(dt), np.asarray(x).imag.astype(dt)
        p = (re * re + im * im) / dt(SM_MAX_PWR)
        if dt is F64:
            mag = 10.0 * np.log10(p + 1e-50)
        else:
            with np.errstate(divide="ignore"):
                mag = np.where(p > 0, dt(10.0) * np.log10(p), dt(-500.0)).astype(dt)
        aa, da, att, dec, ave, peak = self.aa, self.da, self.att, self.dec, self.ave, self.peak
        for m in mag.astype(F64).tolist():
            att = (1.0 - aa) * att + aa * m
            dec = (1.0 - da) * dec + da * m
            if att > dec:
                ave = att; dec = att
            else:
                ave = dec
            if m > peak:
                peak = m
        self.att, self.dec, self.ave, self.peak = att, dec, ave, peak

    def get_ave(self):
        return self.ave + (5.005 if self.fault == "sm_cal" else SM_CAL)

    def get_peak(self):
        v, self.peak = self.peak, 0.0
        return v + (5.005 if self.fault == "sm_cal" else SM_CAL)


# ---- CAgc (agc.cpp:104-401) -------------------------------------------------------------------------------------------------------
class Agc:
    """log magnitude, gain law and the product with the delayed sample in dt; window peak by comparison (a sliding maximum,
    as pc_paths_ref states it); both averagers, the hang timer and the rings carried.  `margin` is the smallest
    |peak - average| any comparison of the stream saw (log10 units)."""

    def __init__(self, on, hang, thresh, manual, slope, decay, fs, dt=F32, fault=None):
        self.on, self.dt, self.fault = bool(on), dt, fault
        self.p = P.AgcParams(hang, thresh, slope, decay, fs)
        self.manual = 32767.0 * 10.0 ** (-(100.0 - float(manual)) / 20.0)
        self.att = self.dec = -5.0
        self.timer, self.hist, self.margin = 0, None, math.inf
        self.dly = np.zeros(self.p.dly_n, dtype=np.complex128)

    def process(self, x):
        dt, p = self.dt, self.p
        x = np.asarray(x)
        cpx = np.iscomplexobj(x)
        xr, xi = x.real.astype(dt), (x.imag.astype(dt) if cpx else None)
        if not self.on:
            g = dt(self.manual)
            return (g * xr).astype(F64) + 1j * (g * xi).astype(F64) if cpx else (g * xr).astype(F64)
        m = np.maximum(np.abs(xr), np.abs(xi)) if cpx else np.abs(xr)
        mag = np.log10(m + dt(P.MIN_CONSTANT)) - dt(math.log10(P.MAX_AMPLITUDE))
        w1 = p.win_n - 1
        e = np.concatenate([np.full(w1, -16.0, dtype=dt) if self.hist is None else self.hist, mag.astype(dt)])
        pk = np.lib.stride_tricks.sliding_window_view(e, p.win_n).max(axis=1) if w1 else e
        self.hist = e[len(e) - w1:]
        ar, af, dr, df, hang, ht = p.att_rise, p.att_fall, p.dec_rise, p.dec_fall, p.hang, p.hang_time
        att, dec, timer, margin = self.att, self.dec, self.timer, self.margin
        lev = np.empty(len(x))
        for i, v in enumerate(pk.astype(F64).tolist()):
            margin = min(margin, abs(v - att), abs(v - dec))
            a = ar if v > att else af
            att = (1.0 - a) * att + a * v
            if v > dec:
                dec = (1.0 - dr) * dec + dr * v
                timer = 0
            elif hang and timer < ht:
                timer += 1
            else:
                dec = (1.0 - df) * dec + df * v
            lev[i] = att if att > dec else dec
        self.att, self.dec, self.timer, self.margin = att, dec, timer, margin
        sl = (p.gain_slope - 1.0) * (1.0 + 1e-4 if self.fault == "agc_slope" else 1.0)
        gain = np.where(lev <= p.knee, dt(p.fixed_gain), dt(P.OUTSCALE) * np.power(dt(10.0), lev.astype(dt) * dt(sl))).astype(dt)
        if self.fault == "agc_gain":
            gain = (gain * dt(1.0 + 1e-4)).astype(dt)
        line = np.concatenate([self.dly, x.astype(np.complex128)])
        self.dly = line[len(line) - p.dly_n:]
        d = line[:len(x)]
        if cpx:
            return (d.real.astype(dt) * gain).astype(F64) + 1j * (d.imag.astype(dt) * gain).astype(F64)
        return (d.real.astype(dt) * gain).astype(F64)


# ---- the demodulators ---------------------------------------------------------------------------------------------------------------
def _dc_block(v, z1, coef):
    """H(z) = (1 - z^-1) / (1 - ALPHA z^-1) on the reference's own variable (amdemod.cpp:73-77): z1 is carried"""
    y = np.empty(len(v))
    for i, m in enumerate(np.asarray(v, dtype=F64).tolist()):
        z0 = m + z1 * coef
        y[i] = z0 - z1
        z1 = z0
    return y, z1


class AmDemod:
    """CAmDemod (amdemod.cpp:50-104): envelope in dt, DC block on a carried z1 with the output stored in dt, Kaiser low-pass"""

    def __init__(self, designs, fs, dt=F32, fault=None):
        self.d, self.fs, self.dt, self.fault, self.z1 = designs, fs, dt, fault, 0.0
        self.set_bandwidth(10000.0)

    def set_bandwidth(self, bw):
        c, i, q = self.d.fir("lp", 1.0, 50.0, bw, bw * 1.8, self.fs)
        bad = len(c) // 2 - 2 if self.fault == "fir_tap" else None
        self.fir_r, self.fir_c = Fir(c, dt=self.dt, bad_tap=bad), Fir(i, q, dt=self.dt, bad_tap=bad)

    def process(self, x, stereo=False):
        dt = self.dt
        re, im = np.asarray(x).real.astype(dt), np.asarray(x).imag.astype(dt)
        mag = np.sqrt(re * re + im * im)
        y, self.z1 = _dc_block(mag, self.z1, 0.9901 if self.fault == "dc_coef" else DC_ALPHA)
        y = y.astype(dt)
        if stereo:
            return self.fir_c.run(y.astype(F64) + 1j * y.astype(F64))
        return self.fir_r.run(y)


class _Pll:
    def __init__(self, fs, bw, zeta, limit):
        norm = K_2PI / fs
        self.lo, self.hi = -limit * norm, limit * norm
        self.alpha = 2.0 * zeta * bw * norm
        self.beta = (self.alpha * self.alpha) / (4.0 * zeta * zeta)
        self.phase = self.freq = 0.0

    def walk(self, x, sin_sign, err_sign, dt, fault=None, fm=None):
        """the loop of fmdemod.cpp:165-188 / samdemod.cpp:81-107 / :118-147 over one call: the rotation and atan2 of a sample
        in dt (sine and cosine of the carried phase rounded to dt), frequency and phase carried.  Returns (rotated samples,
        the loop frequency after each sample or FM's audio, the phase error of each sample in radians)."""
        re, im = np.asarray(x).real.astype(dt), np.asarray(x).imag.astype(dt)
        n = len(re)
        tr, ti, out, errs = np.empty(n, dtype=dt), np.empty(n, dtype=dt), np.empty(n, dtype=dt), np.empty(n)
        ph, fr, lo, hi, alpha, beta = self.phase, self.freq, self.lo, self.hi, self.alpha, self.beta
        if fm is not None:
            dc, dca, gain = fm
            g = dt(gain)
        for i in range(n):
            pa = ph
            if fault == "sam_phase":
                pa = round(ph / K_2PI * 65536.0) / 65536.0 * K_2PI
            s, c = dt(sin_sign * math.sin(pa)), dt(math.cos(pa))
            a, b = re[i], im[i]
            r0 = c * a - s * b
            r1 = c * b + s * a
            if fault in ("theta_turns", "theta_unwrap32"):
                # the kernels' phase-domain form (postchain_kernels.hip, pll_theta_of / pll_step / pll_scan; FM's signs): theta =
                # atan2f(im, re) / 2 pi as an fp32 number of TURNS over the whole circle, error = -wrap(theta + phi) in float64.
                # "theta_unwrap32" is pll_scan as it was: the input phase unwrapped per tile of 1024 by wrapped DIFFERENCES taken
                # in fp32 -- across the half-turn wrap |d| is near 1, where fp32 is one bit coarser than the angles, so every wrap
                # leaves up to 2^-25 turns in the unwrapped phase for the rest of the tile, released as a step at the next tile
                th = dt(np.arctan2(b, a)) * dt(0.15915494309189535)
                if fault == "theta_unwrap32":
                    if i % 1024 == 0:
                        first, run, K = float(th), 0.0, round(float(th) + ph / K_2PI)
                    else:
                        d = th - th_prev
                        run += float(d - np.rint(d))
                    th_prev = th
                    err = ((K - first - run) - ph / K_2PI) * K_2PI
                else:
                    v = float(th) + ph / K_2PI
                    err = -(v - round(v)) * K_2PI
            else:
                err = err_sign * float(np.arctan2(r1, r0))
            if fault == "atan2":
                err += 1e-5 * math.sin(3.0 * err)
            fr += beta * err
            if fr > hi:
                fr = hi
            elif fr < lo:
                fr = lo
            ph += fr + alpha * err
            tr[i], ti[i], errs[i] = r0, r1, err
            if fm is not None:
                dc = (1.0 - dca) * dc + dca * fr
                out[i] = dt(fr - dc) * g
        self.phase, self.freq = math.fmod(ph, K_2PI), fr
        return tr, ti, out, errs, (dc if fm is not None else None)


class FmDemod:
    """CFmDemod (fmdemod.cpp:62-236): PLL discriminator, DC removal, then per CALL the noise squelch (Kaiser high-pass,
    |.|, 20 ms average on a carried value, hysteresis) and zeros or the 3 kHz biquad.  `sq_aves`: the squelch average at
    every call's end; `errs`: the phase error of every sample (radians)."""

    def __init__(self, designs, fs, dt=F32, fault=None):
        self.d, self.fs, self.dt, self.fault = designs, fs, dt, fault
        self.pll = _Pll(fs, FM_VOICE * 2.0, FM_ZETA, FM_RANGE)
        self.gain = FM_MAX_OUT / self.pll.hi * (1.0 + 1e-4 if fault == "fm_gain" else 1.0)
        self.dc, self.dca = 0.0, 1.0 - math.exp(-1.0 / (fs * FM_DC))
        self.sq_alpha = 1.0 - math.exp(-1.0 / (fs * FM_SQ_TC))
        self.sq_ave, self.squelched, self.thresh, self.hp_freq = 0.0, True, None, FM_VOICE
        self.lp = Biquad(designs.iir("LP", FM_VOICE, 1.0, fs), dt=dt, b0_off=1e-4 if fault == "biquad_b0" else 0.0)
        self._hp()
        self.sq_aves, self.decisions, self.errs = [], [], []

    def _hp(self):
        c, _, _ = self.d.fir("hp", 1.0, 50.0, self.hp_freq, self.hp_freq * .6, self.fs)
        self.hp = Fir(c, dt=self.dt)

    def set_squelch(self, value):
        self.thresh = FM_SQ_MAX - (FM_SQ_MAX * value) / 99

    def process(self, x, fm_bw, stereo=False):
        if fm_bw != self.hp_freq:
            self.hp_freq = fm_bw
            self._hp()
        _, _, out, errs, self.dc = self.pll.walk(x, 1.0, -1.0, self.dt, self.fault, fm=(self.dc, self.dca, self.gain))
        self.errs.append(errs)
        if len(out) > FM_MAX_SQBUF:                                      # fmdemod.cpp:115-116: no squelch, no low-pass on such a call
            self.sq_aves.append(self.sq_ave); self.decisions.append(self.squelched)
            y = out.astype(F64)
            return y + 1j * y if stereo else y
        mag = np.abs(self.hp.run(out))
        a, ave = self.sq_alpha, self.sq_ave
        for v in mag.tolist():
            ave = (1.0 - a) * ave + a * v
        self.sq_ave = ave
        if self.thresh == 0:
            self.squelched = True
        elif self.squelched:
            if ave < self.thresh - FM_SQ_HYST:
                self.squelched = False
        elif ave >= self.thresh + FM_SQ_HYST:
            self.squelched = True
        self.sq_aves.append(ave); self.decisions.append(self.squelched)
        y = np.zeros(len(out)) if self.squelched else self.lp.run(out.astype(F64))
        return y + 1j * y if stereo else y


class SamDemod:
    """CSamDemod (samdemod.cpp:54-158): mono rotates by e^{-j phi} and takes +atan2, stereo by e^{+j phi} and -atan2; DC
    blockers on carried z1 / y1; stereo through the Hilbert pair, then sum and difference in dt"""

    def __init__(self, designs, fs, dt=F32, fault=None):
        self.dt, self.fault = dt, fault
        self.pll = _Pll(fs, SAM_BW, SAM_ZETA, SAM_LIMIT)
        self.z1 = self.y1 = 0.0
        _, i, q = designs.fir("lp", 1.0, 40.0, 4500, 5500, fs, hilbert=5000.0)
        self.fir = Fir(i, q, dt=dt, bad_tap=len(i) // 2 - 2 if fault == "fir_tap" else None)
        self.errs = []

    def process(self, x, stereo=False):
        dt = self.dt
        coef = 0.9901 if self.fault == "dc_coef" else DC_ALPHA
        sgn = 1.0 if stereo else -1.0
        tr, ti, _, errs, _ = self.pll.walk(x, sgn, -sgn, dt, self.fault)
        self.errs.append(errs)
        a, self.z1 = _dc_block(tr, self.z1, coef)
        a = a.astype(dt)
        if not stereo:
            return a.astype(F64)
        b, self.y1 = _dc_block(ti, self.y1, coef)
        f = self.fir.run(a.astype(F64) + 1j * b.astype(dt).astype(F64))
        fr, fi = f.real.astype(dt), f.imag.astype(dt)
        return (fr + fi).astype(F64) + 1j * (fr - fi).astype(F64)


class PostChain:
    """the stages behind the filter of one receiver as CDemodulator::SetDemod configures them (demodulator.cpp:107-157,
    :183-260): S-meter on the filter output, AGC, demodulator -- the shape of test_chain_taps_gpu._oracle_post_chain.
    info: the tDemodInfo fields as a dict"""

    def __init__(self, designs, mode, info, fs, dt=F32):
        self.mode, self.info, self.fs = mode, info, fs
        self.sm = SMeter(dt)
        self.agc = Agc(info["AgcOn"], info["AgcHangOn"], info["AgcThresh"], info["AgcManualGain"], info["AgcSlope"], info["AgcDecay"], fs, dt)
        self.dem = None
        if mode == "AM":
            self.dem = AmDemod(designs, fs, dt); self.dem.set_bandwidth((info["HiCut"] - info["LowCut"]) / 2.0)
        elif mode == "SAM":
            self.dem = SamDemod(designs, fs, dt)
        elif mode == "FM":
            self.dem = FmDemod(designs, fs, dt); self.dem.set_squelch(info["SquelchValue"])

    def process(self, z):
        self.sm.process(z, self.fs)
        a = self.agc.process(z)
        if self.mode == "FM":
            return self.dem.process(a, float(self.info["HiCut"]))
        if self.dem is not None:
            return self.dem.process(a)
        return a.real.copy()                                           # ssbdemod.cpp:48-53, mono


# ---- guards: computed from the reference's statement (dt = float64) alone ------------------------------------------------------------
def pll_windows_left_out(errs, win=WIN):
    """windows of the stream in which the fp64 loop's phase error exceeds PLL_SLIP turns anywhere"""
    e = np.abs(np.concatenate(errs)) / K_2PI
    return [w for w, j in enumerate(range(0, len(e), win)) if e[j:j + win].max() > PLL_SLIP]


def squelch_clear(fm):
    """every call end's squelch average at least SQUELCH_CLEAR x threshold from both hysteresis edges"""
    a = np.array(fm.sq_aves)
    return bool((np.abs(a - (fm.thresh - FM_SQ_HYST)) >= SQUELCH_CLEAR * fm.thresh).all()
                and (np.abs(a - (fm.thresh + FM_SQ_HYST)) >= SQUELCH_CLEAR * fm.thresh).all())


def agc_undecided_share(params, x, calls, burst=None):
    """share of the stream's tiles in which a comparison of the selector iteration comes within pc_paths_ref.TIE"""
    _, rec = P.agc_stream(params, x, calls, burst)
    d = P.decided(rec)
    return 1.0 - sum(d) / max(len(d), 1)


# ---- the inputs of tests/test_pc_samples_gpu.py (tests/test_pc_samples_host.py checks every condition on them) ------------------------
N_STREAM = 8 * WIN
CUTS = [1, 17, 1000, 1025, 2500, 1, 4099, 333, 2048]           # test_leaf_objects_ragged_call_lengths
EVEN = [WIN] * 8
FS_AM, FS_FM, FS_AGC = 31250.0, 62500.0, 62500.0
# name: amplitude of the carrier in counts.  Three levels of the same input and one above full scale.
LEVELS = {"-12dBFS": FULL_SCALE * 10 ** (-12 / 20.0), "-60dBFS": FULL_SCALE * 1e-3, "-100dBFS": FULL_SCALE * 1e-5, "over": 40000.0}
AGC_SETTINGS = [(0, 0, -100, 200), (1, 5, -60, 500), (0, 10, -20, 50)]      # hang, slope, thresh, decay: test_agc_complex_and_real
MANUAL_GAINS = [0, 30, 60]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(0xC0DE0000 + seed))


def am_input(level, n=N_STREAM, fs=FS_AM, fc=150.0):
    """an AM carrier fc off tune, 800 Hz tone at 60 %, noise 58 dB under the carrier -- scaled as a whole"""
    t = np.arange(n) / fs
    r = _rng(11)
    x = (1.0 + 0.6 * np.sin(2 * np.pi * 800.0 * t)) * np.exp(2j * np.pi * fc * t) + 1.26e-3 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return f32_values(LEVELS[level] * x)


def fm_input(level, n=N_STREAM, fs=FS_FM, fc=300.0):
    """an FM carrier 300 Hz off tune, 1 kHz tone at 3 kHz deviation, noise 54 dB under it -- scaled as a whole"""
    t = np.arange(n) / fs
    r = _rng(12)
    x = np.exp(1j * (2 * np.pi * fc * t + 3.0 * np.sin(2 * np.pi * 1000.0 * t))) + 2e-3 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return f32_values(LEVELS[level] * x)


def fm_noise_input(n=N_STREAM):
    """no carrier: the squelch stays shut"""
    r = _rng(13)
    return f32_values(3000.0 * (r.standard_normal(n) + 1j * r.standard_normal(n)))


def steps_input(level, n=N_STREAM, fs=FS_AGC, seed=14):
    """level steps of 34 dB every 25 ms under a 30 Hz modulation (pc_paths_ref.agc_input's envelope): the AGC's averagers and
    the S-meter's two averages cross in most windows.  `level` is the upper step's."""
    t = np.arange(n) / fs
    r = _rng(seed)
    env = np.where((t % 0.05) < 0.025, 1.0, 0.02) * (1 + 0.3 * np.sin(2 * np.pi * 30 * t))
    x = env * np.exp(2j * np.pi * 1000 * t) + 1.7e-3 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return f32_values(LEVELS[level] * x)


def split(x, calls):
    assert sum(calls) == len(x), (sum(calls), len(x))
    c = np.cumsum([0] + list(calls))
    return [x[c[k]:c[k + 1]] for k in range(len(calls))]


# ---- running a stream through one side ------------------------------------------------------------------------------------------------
def run_stream(obj, parts, *args):
    """concatenated output of obj.process (a model) or obj.ProcessData (oracle / product) over the calls"""
    f = obj.process if hasattr(obj, "process") else obj.ProcessData
    return np.concatenate([f(p, *args) for p in parts])


def smeter_stream(obj, parts, fs):
    """(GetAve after each call, GetPeak after each call)"""
    ave, peak = [], []
    for p in parts:
        if hasattr(obj, "process"):
            obj.process(p, fs); ave.append(obj.get_ave()); peak.append(obj.get_peak())
        else:
            obj.ProcessData(p, fs); ave.append(obj.GetAve()); peak.append(obj.GetPeak())
    return np.array(ave), np.array(peak)


# ---- the rows of the leaf tests: (stage, form, settings, input, calls), built alike on the model, the oracle and the product -----------
class Row:
    """one leaf stream.  stage: smeter | agc | am | sam | fm; form: the column of DESIGN.md's table.  build(side) makes the
    object on a side -- "model" (with dt and fault), or a module with the reference's class names (the oracle, the product);
    run(obj) gives the concatenated output, for the S-meter (GetAve, GetPeak) after each call."""

    def __init__(self, name, stage, form, x, calls, level=None, fs=None, stereo=False, real=False, agc=None, manual=None, carrier=True):
        self.name, self.stage, self.form, self.calls, self.level, self.fs = name, stage, form, list(calls), level, fs
        self.stereo, self.real, self.agc, self.manual, self.carrier = stereo, real, agc, manual, carrier
        self.x = x.real.copy() if real else x

    def build(self, side, designs=None, dt=F32, fault=None):
        model = side == "model"
        if self.stage == "smeter":
            return SMeter(dt, fault) if model else side.CSMeter()
        if self.stage == "agc":
            on = self.manual is None
            hang, slope, thresh, decay = self.agc if on else AGC_SETTINGS[0]
            args = (on, bool(hang), thresh, 30 if on else self.manual, slope, decay, self.fs)
            if model:
                return Agc(*args, dt=dt, fault=fault)
            o = side.CAgc(); o.SetParameters(*args)
            return o
        if self.stage == "am":
            o = AmDemod(designs, self.fs, dt, fault) if model else side.CAmDemod(self.fs)
            (o.set_bandwidth if model else o.SetBandwidth)(4000.0)
            return o
        if self.stage == "sam":
            return SamDemod(designs, self.fs, dt, fault) if model else side.CSamDemod(self.fs)
        o = FmDemod(designs, self.fs, dt, fault) if model else side.CFmDemod(self.fs)
        (o.set_squelch if model else o.SetSquelch)(50)
        return o

    def run(self, obj):
        parts = split(self.x, self.calls)
        if self.stage == "smeter":
            return smeter_stream(obj, parts, self.fs)
        if self.stage == "agc":
            return run_stream(obj, parts)
        if self.stage == "fm":
            return run_stream(obj, parts, 5000.0, self.stereo)
        return run_stream(obj, parts, self.stereo)

    def faults(self):
        """the fault models that apply to this row"""
        if not self.carrier:
            return ()
        return {"smeter": ("sm_coef", "sm_cal"), "agc": ("agc_gain", "agc_slope") if self.manual is None else (),
                "am": ("dc_coef", "fir_tap"), "sam": ("dc_coef", "atan2", "sam_phase") + (("fir_tap",) if self.stereo else ()),
                "fm": ("fm_gain", "biquad_b0", "atan2")}[self.stage]


_rows = None


def leaf_rows():
    """{name: Row}: a. every object and form at the three levels and above full scale in even calls of one tile; the manual
    gains; FM without a carrier; b. one stream per stage through the ragged cuts (tile and call edges)"""
    global _rows
    if _rows is not None:
        return _rows
    rows = []
    for lev in LEVELS:
        st, am, fm = steps_input(lev), am_input(lev), fm_input(lev)
        rows.append(Row("smeter/%s" % lev, "smeter", "S-meter", st, EVEN, lev, FS_AGC))
        for k, s in enumerate(AGC_SETTINGS):
            rows.append(Row("agc%d/cpx/%s" % (k, lev), "agc", "AGC complex", st, EVEN, lev, FS_AGC, agc=s))
            rows.append(Row("agc%d/real/%s" % (k, lev), "agc", "AGC real", st, EVEN, lev, FS_AGC, agc=s, real=True))
        for stereo, w in ((False, "mono"), (True, "stereo")):
            rows.append(Row("am/%s/%s" % (w, lev), "am", "AM", am, EVEN, lev, FS_AM, stereo=stereo))
            rows.append(Row("sam/%s/%s" % (w, lev), "sam", "SAM " + w, am, EVEN, lev, FS_AM, stereo=stereo))
            rows.append(Row("fm/%s/%s" % (w, lev), "fm", "FM " + w, fm, EVEN, lev, FS_FM, stereo=stereo))
    for lev in ("-12dBFS", "over"):
        for g in MANUAL_GAINS:
            rows.append(Row("manual%d/cpx/%s" % (g, lev), "agc", "AGC manual", steps_input(lev), EVEN, lev, FS_AGC, manual=g))
            rows.append(Row("manual%d/real/%s" % (g, lev), "agc", "AGC manual", steps_input(lev), EVEN, lev, FS_AGC, manual=g, real=True))
    rows.append(Row("fm/mono/nocarrier", "fm", "FM mono", fm_noise_input(), EVEN, None, FS_FM, carrier=False))
    n, lev = sum(CUTS), "-12dBFS"
    st, am, fm = steps_input(lev, n, FS_AM), am_input(lev, n), fm_input(lev, n)
    rows.append(Row("cuts/smeter", "smeter", "S-meter", st, CUTS, lev, FS_AM))
    rows.append(Row("cuts/agc0/cpx", "agc", "AGC complex", st, CUTS, lev, FS_AM, agc=AGC_SETTINGS[0]))
    rows.append(Row("cuts/agc1/real", "agc", "AGC real", st, CUTS, lev, FS_AM, agc=AGC_SETTINGS[1], real=True))
    rows.append(Row("cuts/am/mono", "am", "AM", am, CUTS, lev, FS_AM))
    for stereo, w in ((False, "mono"), (True, "stereo")):
        rows.append(Row("cuts/sam/" + w, "sam", "SAM " + w, am, CUTS, lev, FS_AM, stereo=stereo))
        rows.append(Row("cuts/fm/" + w, "fm", "FM " + w, fm, CUTS, lev, FS_FM, stereo=stereo))
    _rows = {r.name: r for r in rows}
    assert len(_rows) == len(rows)
    return _rows


_model_cache = {}


def model_output(row, designs, dt=F32, fault=None):
    """(output, the model object) of a row on the model, computed once per (row, dt, fault)"""
    key = (row.name, dt, fault)
    if key not in _model_cache:
        m = row.build("model", designs, dt, fault)
        _model_cache[key] = (row.run(m), m)
    return _model_cache[key]


def manual_bound(want):
    """AGC off: one rounding of the gain, one of the product"""
    return 2.0 * U * np.abs(want)
