"""CPU model of the path decisions of the post-chain walk (K4, cutesdr_amd/csrc/postchain_kernels.hip), in numpy.

AGC (pc_agc_stage): the kernel takes fp32 log magnitudes and their fp32 sliding maximum (the "peaks"), and solves the two
piecewise-linear averagers of a 1024-sample tile by guessing the selector bits (peak > average?), solving the then-linear
recurrence and re-deriving the selectors until they reproduce themselves (agc_ave_scan / agc_ave_scan2, at most PC_AGC_ROUNDS
rounds; otherwise the tile is walked sample by sample).  This module computes the peaks the same way, walks both averagers
sequentially in fp64 (that walk is what tests/test_pc_paths_host.py pins to oracle.CAgc), and counts, per tile, the rounds the
selector iteration needs -- from the same start (every selector taken against the average the tile starts with) and with the
same update, so the count is the kernel's as long as no comparison is a near tie: the kernel's peaks may differ from numpy's
by an fp32 rounding of log10f, its averages by the order of a scan's additions.  A tile in which any comparison of any round
has |peak - average| < TIE (log10 units) is "undecided" and left out of exact comparisons.

PLL: there is no per-sample model.  Inputs are built in segments whose path is known by construction (pll_segments).

The census records of the diagnostic build (postchain.h, -DPC_CENSUS) are decoded here too (decode), so that the host and the
GPU tests speak of paths in the same words."""
import math
import numpy as np

PT = 1024                  # the walk's tile (pc_scan.hpp)
AGC_ROUNDS = 8             # PC_AGC_ROUNDS
AGC_RING = 2048
TIE = 1e-6                 # log10 units
UNDECIDED_CAP = 0.05       # at most this share of a test's tiles may be undecided

# dsp/agc.cpp:50-72, as oracle/cutesdr_oracle.c and ref_constants.hpp name them
DELAY_TIMECONST, WINDOW_TIMECONST = .015, .018
ATTACK_RISE_TIMECONST, ATTACK_FALL_TIMECONST = .002, .005
DECAY_RISEFALL_RATIO, RELEASE_TIMECONST = .3, .05
OUTSCALE, MAX_AMPLITUDE, MIN_CONSTANT = 0.7, 32767.0, 3.2767e-4


class AgcParams:
    """CAgc::SetParameters (agc.cpp:104-167) with the AGC on"""

    def __init__(self, hang, thresh, slope, decay, fs):
        self.hang, self.fs = bool(hang), float(fs)
        self.knee = thresh / 20.0
        self.gain_slope = slope / 100.0
        self.fixed_gain = OUTSCALE * 10.0 ** (self.knee * (self.gain_slope - 1.0))
        self.att_rise = 1.0 - math.exp(-1.0 / (fs * ATTACK_RISE_TIMECONST))
        self.att_fall = 1.0 - math.exp(-1.0 / (fs * ATTACK_FALL_TIMECONST))
        self.dec_rise = 1.0 - math.exp(-1.0 / (fs * decay * .001 * DECAY_RISEFALL_RATIO))
        self.hang_time = int(fs * decay * .001)
        self.dec_fall = 1.0 - math.exp(-1.0 / (fs * RELEASE_TIMECONST)) if hang else 1.0 - math.exp(-1.0 / (fs * decay * .001))
        self.dly_n = max(1, min(int(fs * DELAY_TIMECONST), AGC_RING - 1))
        self.win_n = max(1, min(int(fs * WINDOW_TIMECONST), AGC_RING))


def log_mags(x):
    """fp32 log magnitudes of complex samples as the kernel takes them (agc.cpp:196-201 in fp32)"""
    x = np.asarray(x)
    re, im = np.abs(x.real.astype(np.float32)), np.abs(x.imag.astype(np.float32))
    m = np.maximum(re, im)
    return (np.log10(m + np.float32(MIN_CONSTANT)) - np.float32(math.log10(MAX_AMPLITUDE))).astype(np.float32)


def sliding_peaks(mg, win_n, history=None):
    """peak[i] = max of the last win_n log magnitudes, the current one included; in front of the stream the ring holds -16
    (agc.cpp:121-136).  Returns (peaks, the last win_n - 1 magnitudes: the next call's history)."""
    w1 = win_n - 1
    hist = np.full(w1, -16.0, dtype=np.float32) if history is None else np.asarray(history, dtype=np.float32)
    e = np.concatenate([hist, np.asarray(mg, dtype=np.float32)])
    if w1 == 0:
        return e.copy(), e[:0]
    win = np.lib.stride_tricks.sliding_window_view(e, win_n)
    return win.max(axis=1), e[len(e) - w1:]


def cut_tiles(calls, burst=None):
    """[(start, n)] of the tiles of a stream given as call lengths: a leaf object's call is ONE burst (burst = None), a chain's
    call is whole bursts of `burst` samples; tiles of PT are cut from each burst's start, the last one short"""
    out, pos = [], 0
    for m in calls:
        b = m if burst is None else burst
        assert b > 0 and m % b == 0
        for b0 in range(0, m, b):
            for t0 in range(0, b, PT):
                out.append((pos + b0 + t0, min(PT, b - t0)))
        pos += m
    return out


def _rounds(pk, ave0, rise, fall, limit=64):
    """rounds of agc_ave_scan's selector iteration on one tile (None beyond `limit`) and the smallest |peak - average| any
    comparison of any round saw"""
    n = len(pk)
    margin = float(np.abs(pk - ave0).min()) if n else float("inf")
    sel = pk > ave0
    for rnd in range(limit):
        al = np.where(sel, rise, fall)
        x, before = ave0, np.empty(n)
        for j in range(n):
            before[j] = x
            x = x + al[j] * (pk[j] - x)
        margin = min(margin, float(np.abs(pk - before).min()) if n else float("inf"))
        nsel = pk > before
        if (nsel == sel).all():
            return rnd + 1, margin
        sel = nsel
    return None, margin


class AgcModel:
    """the AGC of one stream: peaks, the sequential averagers, the gain and the delayed output, and per tile the rounds of the
    two selector iterations"""

    def __init__(self, params):
        self.p = params
        self.att, self.dec, self.timer = -5.0, -5.0, 0
        self.hist = None
        self.dly = np.zeros(params.dly_n, dtype=np.complex128)

    def peaks_of(self, x):
        pk, self.hist = sliding_peaks(log_mags(x), self.p.win_n, self.hist)
        return pk.astype(np.float64)

    def walk(self, pk):
        """both averagers over the peaks pk, sample by sample (agc.cpp:233-262); returns (attack, decay) after every sample"""
        p, att, dec, timer = self.p, self.att, self.dec, self.timer
        va, vd = np.empty(len(pk)), np.empty(len(pk))
        for i, v in enumerate(pk):
            att = att + (p.att_rise if v > att else p.att_fall) * (v - att)
            if v > dec:
                dec = dec + p.dec_rise * (v - dec)
                timer = 0
            elif p.hang and timer < p.hang_time:
                timer += 1
            else:
                dec = dec + p.dec_fall * (v - dec)
            va[i], vd[i] = att, dec
        self.att, self.dec, self.timer = att, dec, timer
        return va, vd

    def gains(self, va, vd):
        m = np.maximum(va, vd)
        return np.where(m <= self.p.knee, self.p.fixed_gain, OUTSCALE * 10.0 ** (m * (self.p.gain_slope - 1.0)))

    def process(self, x, tiles=None):
        """one call: returns (output, [(rounds of the attack scan, rounds of the decay scan, margin)] per tile of `tiles`
        = [(start in x, n)]).  A count is None where the iteration has not converged in 64 rounds."""
        x = np.asarray(x, dtype=np.complex128)
        pk = self.peaks_of(x)
        rec = []
        va, vd = np.empty(len(x)), np.empty(len(x))
        for start, n in (tiles if tiles is not None else [(0, len(x))]):
            seg = pk[start:start + n]
            if not self.p.hang:
                ra, ma = _rounds(seg, self.att, self.p.att_rise, self.p.att_fall)
                rd, md = _rounds(seg, self.dec, self.p.dec_rise, self.p.dec_fall)
                rec.append((ra, rd, min(ma, md)))
            else:
                rec.append((0, 0, float("inf")))
            va[start:start + n], vd[start:start + n] = self.walk(seg)
        g = self.gains(va, vd)
        line = np.concatenate([self.dly, x.astype(np.complex64).astype(np.complex128)])
        self.dly = line[len(line) - self.p.dly_n:]
        return line[:len(x)] * g, rec


def agc_stream(params, x, calls, burst=None):
    """a whole stream cut into calls: (output, per tile (rounds_att, rounds_dec, margin)) in stream order"""
    m = AgcModel(params)
    out, rec, pos = [], [], 0
    for n in calls:
        y, r = m.process(x[pos:pos + n], cut_tiles([n], burst))
        out.append(y); rec += r
        pos += n
    return np.concatenate(out), rec


def scan2_rounds(rec):
    """rounds of agc_ave_scan2 (both averagers in lockstep: a fixed point of one stays one) per tile"""
    return [None if ra is None or rd is None else max(ra, rd) for ra, rd, _ in rec]


def decided(rec):
    return [m >= TIE for _, _, m in rec]


def histogram(rounds):
    """{rounds: tiles}"""
    h = {}
    for r in rounds:
        h[r] = h.get(r, 0) + 1
    return h


def agc_path(ra, rd, limit, nw):
    """what the census must say of a hang-off tile under a round limit: (path, rounds word, which-failed) -- see decode()"""
    big = lambda r: r is None or r > limit
    if nw == 4:
        r = None if big(ra) or big(rd) else max(ra, rd)
        return ("scan", r, 0) if r is not None else ("walk_rounds", 0, 0)
    if big(ra):
        return ("walk_rounds", 0, 1)
    if big(rd):
        return ("walk_rounds", ra, 2)
    return ("scan", (ra, rd), 0)


# ---- the census buffer of the diagnostic build (postchain.h) -------------------------------------------------------------
HEADER_WORDS, RECORD_WORDS = 8, 4
AGC_PATHS = ["off", "manual", "scan", "walk_hang", "walk_rounds"]
PLL_PATHS = ["none", "scan", "overlap", "walk"]
FORCE_SKIP_SCAN = 16


def force_word(agc_limit=None, skip_scan=False, overlap_mod=0, overlap_rem=0):
    return (0 if agc_limit is None else agc_limit + 1) | (FORCE_SKIP_SCAN if skip_scan else 0) | overlap_mod << 8 | overlap_rem << 16


def decode(words):
    """the buffer's words -> (header dict, list of record dicts in buffer order)"""
    w = np.asarray(words, dtype=np.uint32)
    head = dict(capacity=int(w[1]), force=int(w[2]), nw=int(w[3] & 255), lean=bool(w[3] >> 8 & 1), records=int(w[4]), walks=int(w[5]))
    recs = []
    for k in range(min(head["records"], head["capacity"])):
        p, a, b, o = (int(v) for v in w[HEADER_WORDS + RECORD_WORDS * k:HEADER_WORDS + RECORD_WORDS * (k + 1)])
        recs.append(dict(agc=AGC_PATHS[p & 7], rounds=p >> 4 & 15, rounds2=p >> 8 & 15, failed=p >> 12 & 3,
                         pll=PLL_PATHS[p >> 16 & 3], scan_bad=bool(p >> 18 & 1), zero_code=bool(p >> 19 & 1),
                         scan_skipped=bool(p >> 20 & 1), overlap_skip_warm=bool(p >> 21 & 1), overlap_skip_seq=bool(p >> 22 & 1),
                         overlap_forced=bool(p >> 23 & 1), n=a & 0xffff, mode=(a >> 16 & 15) - 1, nw=a >> 20 & 255, lean=bool(a >> 28 & 1), walk=b & 0xffff, ch=b >> 16 & 255,
                         row=b >> 24, ordinal=o, raw=p))
    return head, recs


# ---- PLL inputs whose path is known by construction ------------------------------------------------------------------------
def pll_segments(kind, fs, seed, tiles_per_segment=4):
    """(x, [(first tile, tiles, expected)]) for a CFmDemod ("fm", fs 62500) or CSamDemod ("sam", fs 31250) leaf fed in tiles of
    PT: segments of whole tiles, each with what the census must show.  expected is "scan" (from the segment's third tile: the
    loop has locked), "never_scan" (every tile long enough to hold a cycle slip) or "zero" (every tile: a zero-sample code):
      a clean carrier well inside the clamp | exact zeros (a muted input) | the carrier again | a carrier outside the
      frequency clamp | noise without a carrier | the carrier again"""
    rng = np.random.default_rng(seed)
    lim = 6000.0 if kind == "fm" else 1000.0       # inside the loops' clamps (FM_PLL_RANGE, SAM_PLL_LIMIT)
    n = tiles_per_segment * PT
    t = np.arange(n) / fs

    def carrier(f, level=6000.0):
        amp = level * (1.0 + 0.4 * np.sin(2 * np.pi * 300.0 * t)) if kind == "sam" else level
        return amp * np.exp(2j * np.pi * f * t) + 3.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))

    f1, f2, f3 = (0.2 * lim, -0.3 * lim, 0.1 * lim) if kind == "fm" else (0.05 * lim, -0.08 * lim, 0.03 * lim)   # (SAM: inside the
    parts = [(carrier(f1), "scan"), (np.zeros(n, dtype=np.complex128), "zero"), (carrier(f2), "scan"),             # 100 Hz loop's pull-in)
             (carrier(3.0 * lim), "never_scan"), (3000.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)), "never_scan"),
             (carrier(f3), "scan")]
    x = np.concatenate([p for p, _ in parts])
    segs = [(k * tiles_per_segment, tiles_per_segment, what) for k, (_, what) in enumerate(parts)]
    return x, segs


# ---- the inputs of tests/test_pc_paths_gpu.py (tests/test_pc_paths_host.py asserts what that test relies on) -----------------
AGC_CALLS = [1, 37, 1024, 1500, 4096, 1024, 1500, 4096, 37, 1, 4096, 1500]      # 24 tiles, ragged
# name: (fs, hang, thresh, slope, decay, seed).  Level steps every 25 ms under a 30 Hz modulation: the averagers cross the
# peak in most tiles, and no comparison comes near a tie (noise and AM tones leave 4 ... 80 % of the tiles undecided).
AGC_CASES = {"steps62k5": (62500.0, False, -100, 0, 200, 1), "steps15k6": (15625.0, False, -100, 0, 50, 1),
             "hang62k5": (62500.0, True, -60, 5, 500, 1)}
# the histograms {rounds of agc_ave_scan2: tiles} the GPU test relies on (asserted against the model on the host)
AGC_HISTOGRAMS = {"steps62k5": {1: 19, 2: 5}, "steps15k6": {1: 5, 2: 15, 3: 4}}


def agc_input(name):
    fs, hang, thresh, slope, decay, seed = AGC_CASES[name]
    n = sum(AGC_CALLS)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    env = np.where((t % 0.05) < 0.025, 3000.0, 60.0) * (1 + 0.3 * np.sin(2 * np.pi * 30 * t))
    return env * np.exp(2j * np.pi * 1000 * t) + 5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def agc_params(name):
    fs, hang, thresh, slope, decay, seed = AGC_CASES[name]
    return AgcParams(hang, thresh, slope, decay, fs)


PLL_CALLS = [1024] * 6 + [1500, 4096, 37, 1, 1024, 4096, 1500, 1024, 4096, 37, 1, 4096, 3068, 1024 * 6]   # 36 tiles of input, ragged in the middle
PLL_FS = {"fm": 62500.0, "sam": 31250.0}
PLL_SETTLE = {"fm": 2, "sam": 4}           # tiles after a frequency jump before the oracle bound applies (test_postchain_gpu.py)


def pll_tile_expectations(kind, seed=5):
    """(x, [(start, n, segment kind, tiles since the segment began) per tile of PLL_CALLS; kind None where a tile straddles two
    segments])"""
    x, segs = pll_segments(kind, PLL_FS[kind], seed, tiles_per_segment=6)
    assert sum(PLL_CALLS) == len(x)
    out = []
    for start, n in cut_tiles(PLL_CALLS):
        s0, s1 = start // (6 * PT), (start + n - 1) // (6 * PT)
        out.append((start, n, segs[s0][2] if s0 == s1 else None, (start - s0 * 6 * PT) // PT))
    return x, out


# ---- the chain input of tests/test_pc_paths_gpu.py end to end ---------------------------------------------------------------------
# Level steps in front of an AGC make the END-TO-END comparison sensitive where no steady carrier is: in the burst in which the
# decay average first lies above the peak of a low step (0.2 s into the stream), the ORACLE chain run on its own filter output
# disturbed like an fp32 filter's (oracle CDemodulator.perturb_filter_output: additive noise of 3e-7 of the largest filter
# input, or the same floor as a grid of 1e-8 -- the measurement behind tests/startup_bounds.py) differs from the undisturbed run
# by the figures below, and forgets it with the decay time constant.  They are the per-burst spread of the oracle against ITSELF,
# maximum over six seeds and both disturbances, in units of full scale, rounded up, for the bursts where twice the spread
# (startup_bounds.FACTOR) lies above the chain rule's steady bound; tests/test_pc_paths_host.py reproduces them and holds every
# other burst's spread under half the steady bound, so the chain rule applies there unchanged.  {mode: {burst of the stream: spread}}
CHAIN_STEP_SPREAD = {"AM": {6: 1.2e-4, 7: 4.1e-5, 8: 4.0e-5, 9: 2.3e-5, 10: 1.7e-5, 11: 1.2e-5},
                     "SAM": {6: 1.1e-4, 7: 4.1e-5, 8: 3.6e-5, 9: 2.3e-5, 10: 1.7e-5, 11: 1.2e-5},
                     "CWU": {3: 5.2e-5, 4: 3.9e-5, 5: 1.7e-5, 6: 1.2e-5}}
