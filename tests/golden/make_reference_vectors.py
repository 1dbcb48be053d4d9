#!/usr/bin/env python3
"""Writes tests/golden/reference_vectors.json: what the REFERENCE's own compiled code (oracle/ref.py) gives for a dozen
and a half seeded cases -- one per dsp/ class, and the whole chain in FM, AM, USB and CWU.  Runs only where the reference
library is available.  Per case the file holds the recipe (kind, parameters, generator and its arguments, call
pattern) and, of the output, the count, the first and last 32 fp64 words as exact hex, and the four digests of
oracle_regression.json plus rms / largest magnitude / largest value for scaling tolerances.  Data and recipes only.

run_case(module, case) replays a recipe on anything with the oracle's class names: oracle.oracle, oracle.ref, and the
library's own drop-in classes (cutesdr_amd).  tests/test_oracle_anchors.py and tests/test_golden_gpu.py use it."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")):
    if os.path.abspath(p) not in [os.path.abspath(q) for q in sys.path]:
        sys.path.insert(0, os.path.abspath(p))
from util_signals import tones_plus_noise, fm_carrier, am_carrier          # noqa: E402
import test_postchain_gpu as T                                             # noqa: E402
from test_frontend_gpu import impulsive                                    # noqa: E402

OUT = os.path.join(HERE, "reference_vectors.json")
WORDS = 32


def _normal(seed, n, scale=1000.0):
    rng = np.random.default_rng(seed)
    return scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


GENERATORS = {
    "tones_plus_noise": tones_plus_noise, "fm_carrier": fm_carrier, "am_carrier": am_carrier, "impulsive": impulsive,
    "level_steps": T.level_steps, "chain_input": T.make_input, "normal": _normal,
    "sine": lambda n, w, amp: amp * np.sin(w * np.arange(n)),
}


def make_input(case):
    x = GENERATORS[case["gen"]](**case["gen_args"])
    return x.real.copy() if case.get("real_part") else x


def _calls(x, lengths):
    pos = 0
    for n in lengths:
        yield x[pos:pos + n]
        pos += n
    assert pos == len(x), (pos, len(x))


def _info(mod, mode):
    m, kw = T.MODES[mode]
    return m, T.info(mod, **kw)


def run_case(mod, case):
    """the case's output as one flat fp64 vector (complex outputs as interleaved re, im)"""
    k, p, x = case["kind"], case.get("params", {}), make_input(case)
    parts = lambda f: np.concatenate([np.asarray(f(c)) for c in _calls(x, case["calls"])])
    if k == "downconvert":
        o = mod.CDownConvert(); o.SetDataRate(p["rate"], p["bw"]); o.SetFrequency(p["freq"])
        y = parts(o.ProcessData)
    elif k == "fastfir":
        o = mod.CFastFIR(2048); o.SetupParameters(p["lo"], p["hi"], p["offset"], p["fs"])
        y = parts(o.ProcessData)
    elif k == "display":
        o = mod.CFft(); o.SetFFTParams(p["n"], False, 0.0, p["fs"]); o.SetFFTAve(p["ave"])
        for c in _calls(x, case["calls"]):
            o.PutInDisplayFFT(c)
        y = np.asarray(o.ave_buf(), dtype=np.float64)
    elif k == "fft":
        o = mod.CFft(); o.SetFFTParams(len(x), False, 0.0, 1.0)
        y = o.FwdFFT(x)
    elif k == "fir":
        o = mod.CFir(); o.InitLPFilter(*p["lp"])
        y = parts(o.ProcessFilter)
    elif k == "iir":
        o = mod.CIir(); o.Init(*p["init"])
        y = parts(o.ProcessFilter)
    elif k == "agc":
        o = mod.CAgc(); o.SetParameters(*p["set"])
        y = parts(o.ProcessData)
    elif k == "smeter":
        o = mod.CSMeter()
        for c in _calls(x, case["calls"]):
            o.ProcessData(c, p["fs"])
        y = np.array([o.GetAve(), o.GetPeak(), o.GetPeak()])
    elif k in ("am", "sam", "fm"):
        o = {"am": mod.CAmDemod, "sam": mod.CSamDemod, "fm": mod.CFmDemod}[k](p["fs"])
        if k == "am":
            o.SetBandwidth(p["bw"]); y = parts(o.ProcessData)
        elif k == "sam":
            y = parts(o.ProcessData)
        else:
            o.SetSquelch(p["squelch"]); y = parts(lambda c: o.ProcessData(c, p["fm_bw"]))
    elif k == "ssb":
        y = mod.ssb_demod(x)
    elif k == "resampler":
        o = mod.CFractResampler(); o.Init(p["init"])
        y = parts(lambda c: o.Resample(c, p["rate"]))
    elif k == "blanker":
        o = mod.CNoiseProc(); o.SetupBlanker(True, p["thresh"], p["width"], p["fs"])
        y = parts(o.ProcessBlanker)
    elif k == "chain":
        o = mod.CDemodulator(2048)
        m, inf = _info(mod, p["mode"])
        o.SetInputSampleRate(p["fs"]); o.SetDemod(m, inf); o.SetDemodFreq(p["freq"])
        y = parts(o.process_append)
    else:
        raise KeyError(k)
    y = np.ascontiguousarray(y)
    return y.astype(np.complex128).view(np.float64) if np.iscomplexobj(y) else y.astype(np.float64)


def digest(v):
    w = np.cos(0.37 * np.arange(len(v)))                        # position-sensitive, as in make_oracle_regression.py
    return {"n": int(len(v)), "sum": float(v.sum()), "abs": float(np.abs(v).sum()), "dot": float((v * w).sum())}


def describe(v):
    d = digest(v)
    d.update(first=[float(a).hex() for a in v[:WORDS]], last=[float(a).hex() for a in v[-WORDS:]],
             rms=float(np.sqrt(np.mean(v * v))), maxabs=float(np.abs(v).max()), max=float(v.max()))
    return d


def _chain(mode, n):
    fs = 2e6
    return dict(kind="chain", params=dict(mode=mode, fs=fs, freq=-100e3), gen="chain_input", gen_args=dict(mode=mode, n=n, fs=fs),
                calls=[3328] * (n // 3328))


CASES = {
    "downconvert_2M_15k": dict(kind="downconvert", params=dict(rate=2e6, bw=15000.0, freq=-100e3), gen="tones_plus_noise",
                               gen_args=dict(channel=6, n=3 * 8192, fs=2e6, tones_hz=[100e3 + 500.0]), calls=[8192] * 3),
    "fastfir_usb": dict(kind="fastfir", params=dict(lo=100.0, hi=2800.0, offset=0.0, fs=62500.0), gen="tones_plus_noise",
                        gen_args=dict(channel=5, n=7 * 1024, fs=62500.0, tones_hz=[1000.0, 20000.0]), calls=[1000, 2048, 4120]),
    "display_4096_ave3": dict(kind="display", params=dict(n=4096, fs=2e6, ave=3), gen="tones_plus_noise",
                              gen_args=dict(channel=7, n=5 * 4096, fs=2e6, tones_hz=[250e3]), calls=[4096] * 5),
    "fwd_fft_2048": dict(kind="fft", gen="normal", gen_args=dict(seed=2048, n=2048)),
    "fir_lowpass": dict(kind="fir", params=dict(lp=[1.0, 50.0, 5000.0, 9000.0, 31250.0]), gen="normal", gen_args=dict(seed=1, n=3000),
                        real_part=True, calls=[1000, 2000]),
    "iir_bandpass": dict(kind="iir", params=dict(init=["BP", 700.0, 5.0, 15625.0]), gen="normal", gen_args=dict(seed=2, n=4000), calls=[4000]),
    "agc_hang": dict(kind="agc", params=dict(set=[True, True, -60, 30, 5, 300, 62500.0]), gen="level_steps",
                     gen_args=dict(n=40000, fs=62500.0, seed=3), calls=[8192, 31808]),
    "smeter": dict(kind="smeter", params=dict(fs=62500.0), gen="level_steps", gen_args=dict(n=40000, fs=62500.0, seed=4), calls=[8192, 31808]),
    "am_leaf": dict(kind="am", params=dict(fs=31250.0, bw=4000.0), gen="am_carrier",
                    gen_args=dict(n=8192, fs=31250.0, fc=150.0, fmod=800.0, depth=0.6, dbfs=-12.0), calls=[1024] * 8),
    "sam_leaf": dict(kind="sam", params=dict(fs=31250.0), gen="am_carrier",
                     gen_args=dict(n=8192, fs=31250.0, fc=150.0, fmod=800.0, depth=0.6, dbfs=-12.0), calls=[1024] * 8),
    "fm_leaf": dict(kind="fm", params=dict(fs=62500.0, squelch=50, fm_bw=5000.0), gen="fm_carrier",
                    gen_args=dict(n=16384, fs=62500.0, fc=300.0, fmod=1000.0, dev=3000.0, dbfs=-6.0, noise_dbfs=-60.0), calls=[1024] * 16),
    "ssb": dict(kind="ssb", gen="normal", gen_args=dict(seed=9, n=100)),
    "resampler_real": dict(kind="resampler", params=dict(init=8192, rate=1.6276), gen="sine", gen_args=dict(n=6000, w=0.01, amp=8000.0), calls=[2048, 2048, 1904]),
    "blanker": dict(kind="blanker", params=dict(thresh=40.0, width=10.0, fs=2e6), gen="impulsive", gen_args=dict(seed=9, n=60000, fs=2e6),
                    calls=[240, 4096, 1, 4095] + [4096] * 12 + [2416]),
    "chain_FM": _chain("FM", 3328 * 197),                    # 20 bursts: the last words lie behind the PLL's start-up
    "chain_AM": _chain("AM", 3328 * 120),
    "chain_USB": _chain("USB", 3328 * 60),
    "chain_CWU": _chain("CWU", 3328 * 160),
}


def build():
    from oracle import ref
    assert ref.available(), "needs oracle/_ref/libcutesdr_ref.so (built where the reference tree is)"
    return {name: dict(case, expect=describe(run_case(ref, case))) for name, case in CASES.items()}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(build(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", os.path.getsize(OUT), "bytes")
