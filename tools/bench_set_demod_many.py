"""What new filter edges for every receiver cost, per step: a loop of csdr_demod_batch_set_demod calls (leg a: filters
designed on the caller's thread) against one csdr_demod_batch_set_demod_many (leg b: designed on the device).

A pipelined batch of 256 mixed AM / FM / USB receivers at 2 MS/s as bench.py's control_plane leg builds it; in front of
every step every receiver of the chosen subset gets new edges (same mode).  Legs plain / a / b run interleaved, `--rounds`
times each, in one process on one object; reported per leg and subset: the caller's time per step (host clock around the
setter calls alone), the step time (host clock around `--steps` steps ending in a device synchronise) and its increase
over untouched steps.  Subsets: all receivers, the FM and USB receivers, the AM receivers (whose Kaiser low-pass is still
designed on the host per entry).  Asserts what the feature is for: on the FM and USB receivers leg b's caller time is at
most half of leg a's, and leg b's step-time increase is below leg a's.  Prints one JSON line.

The design launch's own time: run `--legs b --rounds 1` under `rocprofv3 --kernel-trace --stats` in a run of its own and
read fastfir_design_kernel's row.

Usage: python tools/bench_set_demod_many.py [--channels 256] [--steps 12] [--rounds 5] [--legs ab] [--no-assert]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FS, T = 2.0e6, 1 << 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--no-assert", action="store_true")
    a = ap.parse_args()
    import torch
    import cutesdr_amd as ca
    C_ = a.channels
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC0DE0000)
    x = torch.randn((C_, T, 2), generator=g, device=dev, dtype=torch.float32) * (32767.0 * 10 ** (-70 / 20))
    t = torch.arange(T, device=dev, dtype=torch.float64) / FS
    for c in range(C_):                                     # a carrier per receiver (the S-meters and AGCs see a station)
        ph = 2 * torch.pi * (100e3 + 500.0 * (c % 1024)) * t
        x[c, :, 0] += (3276.7 * torch.cos(ph)).float(); x[c, :, 1] += (3276.7 * torch.sin(ph)).float()
    del t
    base = dict(HiCut=5000, HiCutmin=5000, HiCutmax=15000, LowCut=-5000, LowCutmin=-15000, LowCutmax=-5000,
                FilterClickResolution=100, Offset=0, SquelchValue=0, AgcSlope=0, AgcThresh=-100,
                AgcManualGain=30, AgcDecay=200, AgcOn=1, AgcHangOn=0, Symetric=1)
    modes = [(ca.DEMOD_AM, dict(HiCutmin=500, HiCutmax=10000, LowCutmax=-500, LowCutmin=-10000)),
             (ca.DEMOD_FM, dict()),
             (ca.DEMOD_USB, dict(HiCut=2800, LowCut=100, HiCutmin=500, HiCutmax=20000, LowCutmax=200, LowCutmin=0, Symetric=0))]
    b = ca.DemodBatch(C_, 2048)
    b.set_input_rate(FS)
    for c in range(C_):
        m, kw = modes[c % 3]
        b.set_demod(c, m, ca.DemodInfo(**dict(base, **kw)))
    b.commit()
    for c in range(C_):
        b.set_freq(c, -(100e3 + 500.0 * (c % 1024)))
    b.set_pipelined(True)
    cap = T // 16 + 4096
    aud = torch.zeros((C_, cap), device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    subsets = {"all": list(range(C_)), "fm_usb": [c for c in range(C_) if c % 3], "am": [c for c in range(C_) if c % 3 == 0]}
    # the entries of both parities of a step, built once: both legs pay the same marshalling
    entries = {}
    for name, chans in subsets.items():
        for par in (0, 1):
            infos = []
            for c in chans:
                m, kw = modes[c % 3]
                kw = dict(base, **kw)
                kw["HiCut"] = kw["HiCut"] - 100 * (1 + par)
                infos.append(ca.DemodInfo(**kw))
            entries[name, par] = (np.asarray(chans, dtype=np.int32), np.asarray([modes[c % 3][0] for c in chans], dtype=np.int32),
                                  infos, (ca.DemodInfo * len(chans))(*infos))

    def step():
        b.process_ptr(x.data_ptr(), T, T, aud.data_ptr(), cap, stream)

    def run(leg, subset):
        for _ in range(3):
            step()
        b.flush(stream); torch.cuda.synchronize()
        host, t0 = 0.0, time.perf_counter()
        for k in range(a.steps):
            if leg != "plain":
                ch, md, infos, arr = entries[subset, k % 2]
                h0 = time.perf_counter()
                if leg == "a":
                    for i in range(len(ch)):
                        b.set_demod(int(ch[i]), int(md[i]), infos[i])
                else:
                    b.set_demod_many(ch, md, arr)
                host += time.perf_counter() - h0
            step()
        b.flush(stream); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, host / a.steps * 1e3

    for leg in a.legs:                                     # warm-up: every shape and path once (first use allocates)
        run(leg, "all")
    res = {}
    for _ in range(a.rounds):
        for leg, subset in [("plain", "all")] + [(leg, s) for s in subsets for leg in a.legs]:
            res.setdefault((leg, subset), []).append(run(leg, subset))
    med = lambda v: float(np.median(v))                    # noqa: E731
    plain = med([r[0] for r in res["plain", "all"]])
    out = {"tool": "bench_set_demod_many", "channels": C_, "steps": a.steps, "rounds": a.rounds, "ms_per_step_plain": round(plain, 4)}
    for (leg, subset), v in res.items():
        if leg == "plain":
            continue
        out["%s_%s" % (leg, subset)] = {"receivers": len(subsets[subset]), "caller_ms_per_step": round(med([r[1] for r in v]), 4),
                                        "caller_ms_min_max": [round(min(r[1] for r in v), 4), round(max(r[1] for r in v), 4)],
                                        "ms_per_step": round(med([r[0] for r in v]), 4),
                                        "step_increase_ms": round(med([r[0] for r in v]) - plain, 4)}
    if "a" in a.legs and "b" in a.legs:
        out["caller_ratio_b_over_a_fm_usb"] = round(out["b_fm_usb"]["caller_ms_per_step"] / out["a_fm_usb"]["caller_ms_per_step"], 4)
        out["caller_under_1ms_for_all"] = bool(out["b_all"]["caller_ms_per_step"] <= 1.0)
    print(json.dumps(out))
    if "a" in a.legs and "b" in a.legs and not a.no_assert:
        assert out["b_fm_usb"]["caller_ms_per_step"] <= 0.5 * out["a_fm_usb"]["caller_ms_per_step"], "caller time"
        assert out["b_all"]["step_increase_ms"] < out["a_all"]["step_increase_ms"], "step-time increase"


if __name__ == "__main__":
    main()
