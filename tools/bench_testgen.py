#!/usr/bin/env python3
"""Timing of the batch signal generator (csdr_testgen_batch, K9) -- not the bench.py contract.

Shapes: BASELINE config C4's per-GPU share (256 receivers x 2^21 complex samples, 4.3 GB written) and 2048-sample
rows (the overhead end).  All generators on: a third constant tones, a third sweeping, a third pulsed; noise off and
noise on (-70 dB) as two figures.  HIP events around every call after warm-up, in the same process and alternating
with a hipMemsetAsync of the same bytes -- the yardstick: the cheapest way the machine writes those bytes, and not
the code under test.  Also the host time of one generate call (state advance + launch), which must not grow with n.

  python tools/bench_testgen.py [--calls 50] [--channels 256] [--once SHAPE]
--once: a single noise-off / noise-on pair of calls at SHAPE (c4 or small), for a kernel trace of its own.
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cutesdr_amd as ca

FS = 2.0e6
PEAK_GBS = 8000.0                        # MI355X HBM3E


def make(channels, noise_db):
    g = ca.TestGenBatch(channels)
    g.OnGenOn(True); g.OnSignalPwr(-20.0); g.OnNoisePwr(noise_db); g.OnPulseWidth(0.0)
    for c in range(channels):
        f = 100e3 + 500.0 * c
        if c % 3 == 0:
            g.OnSweepStart(f, channel=c); g.OnSweepStop(f, channel=c)
        elif c % 3 == 1:                 # sweeps for the whole run
            g.OnSweepStart(-400e3 + 100.0 * c, channel=c); g.OnSweepStop(900e3, channel=c); g.OnSweepRate(2000.0, channel=c)
        else:
            g.OnSweepStart(-f, channel=c); g.OnSweepStop(-f, channel=c)
            g.OnPulseWidth(0.001, channel=c); g.OnPulsePeriod(0.1, channel=c)
    return g


def measure(hip, channels, n, calls, warmup):
    rows = torch.empty((channels, n), dtype=torch.complex64, device="cuda")
    nbytes = rows.numel() * 8
    stream = torch.cuda.current_stream().cuda_stream
    out = {"channels": channels, "n": n, "bytes": nbytes}
    gens = {"noise_off": make(channels, -160.0), "noise_on": make(channels, -70.0)}
    times = {k: [] for k in list(gens) + ["memset"]}
    host = {k: [] for k in gens}
    for it in range(warmup + calls):
        for name in ("memset", "noise_off", "memset", "noise_on"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "memset":
                rc = hip.hipMemsetAsync(ctypes.c_void_p(rows.data_ptr()), 0, ctypes.c_size_t(nbytes), ctypes.c_void_p(stream))
                assert rc == 0, rc
            else:
                t0 = time.perf_counter()
                gens[name].CreateGeneratorSamples(rows, n, FS)
                host[name].append(time.perf_counter() - t0)
            b.record()
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b) * 1e-3)
    ms = statistics.median(times["memset"])
    out["memset_ms"] = ms * 1e3
    out["memset_gbs"] = nbytes / ms * 1e-9
    for k in gens:
        t = statistics.median(times[k])
        out[k + "_ms"] = t * 1e3
        out[k + "_gbs"] = nbytes / t * 1e-9
        out[k + "_of_peak"] = nbytes / t * 1e-9 / PEAK_GBS
        out[k + "_over_memset"] = t / ms
        out[k + "_host_us"] = statistics.median(host[k][warmup:]) * 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--once", choices=["c4", "small"])
    a = ap.parse_args()
    hip = ctypes.CDLL("libamdhip64.so")
    shapes = {"c4": 1 << 21, "small": 2048}
    if a.once:
        res = {a.once: measure(hip, a.channels, shapes[a.once], 1, 1)}
    else:
        res = {k: measure(hip, a.channels, n, a.calls, a.warmup) for k, n in shapes.items()}
    print(json.dumps({"tool": "bench_testgen", "calls": a.calls, **res}))


if __name__ == "__main__":
    main()
