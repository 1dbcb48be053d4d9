#!/usr/bin/env python3
"""Timing of the batch test-bench scope (csdr_scope_batch, K10) -- not the bench.py contract.

Shapes: one audio call (256 receivers x 8192 fp32 samples at 48 kHz, put_real) and BASELINE config C4's per-GPU share
(256 receivers x 2^21 complex samples at 2 MHz, put_cpx), screen 100 x 100, span 100 ms, PNORM.  Two states each:
"wait": the level is never reached, so every emission of the call is compared (the worst case: the scope reads the
emitted samples only, 100 per sweep, not the stream); "trigger": re-armed before every call with a crossing in the
first sweep, so a screen is gathered per call.  HIP events around every call after warm-up, in the same process and
alternating with a device-to-host copy of the same rows into pinned memory -- the yardstick: the least a host without
the scope must spend before it can run the reference's loop at all, and not the code under test.  Also the host time
of one put (settings + launch).

  python tools/bench_scope.py [--calls 30] [--copies 5] [--channels 256]
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cutesdr_amd as ca

SHAPES = {"audio_real": (8192, 48000.0, False), "c4_cpx": (1 << 21, 2.0e6, True)}


def rows_for(channels, n, cpx):
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    re = (3000.0 * torch.sin(2.0 * math.pi * 0.0137 * i)).to(torch.float32)
    if not cpx:
        return re.repeat(channels, 1).contiguous()
    im = (3000.0 * torch.cos(2.0 * math.pi * 0.0137 * i)).to(torch.float32)
    return torch.complex(re, im).repeat(channels, 1).contiguous()


def measure(channels, n, fs, cpx, calls, copies, warmup):
    rows = rows_for(channels, n, cpx)
    nbytes = rows.numel() * rows.element_size()
    host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
    out = {"channels": channels, "n": n, "bytes": nbytes, "sample_rate": fs}
    scopes = {}
    for name, level in (("wait", 2000000000), ("trigger", 100)):
        s = ca.ScopeBatch(channels)
        s.OnTriggerMode(s.TRIG_PNORM); s.OnTrigLevel(level)
        s.DisplayData(rows, n, fs)                       # the first call carries the rate and is dropped
        scopes[name] = s
    times = {k: [] for k in list(scopes) + ["d2h"]}
    hostt = {k: [] for k in scopes}
    emits = {k: 0 for k in scopes}
    for it in range(warmup + calls):
        for name in ("d2h", "wait", "trigger"):
            if name == "d2h" and it >= warmup + copies:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "d2h":
                host.copy_(rows, non_blocking=True)
            else:
                s = scopes[name]
                t0 = time.perf_counter()
                s.time_plot_done()
                s.DisplayData(rows, n, fs)
                hostt[name].append(time.perf_counter() - t0)
            b.record()
            b.synchronize()
            shown = int(scopes[name].get_emits().sum()) if name != "d2h" else 0
            if it >= warmup:
                times[name].append(a.elapsed_time(b) * 1e-3)
                emits[name] = emits.get(name, 0) + shown
    d2h = statistics.median(times["d2h"])
    out["d2h_ms"] = d2h * 1e3
    out["d2h_gbs"] = nbytes / d2h * 1e-9
    for k in scopes:
        t = statistics.median(times[k])
        out[k + "_ms"] = t * 1e3
        out[k + "_min_ms"] = min(times[k]) * 1e3
        out[k + "_d2h_over_put"] = d2h / t
        out[k + "_host_us"] = statistics.median(hostt[k][warmup:]) * 1e6
        out[k + "_screens_per_call"] = emits[k] / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--copies", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=256)
    a = ap.parse_args()
    res = {k: measure(a.channels, n, fs, cpx, a.calls, a.copies, a.warmup) for k, (n, fs, cpx) in SHAPES.items()}
    print(json.dumps({"tool": "bench_scope", "calls": a.calls, **res}))


if __name__ == "__main__":
    main()
