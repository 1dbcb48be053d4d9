#!/usr/bin/env python3
"""Timing of the FFT view of the batch test-bench scope (csdr_scope_batch after OnTimeDisplay(False), K10) -- not the
bench.py contract.

Shapes: 256 receivers x 65 536 real samples at 62.5 kS/s (skip value 3: 32 frames a call, 10 or 11 of them used) and
256 x 2^21 complex samples at 2 MS/s (display rate 10, skip value 97: 1024 frames a call, 10 or 11 used), screen
700 x 255.  HIP events around every put after warm-up, in the same process and alternating with two yardsticks:
  "compose": what the library could do for the same used frames without the view -- FftBatch(2048 points, average 1)
             .put_display on each used frame (one launch for all receivers) plus one get_screen_all per frame; it leaves
             out the carry, the per-receiver frame logic and the peak hold (a read-back per frame).  FftBatch takes
             complex rows only, so for the real shape it runs on a complex copy of the rows made beforehand;
  "d2h":     the device-to-host copy of the same rows into pinned memory, the least a host that runs the reference's
             loop itself must spend.
Also the host time of one put (settings, plan, launches).

  python tools/bench_scope_fft.py [--calls 20] [--copies 5] [--channels 256]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cutesdr_amd as ca
from cutesdr_amd._capi import lib, check

SHAPES = {"real_62k5": (1 << 16, 62500.0, False), "cpx_2M": (1 << 21, 2.0e6, True)}
W, H, N = 700, 255, 2048


def rows_for(channels, n, cpx):
    g = torch.Generator(device="cuda").manual_seed(1)
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    tone = 3276.7 * torch.exp(2j * torch.pi * 0.1317 * i)
    x = tone.repeat(channels, 1) + 327.67 * torch.complex(torch.randn((channels, n), generator=g, device="cuda", dtype=torch.float64),
                                                          torch.randn((channels, n), generator=g, device="cuda", dtype=torch.float64))
    x = x.to(torch.complex64).contiguous()
    return (x if cpx else x.real.contiguous()), x


def measure(channels, n, fs, cpx, calls, copies, warmup):
    rows, crows = rows_for(channels, n, cpx)
    nbytes = rows.numel() * rows.element_size()
    host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
    s = ca.ScopeBatch(channels)
    s.resizeEvent(W, H); s.OnTimeDisplay(False); s.OnDisplayRate(10)
    s.DisplayData(rows, n, fs)                           # the first call carries the rate and is dropped
    skip = int(fs / (N * 10))
    step = max(skip, 1)
    f = ca.FftBatch(channels)
    f.set_params(N, False, 0.0, fs); f.set_ave(1)
    scr = torch.zeros((channels, W), dtype=torch.int32, device="cuda")
    ov = torch.zeros(channels, dtype=torch.int32, device="cuda")
    span = int(fs) - (int(fs) + 5) % 10 + 5
    stream = torch.cuda.current_stream().cuda_stream

    def compose(used):
        for k in range(used):
            f.put_display_ptr(crows.data_ptr() + 8 * (k * step * N), crows.stride(0), 1, stream)
            check(lib().csdr_fft_batch_get_screen_all(f.h, H, W, 10.0, -170.0, -(span // 2) if cpx else 0, span // 2,
                                                      C.c_void_p(scr.data_ptr()), W, C.c_void_p(ov.data_ptr()), C.c_void_p(stream)),
                  "csdr_fft_batch_get_screen_all")

    times, hostt, frames = {"put": [], "compose": [], "d2h": []}, [], []
    for it in range(warmup + calls):
        used = 0
        for name in ("d2h", "put", "compose"):
            if name == "d2h" and it >= warmup + copies:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "d2h":
                host.copy_(rows, non_blocking=True)
            elif name == "put":
                t0 = time.perf_counter()
                s.DisplayData(rows, n, fs)
                dt = time.perf_counter() - t0
            else:
                compose(used)
            b.record()
            b.synchronize()
            if name == "put":
                used = int(s.get_emits()[0])
                if it >= warmup:
                    hostt.append(dt); frames.append(used)
            if it >= warmup:
                times[name].append(a.elapsed_time(b) * 1e-3)
    out = {"channels": channels, "n": n, "bytes": nbytes, "sample_rate": fs, "skip": skip,
           "used_frames_per_call": statistics.mean(frames)}
    for k, v in times.items():
        out[k + "_ms"] = statistics.median(v) * 1e3
        out[k + "_min_ms"] = min(v) * 1e3
    out["put_host_us"] = statistics.median(hostt) * 1e6
    out["compose_over_put"] = out["compose_ms"] / out["put_ms"]
    out["d2h_over_put"] = out["d2h_ms"] / out["put_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--copies", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, default=256)
    a = ap.parse_args()
    res = {k: measure(a.channels, n, fs, cpx, a.calls, a.copies, a.warmup) for k, (n, fs, cpx) in SHAPES.items()}
    print(json.dumps({"tool": "bench_scope_fft", "calls": a.calls, **res}))


if __name__ == "__main__":
    main()
