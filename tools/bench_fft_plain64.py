#!/usr/bin/env python3
"""Timing of the fp64 batch plain transforms (csdr_fft_batch_fwd_f64, fft_batch_plain64_kernels.hip) -- not the bench.py
contract.

For every size 512 ... 65536: 256 rows x (2^18 / n) frames of complex fp64 (1 GiB in, 1 GiB out), forward, out of place
and in place.  HIP events around every call after warm-up, medians, the legs alternating in one process:
  "fwd"      csdr_fft_batch_fwd_f64, d_out another buffer
  "inplace"  csdr_fft_batch_fwd_f64, d_out == d_in
  "copy"     a device-to-device copy of the same input + output bytes
  "fp32"     csdr_fft_batch_fwd of the same point count (complex fp32 rows of the same length: half the bytes)
and the bytes the fp64 transform must move (32 per point: 16 in, 16 out) over its time, against the 8 TB/s peak.

  python tools/bench_fft_plain64.py [--calls 30] [--rows 256] [--sizes 512,32768]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cutesdr_amd as ca

FS, PEAK = 2.0e6, 8.0e12
SIZES = (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)


def measure(rows, n, per_row, calls, warmup):
    nframes = per_row // n
    stream = torch.cuda.current_stream().cuda_stream
    f = ca.FftBatch(rows)
    f.set_params(n, False, 0.0, FS); f.set_ave(1)
    f.prepare64()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (3000.0 * torch.randn((rows, per_row, 2), generator=g, device="cuda", dtype=torch.float64)).contiguous()
    y = torch.empty_like(x)
    z = x.clone()                                            # the in-place leg's rows (they grow by n a call: re-filled)
    x32 = x.to(torch.float32).contiguous()
    y32 = torch.empty_like(x32)
    legs = {
        "fwd": lambda: f.fwd64_ptr(x.data_ptr(), per_row, y.data_ptr(), per_row, nframes, stream),
        "inplace": lambda: f.fwd64_ptr(z.data_ptr(), per_row, z.data_ptr(), per_row, nframes, stream),
        "copy": lambda: y.copy_(x),
        "fp32": lambda: f.fwd_ptr(x32.data_ptr(), per_row, y32.data_ptr(), per_row, nframes, stream),
    }
    times = {k: [] for k in legs}
    for it in range(warmup + calls):
        for name, call in legs.items():
            if name == "inplace":
                z.copy_(x)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    moved = 32.0 * rows * per_row
    out = {"n": n, "rows": rows, "frames": nframes, "bytes": moved, "group": f.plain_group64()}
    for k, v in times.items():
        out[k + "_ms"] = statistics.median(v)
        out[k + "_min_ms"] = min(v)
    for k in ("fwd", "inplace", "copy"):
        out[k + "_tbps"] = moved / (out[k + "_ms"] * 1e-3) / 1e12
        out[k + "_of_peak"] = moved / (out[k + "_ms"] * 1e-3) / PEAK
    out["fp32_tbps"] = 0.5 * moved / (out["fp32_ms"] * 1e-3) / 1e12
    out["fwd_over_copy"] = out["fwd_ms"] / out["copy_ms"]
    out["fwd_over_fp32"] = out["fwd_ms"] / out["fp32_ms"]
    out["fwd_us_per_frame"] = out["fwd_ms"] * 1e3 / (rows * nframes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--per-row", type=int, default=1 << 18)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    a = ap.parse_args()
    res = {}
    for n in (int(s) for s in a.sizes.split(",")):
        res[str(n)] = measure(a.rows, n, a.per_row, a.calls, a.warmup)
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bench_fft_plain64", "calls": a.calls, **res}))


if __name__ == "__main__":
    main()
