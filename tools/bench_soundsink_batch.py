"""Batch sound sink against a loop of single sinks: 256 receivers spread over three output rates, 20 ms blocks.

Times csdr_soundsink_batch_put (one launch for every receiver; HIP-event device time on the caller's stream and wall
time per put) and, fed the same rows, a loop of 256 csdr_soundsink_put calls (rows copied to the host and widened to
doubles first, as such a host has to).  Every sound card pops what a put brought, so the queues stay steady.
Prints one JSON line.  Usage: python tools/bench_soundsink_batch.py [--channels 256] [--puts 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--puts", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-puts", type=int, default=20)
    ap.add_argument("--stereo", action="store_true")
    a = ap.parse_args()
    import torch
    import cutesdr_amd as ca
    C, block = a.channels, 0.02
    rates = np.array([62500.0, 31250.0, 15625.0])[np.arange(C) % 3]
    counts = np.array([int(r * block) for r in rates], dtype=np.int32)
    T = int(counts.max())
    dev = torch.device("cuda:0")
    k = torch.arange(T, device=dev, dtype=torch.float64)
    f = torch.tensor(600.0 + 5.0 * np.arange(C), device=dev, dtype=torch.float64)[:, None]
    ph = 2 * np.pi * f * k[None, :] / torch.tensor(rates, device=dev)[:, None]
    rows = (9000.0 * torch.sin(ph)).float().contiguous()
    if a.stereo:
        rows = torch.complex(rows, (9000.0 * torch.cos(ph)).float()).contiguous()
    sink = ca.SoundSinkBatch(C, a.stereo)
    for c in range(C):
        sink.ChangeUserDataRate(c, float(rates[c]))
    sink.SetVolume(-1, 90)
    stream = torch.cuda.current_stream(dev)
    pop = int(48000 * block)

    def drain():
        for c in range(C):
            sink.GetOutQueue(c, pop)
    for _ in range(a.warmup):
        sink.PutOutQueue(rows, counts)
        drain()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(a.puts):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        sink.PutOutQueue(rows, counts)
        t1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
        wall_ms.append((t1 - t0) * 1e3)
        drain()
    singles = [ca.CSoundOut(a.stereo) for _ in range(C)]
    for c in range(C):
        singles[c].ChangeUserDataRate(float(rates[c]))
        singles[c].SetVolume(90)
    loop_ms, loop_put_ms = [], []
    for i in range(a.warmup + a.loop_puts):
        t0 = time.perf_counter()
        host = rows.cpu().numpy()                                   # the rows copied back to the host
        t1 = time.perf_counter()
        for c in range(C):
            singles[c].PutOutQueue(host[c, :counts[c]])             # widened to doubles, one resample + wait each
        t2 = time.perf_counter()
        if i >= a.warmup:
            loop_ms.append((t2 - t0) * 1e3)
            loop_put_ms.append((t2 - t1) * 1e3)
        for c in range(C):
            singles[c].GetOutQueue(pop)
    med = lambda v: float(np.median(v))                            # noqa: E731
    print(json.dumps({"tool": "bench_soundsink_batch", "channels": C, "stereo": a.stereo, "block_ms": block * 1e3,
                      "rates": [62500.0, 31250.0, 15625.0], "batch_put_device_ms": round(med(dev_ms), 4),
                      "batch_put_wall_ms": round(med(wall_ms), 4), "batch_put_wall_p90_ms": round(float(np.percentile(wall_ms, 90)), 4),
                      "loop_wall_ms": round(med(loop_ms), 3), "loop_put_only_ms": round(med(loop_put_ms), 3),
                      "speedup_wall": round(med(loop_ms) / med(wall_ms), 1), "puts": a.puts, "loop_puts": a.loop_puts}))


if __name__ == "__main__":
    main()
