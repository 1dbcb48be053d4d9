"""The blanker's trace form (csdr_noiseproc_batch_trace_last, PROFILE_7) beside the call it traces, on one buffer.

256 receivers x 2^21 samples per call at 2 MS/s (the 10 001-sample window: the ring form), every blanker on; fp32 rows,
and 24-bit datagrams (8738 of 1444 bytes: 2 097 120 samples).  Device time per call with HIP events on one stream,
medians of --calls; the calls ALTERNATE in one process (one round = each of them once), so that drift of the box lands
on all of them alike:
  process      csdr_noiseproc_batch_process (rows) / the internal packets form: the sample form, blanked samples out
  trace_last   the trace of that call: the same loads and sums, 8 bytes out per sample, one fp64 division per sample
  memset       a device fill of the trace's bytes (zero_ of the tensor): what writing 8 bytes per sample costs alone
A diagnostic path: no threshold.  The payload is noise with a few impulses, so that both branches of the trace run.
Each input form is one step: a child process of its own under its own time limit (--step-timeout seconds); a step that
fails or runs out of time ends the run.  Prints one JSON line.
Usage: python tools/bench_nbtrace.py [--channels 256] [--log2n 21] [--calls 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def step(a, pkt):
    import torch
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__noiseproc_batch_process_packets.restype = C.c_int
    L.csdr__noiseproc_batch_process_packets.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    Cn, fs = a.channels, 2e6
    npk = (1 << a.log2n) // 240 if pkt else 0
    n = npk * 240 if pkt else 1 << a.log2n
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    g = torch.Generator(device=dev); g.manual_seed(7)
    if pkt:
        # random low bytes, the top byte of every 24-bit value 0 (|x| < 256 on the 16-bit scale) but for a few impulses
        src = torch.randint(0, 256, (Cn, npk, pkt), dtype=torch.uint8, device=dev, generator=g)
        top = src[:, :, 4:].view(Cn, npk, 480, 3)[..., 2]
        top.zero_()
        top[torch.rand((Cn, npk, 480), device=dev, generator=g) < 5e-5] = 0x60
    else:
        src = torch.randn((Cn, n, 2), dtype=torch.float32, device=dev, generator=g) * 1500.0
        src[torch.rand((Cn, n), device=dev, generator=g) < 5e-5] += 25000.0
    out = torch.empty((Cn, n, 2), dtype=torch.float32, device=dev)
    trace = torch.zeros((Cn, n, 2), dtype=torch.float32, device=dev)
    nb = ca.NoiseProcBatch(Cn)
    nb.setup(True, 30.0, 50.0, fs)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def process():
        if pkt:
            assert L.csdr__noiseproc_batch_process_packets(nb.h, C.c_void_p(src.data_ptr()), npk, pkt, C.c_void_p(out.data_ptr()), n, C.c_void_p(sp)) == 0, ca._capi.last_error()
        else:
            nb.process_ptr(src.data_ptr(), n, n, out.data_ptr(), n, sp)

    def trace_last():
        kw = dict(d_packets=src.data_ptr(), npackets=npk, pkt_len=pkt) if pkt else dict(d_in=src.data_ptr(), in_stride=n)
        assert nb.trace_last(trace.data_ptr(), n, n, stream=sp, **kw) == 0, ca._capi.last_error()

    calls = (("process", process), ("trace_last", trace_last), ("memset", lambda: trace.zero_()))
    ms = {k: [] for k, _ in calls}
    for i in range(a.warmup + a.calls):
        for name, fn in calls:
            t = timed(fn)
            if i >= a.warmup:
                ms[name].append(t)
    # what was timed did what it says: the trace of the last call blanks exactly where that call's output is zero
    process(); trace_last()
    torch.cuda.synchronize()
    d = 50 + 1                                           # delay_n + 1 at 50 us, 2 MS/s: width 100 samples
    zero = (out[0, d:, 0] == 0) & (out[0, d:, 1] == 0)
    assert bool(((trace[0, d:, 0] == 0) == zero).all()) and 0 < int(zero.sum()) < n - d
    tag = "pkt%d" % pkt if pkt else "rows"
    res = {"samples_%s" % tag: n}
    for name, v in ms.items():
        res["%s_%s_ms" % (name, tag)] = round(float(np.median(v)), 4)
        res["%s_%s_min_ms" % (name, tag)] = round(float(np.min(v)), 4)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", type=int, default=-1, help="(internal) run the one step of this input form: 0 rows, 1444 datagrams")
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.step >= 0:
        return step(a, a.step)
    out = {"tool": "bench_nbtrace", "channels": a.channels, "log2n": a.log2n, "calls": a.calls}
    for pkt in (0, 1444):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(pkt)] + \
            ["--%s=%d" % (k.replace("_", "-"), getattr(a, k)) for k in ("channels", "log2n", "calls", "warmup")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:
            sys.exit("bench_nbtrace: the step of input form %d ended with status %d; nothing more is started" % (pkt, r.returncode))
        out.update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
