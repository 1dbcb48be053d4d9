"""Display stream behind the fused noise blanker against the two-pass workaround and the unblanked display.

256 channels x 2185 24-bit datagrams (524400 samples) per call, 4096 points, average 1, blanker on, at display skip
values 1 and 48 (SetMaxDisplayRate: 48 is 2 MS/s, 4096 points, 10 updates/s).  Device time per call with HIP events on
one stream, medians:
  blanked          csdr_fft_batch_put_display_packets_blanked behind csdr_demod_batch_process_packets(nb) -- the display
                   call ALONE is timed (the chain call in front of it is the host's anyway)
  blanked_gather   the same call with the frame loaders off (CSDR_DISPLAY_BLANKED_LOADERS=0: every used frame gathered)
  workaround       csdr_ingest_unpack + csdr_noiseproc_batch_process + csdr_fft_batch_put_display_stream(dc): what a host
                   with the blanker on had to run for a blanked display before
  packets          csdr_fft_batch_put_display_packets(dc), unblanked
The chain is there to leave a mask: FM / AM receivers at a 500 kHz input rate (their decimation, 8 and 16, divides the
call's 524400 samples; the display does not see the chain's rate).  Each step is a child process of its own under a time
limit; the first one that fails ends the run.  Prints one JSON line.
Usage: python tools/bench_display_blanked.py [--channels 256] [--calls 30] [--warmup 5] [--limit 240]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
STEPS = [(form, skip) for skip in (1, 48) for form in ("blanked", "blanked_gather", "workaround", "packets")]


def step(a, form, skip):
    import torch
    import cutesdr_amd as ca
    L = ca.lib()
    Cn, npk, N, pkt = a.channels, a.npackets, a.size, 1444
    n = npk * 240
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    # noise at -30 dBFS with an impulse every ~20000 samples: the blanker triggers, as in the chain's own benchmark
    v = (torch.randn((Cn, npk, 480), device=dev, generator=g) * 1000.0 * 256.0)
    v[torch.rand((Cn, npk, 480), device=dev, generator=g) < 2.5e-5] += 25000.0 * 256.0
    v = v.round().clamp(-(1 << 23), (1 << 23) - 1).to(torch.int32)
    packets = torch.zeros((Cn, npk, pkt), dtype=torch.uint8, device=dev)
    packets[:, :, 4:] = torch.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], dim=-1).to(torch.uint8).reshape(Cn, npk, 1440)
    del v
    dc = torch.tensor([[3.5, -1.25]] * Cn, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    f = ca.FftBatch(Cn)
    f.set_params(N, False, 0.0, 2e6); f.set_ave(1)
    f.set_display_rate(N * 10 * skip + 1.0, 10)
    nb = ca.NoiseProcBatch(Cn); nb.setup(True, 50.0, 2.0, 2e6)
    before = None
    if form in ("blanked", "blanked_gather"):
        b = ca.DemodBatch(Cn, 2048); b.set_input_rate(500e3)
        base = dict(HiCut=5000, HiCutmin=5000, HiCutmax=15000, LowCut=-5000, LowCutmin=-15000, LowCutmax=-5000,
                    FilterClickResolution=100, Offset=0, SquelchValue=0, AgcSlope=0, AgcThresh=-100, AgcManualGain=30,
                    AgcDecay=200, AgcOn=1, AgcHangOn=0, Symetric=1)
        am = dict(base, HiCutmin=500, HiCutmax=10000, LowCutmax=-500, LowCutmin=-10000)
        for c in range(Cn):
            b.set_demod(c, 0 if c % 2 else 2, ca.DemodInfo(**(am if c % 2 else base)))
        b.commit()
        cap = n // 8 + 8192
        aud = torch.empty((Cn, cap), dtype=torch.float32, device=dev)

        def before():
            rc = L.csdr_demod_batch_process_packets(b.h, C.c_void_p(packets.data_ptr()), npk, pkt, nb.h,
                                                    C.c_void_p(aud.data_ptr()), cap, sp)
            assert rc == 0, ca._capi.last_error()

        def fn():
            return f.put_display_packets_blanked_ptr(b, packets.data_ptr(), npk, pkt, dc.data_ptr(), stream.cuda_stream)
    elif form == "workaround":
        rows = torch.empty((Cn, n, 2), dtype=torch.float32, device=dev)
        blanked = torch.empty((Cn, n, 2), dtype=torch.float32, device=dev)

        def fn():
            r = L.csdr_ingest_unpack(0, C.c_void_p(packets.data_ptr()), Cn, npk, pkt, C.c_void_p(rows.data_ptr()), n, None, sp)
            assert r == n, r
            nb.process_ptr(rows.data_ptr(), n, n, blanked.data_ptr(), n, stream.cuda_stream)
            return f.put_display_stream_ptr(blanked.data_ptr(), n, n, dc.data_ptr(), stream.cuda_stream)
    else:
        def fn():
            return f.put_display_packets_ptr(packets.data_ptr(), npk, pkt, dc.data_ptr(), stream.cuda_stream)
    ms, frames = [], []
    for i in range(a.warmup + a.calls):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        k = fn()
        e1.record(stream)
        e1.synchronize()
        if i >= a.warmup:
            ms.append(e0.elapsed_time(e1)); frames.append(k)
    torch.cuda.synchronize()
    print(json.dumps({"ms": round(float(np.median(ms)), 4), "frames": round(float(np.mean(frames)), 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--npackets", type=int, default=2185)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", default=None, help="internal: FORM:SKIP, one measurement in this process")
    a = ap.parse_args()
    if a.step:
        form, skip = a.step.split(":")
        return step(a, form, int(skip))
    out = {"tool": "bench_display_blanked", "channels": a.channels, "samples_per_call": a.npackets * 240, "size": a.size,
           "pkt_len": 1444, "calls": a.calls}
    for form, skip in STEPS:
        env = dict(os.environ)
        if form == "blanked_gather":
            env["CSDR_DISPLAY_BLANKED_LOADERS"] = "0"
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%d" % (form, skip)] + \
            [x for k in ("channels", "npackets", "size", "calls", "warmup") for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            out["failed"] = "%s skip %d: time limit" % (form, skip)
            break
        if r.returncode != 0:
            out["failed"] = "%s skip %d: exit status %d" % (form, skip, r.returncode)
            break
        res = json.loads(r.stdout.decode().strip().splitlines()[-1])
        out["%s_skip%d_ms" % (form, skip)] = res["ms"]
        out["%s_skip%d_frames" % (form, skip)] = res["frames"]
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
