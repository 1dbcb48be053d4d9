"""Batch NCO-spur calibration (csdr_spurcal_batch, K13) beside what a host had before it, on one buffer.

256 channels x 2185 datagrams per call (the shape of tools/bench_seqcheck.py), 24 bit (1444 bytes) and 16 bit (1028 bytes).
Device time per call with HIP events on one stream, medians of --calls; the calls ALTERNATE in one process (one round =
each of them once), so that drift of the box lands on all of them alike:
  put_all / put_16 / put_none   csdr_spurcal_batch_put_packets with 256, 16 and 0 of the receivers calibrating (the
                                commands that arm them are issued and waited for before the clock starts)
  old_packets                   csdr_ingest_spurcal_packets: the stateless kernel, always every receiver
  seqcheck                      csdr_seqcheck_batch_put: one header word per datagram -- the yardstick of put_none
  blanked_all                   csdr_spurcal_batch_put_packets_blanked behind a blanked chain call (the chain call is not
                                timed), every receiver calibrating, every blanker on
  old_two_pass                  what a host had to do for those samples: a blanker pass into fp32 rows
                                (csdr__noiseproc_batch_process_packets) + csdr_ingest_spurcal on the rows
put_all_GBps is the datagram bytes / the median: against the mask pass's measured load rate (HISTORY.md) it says whether
the put reads the datagrams once at bandwidth.  The payload is random bytes.
Each packet length is one step: a child process of its own under its own time limit (--step-timeout seconds); a step that
fails or runs out of time ends the run.  Prints one JSON line.
Usage: python tools/bench_spurcal.py [--channels 256] [--npackets 2185] [--calls 30] [--warmup 5]
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
    Cn, npk = a.channels, a.npackets
    per, bits = (240, 24) if pkt == 1444 else (256, 16)
    n = npk * per
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    fs = 500e3
    base = dict(HiCut=5000, HiCutmin=5000, HiCutmax=15000, LowCut=-5000, LowCutmin=-15000, LowCutmax=-5000,
                FilterClickResolution=100, Offset=0, SquelchValue=0, AgcSlope=0, AgcThresh=-100, AgcManualGain=30,
                AgcDecay=200, AgcOn=1, AgcHangOn=0, Symetric=1)
    am = dict(base, HiCutmin=500, HiCutmax=10000, LowCutmax=-500, LowCutmin=-10000)
    g = torch.Generator(device=dev); g.manual_seed(bits)
    packets = torch.randint(0, 256, (Cn, npk, pkt), dtype=torch.uint8, device=dev, generator=g)
    pp = C.c_void_p(packets.data_ptr())
    dc = torch.zeros((Cn, 2), dtype=torch.float64, device=dev)
    dc2 = torch.zeros((Cn, 2), dtype=torch.float64, device=dev)
    rows = torch.empty((Cn, n, 2), dtype=torch.float32, device=dev)
    sc, scb, sq = ca.SpurCalBatch(Cn), ca.SpurCalBatch(Cn), ca.SeqCheckBatch(Cn)
    nb, nb2 = ca.NoiseProcBatch(Cn), ca.NoiseProcBatch(Cn)
    for x in (nb, nb2):
        x.setup(True, 60.0, 100.5 / fs * 1e6, fs)
    b = ca.DemodBatch(Cn, 2048); b.set_input_rate(fs)
    for c in range(Cn):
        b.set_demod(c, 0 if c % 2 else 2, ca.DemodInfo(**(am if c % 2 else base)))
    b.commit()
    cap = n // 8 + 8192
    aud = torch.empty((Cn, cap), dtype=torch.float32, device=dev)

    def arm(s, active):
        s.set(0.0, 0.0, -1)
        if active == Cn:
            s.start_cal(-1)
        else:
            for c in range(0, Cn, max(1, Cn // max(active, 1)))[:active]:
                s.start_cal(c)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def put(active):
        def run():
            arm(sc, active)
            return timed(lambda: sc.put_packets_ptr(packets.data_ptr(), npk, pkt, stream.cuda_stream))
        return run

    def old_packets():
        return timed(lambda: L.csdr_ingest_spurcal_packets(0, pp, Cn, npk, pkt, C.c_void_p(dc.data_ptr()), sp))

    def seqcheck():
        return timed(lambda: sq.put(packets.data_ptr(), npk, pkt, stream.cuda_stream))

    def blanked_all():
        arm(scb, Cn)
        assert L.csdr_demod_batch_process_packets(b.h, pp, npk, pkt, nb.h, C.c_void_p(aud.data_ptr()), cap, sp) == 0, ca._capi.last_error()
        return timed(lambda: scb.put_packets_blanked_ptr(b, packets.data_ptr(), npk, pkt, stream.cuda_stream))

    def old_two_pass():
        def run():
            assert L.csdr__noiseproc_batch_process_packets(nb2.h, pp, npk, pkt, C.c_void_p(rows.data_ptr()), n, sp) == 0, ca._capi.last_error()
            assert L.csdr_ingest_spurcal(0, C.c_void_p(rows.data_ptr()), n, Cn, n, C.c_void_p(dc2.data_ptr()), sp) == 0, ca._capi.last_error()
        return timed(run)

    calls = (("put_all", put(Cn)), ("put_16", put(min(16, Cn))), ("put_none", put(0)), ("old_packets", old_packets),
             ("seqcheck", seqcheck), ("blanked_all", blanked_all), ("old_two_pass", old_two_pass))
    ms = {k: [] for k, _ in calls}
    for i in range(a.warmup + a.calls):
        for name, fn in calls:
            t = fn()
            if i >= a.warmup:
                ms[name].append(t)
    b.flush(stream.cuda_stream)
    torch.cuda.synchronize()
    out = {"input_MB_%dbit" % bits: round(Cn * npk * pkt / 1e6, 1)}
    for name, v in ms.items():
        out["%s_%dbit_ms" % (name, bits)] = round(float(np.median(v)), 4)
        out["%s_%dbit_min_ms" % (name, bits)] = round(float(np.min(v)), 4)
    out["put_all_%dbit_GBps" % bits] = round(Cn * npk * pkt / 1e6 / out["put_all_%dbit_ms" % bits], 1)
    # what was timed did what it says: every receiver of put_all / blanked_all used its datagrams, none of put_none's moved
    arm(sc, Cn); sc.put_packets_ptr(packets.data_ptr(), npk, pkt, stream.cuda_stream)
    q = per // 2
    used = min(npk, -(-300000 // q))
    assert sc.get_state(Cn - 1)[2:] == (used * q, used == npk), sc.get_state(Cn - 1)
    assert scb.get_state(0)[2] == used * q
    arm(sc, 0); sc.put_packets_ptr(packets.data_ptr(), npk, pkt, stream.cuda_stream)
    assert sc.get_state(0) == (0.0, 0.0, used * q, False)       # (SET leaves the count)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--npackets", type=int, default=2185)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", type=int, default=0, help="(internal) run the one step of this packet length")
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.step:
        return step(a, a.step)
    out = {"tool": "bench_spurcal", "channels": a.channels, "npackets": a.npackets, "calls": a.calls}
    for pkt in (1444, 1028):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(pkt)] + \
            ["--%s=%d" % (k, getattr(a, k)) for k in ("channels", "npackets", "calls", "warmup")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.step_timeout)
        if r.returncode != 0:
            sys.exit("bench_spurcal: the %d-byte step ended with status %d; nothing more is started" % (pkt, r.returncode))
        out.update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
