"""The two test-bench tap points that end in the batch scope, wired as INTEGRATION.md section 4 describes them:
  PROFILE_5  SoundSinkBatch put -> csdr_soundsink_batch_get_tap -> csdr_scope_batch_put_mono16 / _put_stereo16 at 48 kHz
  PROFILE_7  blanked chain call -> csdr_noiseproc_batch_trace_last -> csdr_scope_batch_put_cpx
Nothing leaves the device on either way; the checks read the same samples a second way (the sink's queue; the
restatement of the blanker's trace) and run the scope's restatement on them: screens and emits are integers and exact."""
import ctypes as C
import numpy as np
import pytest

import nbtrace_ref as N
import scope16_ref as S
import scope_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_sink_tap_into_the_scope(stereo):
    """four receivers, a 1 kHz tone at user rates of 12 and 8 kHz, three puts.  After each put the tap's rows go into
    the scope (PNORM, 5 ms across 100 pixels, rate 48000).  The sink's queue hands out its first sample once it is more
    than half full (soundout.cpp:316-333), so after the third put one GetOutQueue per receiver delivers, in order, the
    very samples the three taps showed: the restatement runs on those, put by put."""
    import torch
    import cutesdr_amd as ca
    torch.cuda.init()
    Cn, w = 4, 100
    rates = [12000.0, 12000.0, 8000.0, 8000.0]
    n_in = [1000, 1000, 700, 700]
    sink = ca.SoundSinkBatch(Cn, stereo=stereo)
    assert sink.tap() is None                            # CSDR_ESTATE before the first put
    for c in range(Cn):
        sink.ChangeUserDataRate(c, rates[c])
    scope, ref = ca.ScopeBatch(Cn), S.RefBatch16(Cn)
    for x in (scope, ref):
        x.resizeEvent(w, 100); x.OnHorzSpan(5); x.OnTrigLevel(100); x.OnTriggerMode(R.TRIG_PNORM)
    stream = torch.cuda.current_stream().cuda_stream
    counts, emits, taps = [], [], []
    for p in range(3):
        rows = np.zeros((Cn, 1000), dtype=np.complex64 if stereo else np.float32)
        for c in range(Cn):
            t = (np.arange(n_in[c]) + p * n_in[c]) / rates[c]
            tone = 8000.0 * np.sin(2 * np.pi * 1000.0 * t + 0.3 * c)
            rows[c, :n_in[c]] = tone + 1j * 5000.0 * np.cos(2 * np.pi * 1000.0 * t) if stereo else tone
        k = sink.PutOutQueue(rows, n_in)
        d_rows, stride, d_counts = sink.tap()
        taps.append((d_rows, stride, d_counts))
        dev_counts = np.zeros(Cn, dtype=np.int32)
        assert ca.lib().csdr_dev_download(0, dev_counts.ctypes.data_as(C.c_void_p), C.c_void_p(d_counts), dev_counts.nbytes) == 0
        assert dev_counts.tolist() == k.tolist() and stride == 16384 and (k > 2000).all()
        scope.put16_ptr(d_rows, stride, k, 48000.0, stream, stereo=stereo)
        e = scope.get_emits().tolist()                   # (waits for the put: the staging is rewritten by the next one)
        for c in range(Cn):
            if e[c]:
                scope.time_plot_done(c)
        counts.append(k.tolist()); emits.append(e)
    assert taps[0] == taps[1] == taps[2]                 # the staging itself: nothing copied, the same pointers
    total = np.sum(counts, axis=0)
    assert (total > 8192).all() and (total < 16384).all()
    heard = [sink.GetOutQueue(c, int(total[c])) for c in range(Cn)]
    assert all(np.abs(h).max() > 3000 for h in heard)
    for p in range(3):
        for c in range(Cn):
            a = sum(counts[q][c] for q in range(p))
            x = heard[c][a:a + counts[p][c]]
            if stereo:
                ref.r[c].DisplayStereo16(x[:, 0].tolist(), x[:, 1].tolist(), 48000.0)
            else:
                ref.r[c].DisplayMono16(x.tolist(), 48000.0)
        want = [r.emits for r in ref.r]
        assert [sum(emits[q][c] for q in range(p + 1)) for c in range(Cn)] == want, (p, emits, want)
        for c in range(Cn):
            if emits[p][c]:
                ref.time_plot_done(c)
    assert all(r.emits >= 1 for r in ref.r), [r.emits for r in ref.r]
    scope.put16_ptr(taps[-1][0], taps[-1][1], [0] * Cn, 48000.0, stream, stereo=stereo)      # a put of nothing applies the last time_plot_done
    for c in range(Cn):
        re, im = scope.get_screen(c)
        assert (re.tolist(), im.tolist()) == ref.screen(c), c
        assert scope.get_state(c)[:7].tolist() == ref.state(c), c
        assert np.abs(re).max() > 3000 and bool(np.abs(im).max() > 1000) == stereo


def test_blanker_trace_into_the_scope():
    """a blanked chain call (csdr_demod_batch_process_blanked, two receivers at 2 MS/s), trace_last into rows, put_cpx in
    PNORM at level 100: the trace's real part is 0 while blanking and about 1330 (the moving sum over the ratio)
    otherwise, so the scope triggers where a blanking stretch ends.  The screens equal the scope's restatement run on
    the blanker restatement's trace (integral input: that trace is the device's bit for bit)."""
    import torch
    import cutesdr_amd as ca
    from test_nbtrace_gpu import make_chain, make_blanker, stream
    torch.cuda.init()
    L = ca.lib()
    fs, Cn, n, w = 2e6, 2, 240 * 256, 100
    settings = [(True, fs, 20.0, 50.0), (True, fs, 20.0, 2.0)]
    x = np.stack([stream(50 + c, 3 * n, False) for c in range(Cn)])
    b, nb = make_chain(ca, Cn, fs), make_blanker(ca, settings)
    refs = []
    for on, f, th, wd in settings:
        r = N.RefNoiseProc(); r.SetupBlanker(on, th, wd, f); refs.append(r)
    scope, sref = ca.ScopeBatch(Cn), R.RefBatch(Cn)
    for s in (scope, sref):
        s.resizeEvent(w, 100); s.OnHorzSpan(1); s.OnTrigLevel(100); s.OnTriggerMode(R.TRIG_PNORM)
    cap = n // 8 + 2048 + 4096
    din, dout = ca.DeviceBuffer(Cn * n * 8), ca.DeviceBuffer(Cn * cap * 4)
    trace = torch.zeros((Cn, n), dtype=torch.complex64, device="cuda")
    shown = 0
    for k in range(3):
        part = x[:, k * n:(k + 1) * n]
        din.upload(part.astype(np.complex64))
        assert L.csdr_demod_batch_process_blanked(b.h, C.c_void_p(din.ptr), n, n, nb.h, C.c_void_p(dout.ptr), cap, None) == 0
        assert nb.trace_last(trace.data_ptr(), n, n, d_in=din.ptr, in_stride=n) == 0
        scope.put_ptr(trace.data_ptr(), n, n, fs, None, cpx=True)
        want = np.stack([N.trace_fp32(refs[c].ProcessBlanker(part[c])[1]) for c in range(Cn)])
        sref.put(want, 0, [n] * Cn, [fs] * Cn)
        emits = scope.get_emits().tolist()
        assert np.array_equal(trace.cpu().numpy().view(np.uint32), want.view(np.uint32)), k
        for c in range(Cn):
            re, im = scope.get_screen(c)
            assert (re.tolist(), im.tolist()) == sref.screen(c), (k, c)
            if emits[c]:
                post = (7 * w) // 10
                assert re[w - post] >= 100 > re[w - post - 1], (k, c)          # the trigger pixel: blanking ends there
                scope.time_plot_done(c); sref.time_plot_done(c); shown += 1
    assert [r.emits for r in sref.r] == [int(s) for s in (scope.get_state(c)[7] for c in range(Cn))] and shown >= 2 * Cn - 2, shown
    b.flush()
