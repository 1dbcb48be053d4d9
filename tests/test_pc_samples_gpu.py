"""The K4 sample rule on the GPU (tests/pc_samples_ref.py; its CPU side: tests/test_pc_samples_host.py): every post-chain
stage against the fp64 oracle, window by window, at m = 4 times the error of the fp32 yardstick --

  a. the leaf objects (CSMeter, CAgc complex / real / manual, CAmDemod, CSamDemod, CFmDemod, mono and stereo) at -12, -60 and
     -100 dBFS and above full scale, FM with and without a carrier;
  b. the same objects through calls of 1, 17, 1000, 1025, 2500, 1, 4099, 333 and 2048 samples (one burst each: tiles of 1024
     and a remainder; FM bursts of exactly one tile and of several);
  c. a DemodBatch of six receivers in two calls of more than four bursts (the lean walk behind smeter_call_kernel,
     agc_peaks_kernel and the fm_squelch kernels), each receiver's audio and S-meter against the oracle's and the yardstick's
     stages fed with the receiver's OWN stage tap 2 -- fp32 values, so all three sides see what K4 saw, from the first window;
  d. all of it again with one wave per receiver (CSDR_POSTCHAIN_WAVES=1);
  e. the leaf filters (filter_leaf_kernel) against derived bounds: CFir (ntaps + 1) u sum|h_k x_(n-k)|, CIir u |y| + 1e-9 rms(y).

The product runs in a fresh child process per wave count (the variable is read once per process); the parent holds what the
child wrote to the oracle and the yardstick, which are computed once and shared.  Run with -s for the measured ratios."""
import os
import subprocess
import sys
import time
import numpy as np
import pytest
import pc_samples_ref as S

pytestmark = pytest.mark.gpu
F32, F64 = S.F32, S.F64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

FIR_DESIGNS = [("lp", (1.0, 50.0, 5000, 9000, 31250.0), None), ("hp", (1.0, 50.0, 5000, 3000, 62500.0), None),
               ("lp", (1.0, 40.0, 4500, 5500, 31250.0), 5000.0)]                                    # test_fir_design_and_filtering
IIR_DESIGNS = [("LP", 3000.0, 1.0, 62500.0), ("HP", 300.0, 0.7, 31250.0), ("BP", 700.0, 5.0, 15625.0), ("BR", 25000, 1000.0, 100000)]
FIR_CALLS, IIR_CALLS = [1000, 2000], [1500, 2500]
IIR_ORDER = 1e-9               # of rms(y): what the order of the fp64 operations may move (the issue's figure; measured below it)

CHAIN = ["AM", "FM", "USB", "SAM", "CWU", "USBH"]             # USBH: USB with the hang timer on
CHAIN_FS, CHAIN_CALL, CHAIN_CALLS = 2e6, 19968 * 32, 2        # 19.5 / 9.75 / 4.9 bursts of audio per call: every pre-kernel runs
BURST = 1024                                                  # one hop of the 2048-point filter


def filter_inputs():
    r = np.random.default_rng(1)
    x = S.f32_values(r.standard_normal(3000) * 1000)
    xc = S.f32_values(x + 1j * r.standard_normal(3000) * 1000)
    r = np.random.default_rng(2)
    y = S.f32_values(r.standard_normal(4000) * 1000)
    yc = S.f32_values(y + 1j * r.standard_normal(4000) * 1000)
    return x, xc, y, yc


def chain_kw(name):
    import test_postchain_gpu as T
    m, kw = T.MODES["USB" if name == "USBH" else name]
    kw = dict(kw)
    if name == "USBH":
        kw.update(AgcHangOn=1, AgcDecay=500)
    return m, kw


def chain_input():
    """[receiver, sample]: each mode's carrier 100 kHz + 1 kHz x receiver off the centre, under level steps of 6 dB every 25 ms
    and a 30 Hz modulation"""
    import test_postchain_gpu as T
    n = CHAIN_CALL * CHAIN_CALLS
    t = np.arange(n) / CHAIN_FS
    env = np.where((t % 0.05) < 0.025, 1.0, 0.5) * (1 + 0.3 * np.sin(2 * np.pi * 30 * t))
    return np.stack([T.make_input("USB" if nm == "USBH" else nm, n, CHAIN_FS) * np.exp(2j * np.pi * 1000.0 * c * t) * env
                     for c, nm in enumerate(CHAIN)]).astype(np.complex64)


# ---- the child: the product's words -> a file --------------------------------------------------------------------------------
def product_outputs(out_path):
    import cutesdr_amd as ca
    import test_postchain_gpu as T
    out = {}
    for row in S.leaf_rows().values():
        o = row.build(ca)
        y = row.run(o)
        out["leaf/" + row.name] = np.stack(y) if row.stage == "smeter" else y
        o.close()
    x, xc, y, yc = filter_inputs()
    for k, (kind, args, hb) in enumerate(FIR_DESIGNS):
        for tag, v in (("real", x), ("cpx", xc)):
            f = ca.CFir()
            (f.InitLPFilter if kind == "lp" else f.InitHPFilter)(*args)
            if hb is not None:
                f.GenerateHBFilter(hb)
            out["fir/%d/%s" % (k, tag)] = np.concatenate([f.ProcessFilter(p) for p in S.split(v, FIR_CALLS)])
            f.close()
    for k, (kind, f0, q, fs) in enumerate(IIR_DESIGNS):
        for tag, v in (("real", y), ("cpx", yc)):
            f = ca.CIir(); f.Init(kind, f0, q, fs)
            out["iir/%d/%s" % (k, tag)] = np.concatenate([f.ProcessFilter(p) for p in S.split(v, IIR_CALLS)])
            f.close()
    xs = chain_input()
    C = len(CHAIN)
    b = ca.DemodBatch(C, 2048)
    b.set_input_rate(CHAIN_FS)
    for c, nm in enumerate(CHAIN):
        m, kw = chain_kw(nm)
        b.set_demod(c, m, T.info(ca, **kw))
    b.commit()
    for c in range(C):
        b.set_freq(c, -100e3 - 1000.0 * c)
    b.set_taps(2)
    got, taps, ave, peak = [[] for _ in range(C)], [[] for _ in range(C)], [], []
    for k in range(CHAIN_CALLS):
        ys = b.process(xs[:, k * CHAIN_CALL:(k + 1) * CHAIN_CALL])
        a, p = b.smeter_all(peak=True)
        ave.append(a.copy()); peak.append(p.copy())
        for c in range(C):
            got[c].append(ys[c]); taps[c].append(b.tap(c, 2))
    out["chain/rates"] = np.array([b.output_rate(c) for c in range(C)])
    out["chain/ave"], out["chain/peak"] = np.stack(ave), np.stack(peak)
    for c in range(C):
        out["chain/%d" % c], out["chain/%d/tap" % c] = np.concatenate(got[c]), np.concatenate(taps[c])
        out["chain/%d/calls" % c] = np.array([len(v) for v in taps[c]])
        assert [len(v) for v in got[c]] == [len(v) for v in taps[c]]
    b.close()
    np.savez(out_path, **out)
    print("product written: %d arrays" % len(out))


@pytest.fixture(scope="module", params=[4, 1], ids=["four-waves", "one-wave"])
def product(request, tmp_path_factory):
    """{name: array} of the product's outputs with four waves per receiver (the launch's own choice here) or one"""
    env = dict(os.environ)
    for k in ("CSDR_POSTCHAIN_WAVES", "CSDR_PLL_OVERLAP", "CSDR_PC_LEAN", "CSDR_AGC_PRE", "CSDR_FM_DEFER", "CSDR_SM_CALL"):
        env.pop(k, None)
    if request.param == 1:
        env["CSDR_POSTCHAIN_WAVES"] = "1"
    path = str(tmp_path_factory.mktemp("pcsamples") / ("product_%d.npz" % request.param))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_pc_samples_gpu as t; t.product_outputs(%r)" % (ROOT, HERE, path)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (request.param, r.stdout[-2000:] + r.stderr[-3000:])
    assert "product written" in r.stdout, r.stdout[-2000:]
    print("K4RULE child with %d wave(s): %.1f s" % (request.param, time.time() - t0))
    with np.load(path) as z:
        return request.param, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def designs(oracle):
    return S.Designs(oracle)


_want = {}


def reference(oracle, designs, row):
    """(the oracle's output, the yardstick's, the PLL windows left out) of a leaf row, computed once"""
    if row.name not in _want:
        lo = []
        if row.stage in ("fm", "sam") and row.carrier:
            lo = S.pll_windows_left_out(S.model_output(row, designs, F64)[1].errs)
        _want[row.name] = (row.run(row.build(oracle)), S.model_output(row, designs, F32)[0], lo)
    return _want[row.name]


def hold_row(oracle, designs, waves, row, got, worst, failed):
    """one leaf row under the rule; worst: {form: largest E / E_y} for the report; failed: what missed the rule (asserted by the
    caller once every row's figures are printed)"""
    want, y, lo = reference(oracle, designs, row)
    if row.stage == "smeter":
        for k, what in enumerate(("GetAve", "GetPeak")):
            E, Ey, ratio = S.db_rule(got[k], want[k], y[k])
            print("K4RULE waves %d %-22s %-8s |dB| %.2e  yardstick %.2e  ratio %.2f" % (waves, row.name, what, E, Ey, ratio))
            worst[row.form] = max(worst.get(row.form, 0.0), ratio)
            if not E <= S.M * Ey:
                failed.append((row.name, what, E, Ey))
        return
    assert got.shape == want.shape, (row.name, got.shape, want.shape)
    w = S.check_windows(got, want, y, leave_out=lo)
    if row.manual is not None:                                      # E_y is one rounding: the derived bound stands in for m E_y
        share = float((np.abs(got - want) / np.maximum(S.manual_bound(want), 1e-300)).max()) if want.any() else 0.0
        print("K4RULE waves %d %-22s largest error / (2 u |want|) %.3f" % (waves, row.name, share))
        worst[row.form] = max(worst.get(row.form, 0.0), share)
        if not (np.abs(got - want) <= S.manual_bound(want)).all():
            failed.append((row.name, share))
        return
    print("K4RULE waves %d %-22s %r" % (waves, row.name, w))
    worst["zero samples"] = worst.get("zero samples", 0) + w.zero_samples
    worst["zero windows"] = worst.get("zero windows", 0) + w.zero_windows
    worst["PLL windows left out"] = worst.get("PLL windows left out", 0) + len(lo)
    if row.carrier:
        worst[row.form] = max(worst.get(row.form, 0.0), w.worst)
    if not w.zeros_equal or (row.carrier and w.low) or not w.passed:
        failed.append((row.name, w, np.round(w.ratio, 2)))
    for j in lo:                                                    # a window left out stays under the bound K4 had
        if not np.abs(got[j * S.WIN:(j + 1) * S.WIN] - want[j * S.WIN:(j + 1) * S.WIN]).max() <= S.OLD_AUDIO:
            failed.append((row.name, "window left out", j))


def report(waves, what, worst):
    print("K4RULE waves %d %s: " % (waves, what) + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("stage", ["smeter", "agc", "am", "sam", "fm"])
def test_leaf_objects_at_four_levels(oracle, designs, product, stage):
    """a: the three levels of the same input and one row above full scale; AGC on at three settings and off at three gains;
    FM with the squelch open on a carrier and shut without one (every word zero on both sides)"""
    waves, out = product
    worst, failed = {}, []
    for row in S.leaf_rows().values():
        if row.stage == stage and not row.name.startswith("cuts/"):
            hold_row(oracle, designs, waves, row, out["leaf/" + row.name], worst, failed)
    report(waves, "leaf " + stage, worst)
    assert not failed, failed
    if stage == "fm":
        assert not out["leaf/fm/mono/nocarrier"].any()


def test_leaf_objects_through_ragged_calls(oracle, designs, product):
    """b: tile and call edges, windows cut from the concatenated stream"""
    waves, out = product
    worst, failed = {}, []
    for row in S.leaf_rows().values():
        if row.name.startswith("cuts/"):
            hold_row(oracle, designs, waves, row, out["leaf/" + row.name], worst, failed)
    report(waves, "ragged calls", worst)
    assert not failed, failed


_chain = {}


def chain_reference(oracle, designs, c, tap, calls, fs):
    """oracle, yardstick and float64 statement of receiver c's stages behind the filter on its own tap 2, once per tap"""
    import test_chain_taps_gpu as TC
    import test_postchain_gpu as T
    key = (c, hash(tap.tobytes()))
    if key not in _chain:
        nm = CHAIN[c]
        mode, (_, kw) = ("USB" if nm == "USBH" else nm), chain_kw(nm)
        di = T.info(oracle, **kw)
        info = {k: getattr(di, k) for k, _ in di._fields_}
        post, sm = TC._oracle_post_chain(oracle, mode, False, fs, kw), oracle.CSMeter()
        y32, y64 = S.PostChain(designs, mode, info, fs, F32), (S.PostChain(designs, mode, info, fs, F64) if mode in ("FM", "SAM") else None)
        want, y, ave, peak, yave, ypeak = [], [], [], [], [], []
        for part in S.split(tap, calls):
            for k in range(0, len(part), BURST):               # burst by burst, as CDemodulator hands them on: FM's squelch is per burst
                want.append(post(part[k:k + BURST])[1]); y.append(y32.process(part[k:k + BURST]))
                if y64 is not None:
                    y64.process(part[k:k + BURST])
            sm.ProcessData(part, fs); ave.append(sm.GetAve()); peak.append(sm.GetPeak())
            yave.append(F32(y32.sm.get_ave())); ypeak.append(F32(y32.sm.get_peak()))          # smeter_all stores fp32
        lo = S.pll_windows_left_out(y64.dem.errs) if y64 is not None else []
        _chain[key] = (np.concatenate(want), np.concatenate(y), lo, np.array(ave), np.array(peak), np.array(yave), np.array(ypeak))
    return _chain[key]


@pytest.mark.parametrize("c", range(len(CHAIN)), ids=CHAIN)
def test_chain_receivers_on_their_own_filter_output(oracle, designs, product, c):
    """c: the lean walk and its pre-kernels; audio from the first window, the S-meter readings after each call"""
    waves, out = product
    fs = float(out["chain/rates"][c])
    got, tap, calls = out["chain/%d" % c].astype(F64), out["chain/%d/tap" % c], [int(v) for v in out["chain/%d/calls" % c]]
    assert min(calls) >= 4 * 1024 and len(got) == len(tap)
    want, y, lo, ave, peak, yave, ypeak = chain_reference(oracle, designs, c, tap, calls, fs)
    w = S.check_windows(got, want, y, leave_out=lo)
    print("K4RULE waves %d chain %-5s %r" % (waves, CHAIN[c], w))
    Ea, Eya, ra = S.db_rule(out["chain/ave"][:, c], ave, yave)
    Ep, Eyp, rp = S.db_rule(out["chain/peak"][:, c], peak, ypeak)
    print("K4RULE waves %d chain %-5s smeter ave |dB| %.2e yardstick %.2e ratio %.2f; peak |dB| %.2e yardstick %.2e" % (waves, CHAIN[c], Ea, Eya, ra, Ep, Eyp))
    assert w.zeros_equal and not w.low, (CHAIN[c], w.rms.min())
    assert len(lo) <= S.PLL_MAX_LEFT_OUT, (CHAIN[c], lo)
    assert w.passed, (CHAIN[c], w, w.ratio)
    for j in lo:
        assert np.abs(got[j * S.WIN:(j + 1) * S.WIN] - want[j * S.WIN:(j + 1) * S.WIN]).max() <= S.OLD_AUDIO, (CHAIN[c], j)
    assert Ea <= S.M * Eya and Ep <= S.M * Eyp, (CHAIN[c], Ea, Eya, Ep, Eyp)


def test_leaf_filters_against_derived_bounds(oracle, designs, product):
    """e: CFir, real and complex, state carried over two calls: |got - y| <= (ntaps + 1) u sum|h_k x_(n-k)| (one rounding of a
    tap, one of a product, ntaps - 1 additions in any order; inputs are fp32 values).  CIir: an fp32 rounding of the fp64
    recurrence, |got - y| <= u |y| + 1e-9 rms(y) per component."""
    waves, out = product
    x, xc, yv, yc = filter_inputs()
    share = 0.0
    for k, (kind, args, hb) in enumerate(FIR_DESIGNS):
        c, i, q = designs.fir(kind, *args, hilbert=hb)
        for tag, v in (("real", x), ("cpx", xc)):
            f = S.Fir(c, dt=F64) if tag == "real" else S.Fir(i, q, dt=F64)
            ys = [f.run(p, want_s=True) for p in S.split(v, FIR_CALLS)]
            want, s = np.concatenate([a for a, _ in ys]), np.concatenate([b for _, b in ys])
            r = oracle.CFir()
            (r.InitLPFilter if kind == "lp" else r.InitHPFilter)(*args)
            if hb is not None:
                r.GenerateHBFilter(hb)
            ref = np.concatenate([r.ProcessFilter(p) for p in S.split(v, FIR_CALLS)])
            assert np.abs(want - ref).max() <= 1e-12 * S._rms(ref)                                # the statement is the oracle's
            e, bound = np.abs(out["fir/%d/%s" % (k, tag)] - ref), (len(c) + 1) * S.U * s
            share = max(share, float((e / bound).max()))
            assert (e <= bound).all(), (k, tag, float((e / bound).max()))
    print("K4RULE waves %d CFir largest error / bound %.3f" % (waves, share))
    share = 0.0
    for k, (kind, f0, q, fs) in enumerate(IIR_DESIGNS):
        for tag, v in (("real", yv), ("cpx", yc)):
            r = oracle.CIir(); r.Init(kind, f0, q, fs)
            ref = np.concatenate([r.ProcessFilter(p) for p in S.split(v, IIR_CALLS)])
            got = out["iir/%d/%s" % (k, tag)]
            for gc, rc in ((got.real, ref.real), (got.imag, ref.imag)) if tag == "cpx" else ((got, ref),):
                bound = S.U * np.abs(rc) + IIR_ORDER * S._rms(rc)
                e = np.abs(gc - rc)
                share = max(share, float((e / bound).max()))
                assert (e <= bound).all(), (k, tag, float((e / bound).max()))
    print("K4RULE waves %d CIir largest error / bound %.3f" % (waves, share))
