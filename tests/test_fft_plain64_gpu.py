"""csdr_fft_batch_fwd_f64 / _rev_f64 (K3q) -- CFft::FwdFFT / RevFFT of every frame of every row in fp64 on the device,
512 ... 65536 points -- held to the rule of fft_plain64_ref.py: per frame E <= 4 E_y, E the per-bin relative error against
scipy.fft in long double on a flat-spectrum fp64 probe, E_y the same figure of scipy's fp64 transform.

512 ... 4096 points run as one LDS image per frame (4 / 4 / 2 / 1 frames per workgroup), 8192 ... 65536 as the four-step
form in two launches through the object's fp64 work buffer: every size is a configuration of its own, so the tests run
all eight."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fft_plain64_ref as P
import fft_plain_ref as P32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.complex128(-12345.5 + 54321.25j)
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def ca():
    P.require_long_double()
    import cutesdr_amd
    yield cutesdr_amd
    for fb in _objs.values():                                  # the module's shared objects go with the module
        fb.close()
    _objs.clear()


_objs = {}


def batch(ca, channels, n):
    """one object per channel count for the module (destroyed by the `ca` fixture's teardown), set to n points; every
    test sets the size it needs, none relies on what another left"""
    if channels not in _objs:
        _objs[channels] = ca.FftBatch(channels)
    fb = _objs[channels]
    if fb.size() != n:
        fb.set_params(n, False, 0.0, P.FS)
    return fb


def frames_of(n, rows, nframes, pool=None):
    """(x [rows, nframes, n] complex128, seeds [rows, nframes]); pool: that many distinct probes, neighbours different"""
    seeds = np.array([[P.seed_of(n, (r * nframes + k) % pool if pool else r * nframes + k) for k in range(nframes)]
                      for r in range(rows)])
    x = np.stack([np.stack([P.probe(n, int(s)) for s in row]) for row in seeds])
    return x, seeds


def run(ca, fb, x, sign, in_stride=None, out_stride=None, in_place=False):
    """the call on rows of in_stride / out_stride samples -> (out rows [rows, out_stride], (input rows after, before))"""
    rows, nframes, n = x.shape
    in_stride = in_stride or nframes * n
    out_stride = in_stride if in_place else (out_stride or nframes * n)
    hin = np.full((rows, in_stride), SENT, dtype=np.complex128)
    hin[:, :nframes * n] = x.reshape(rows, -1)
    din = ca.host.DeviceBuffer(hin.nbytes)
    din.upload(hin)
    dout = din
    if not in_place:
        dout = ca.host.DeviceBuffer(rows * out_stride * 16)
        dout.upload(np.full((rows, out_stride), SENT, dtype=np.complex128))
    (fb.fwd64_ptr if sign > 0 else fb.rev64_ptr)(din.ptr, in_stride, dout.ptr, out_stride, nframes)
    ca.host.sync()
    out = dout.download(np.complex128, rows * out_stride).reshape(rows, out_stride)
    back = din.download(np.complex128, rows * in_stride).reshape(rows, in_stride)
    din.free()
    if not in_place:
        dout.free()
    return out, (back, hin)


def check_all(out, seeds, n, sign, what):
    rows, nframes = seeds.shape
    worst, orc = 0.0, 0.0
    for r in range(rows):
        for k in range(nframes):
            e, eo = P.check_frame(out[r, k * n:(k + 1) * n], n, int(seeds[r, k]), sign, "%s row %d frame %d" % (what, r, k))
            worst, orc = max(worst, e), max(orc, eo)
    e_y = max(P.reference(n, int(s), sign)[1] for s in seeds.ravel())
    print("%s n=%d sign=%+d: worst E / E_y = %.2f (allowed %g), the oracle's %.2f, E_y = %.3g" % (what, n, sign, worst, P.MARGIN, orc, e_y))
    return worst


# 1 ---- the rule: every size, both signs, out of place, rows with different strides and guard words
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_every_size_out_of_place(ca, n, sign):
    x, seeds = frames_of(n, 3, 2)
    out, (back, hin) = run(ca, batch(ca, 3, n), x, sign, in_stride=2 * n + 8, out_stride=2 * n + 24)
    check_all(out, seeds, n, sign, "out of place")
    assert (P.words(out[:, 2 * n:]) == P.words(np.full((3, 24), SENT))).all(), "the guard words of d_out were written"
    assert (P.words(back) == P.words(hin)).all(), "d_in was changed"


# 2 ---- in place = out of place
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_in_place_equals_out_of_place(ca, n, sign):
    x, _ = frames_of(n, 3, 2)
    fb = batch(ca, 3, n)
    a, _ = run(ca, fb, x, sign)
    b, _ = run(ca, fb, x, sign, in_place=True)
    assert (P.words(a) == P.words(b)).all()


# 3 ---- impulses: correctly rounded twiddles, and the bin order of every pass
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_impulses(ca, n, sign):
    ms = [1, n // 2 + 3]
    amp = 3000.0
    x = np.zeros((len(ms), 1, n), dtype=np.complex128)
    for i, m in enumerate(ms):
        x[i, 0, m] = amp
    out, _ = run(ca, batch(ca, len(ms), n), x, sign)
    for i, m in enumerate(ms):
        err = float(np.abs(out[i].astype(P.CLD) - P.impulse_ref(n, m, sign, amp)).max())
        print("impulse n=%d m=%d sign=%+d: %.3g of the allowed %.3g" % (n, m, sign, err, 4 * EPS * amp))
        assert err <= 4 * EPS * amp, (n, m, sign, err)


# 4 ---- round trip: both transforms' bounds added
@pytest.mark.parametrize("n", P.SIZES)
def test_round_trip(ca, n):
    x, seeds = frames_of(n, 3, 2)
    fb = batch(ca, 3, n)
    y, _ = run(ca, fb, x, +1)
    z, _ = run(ca, fb, y.reshape(3, 2, n), -1)
    for r in range(3):
        for k in range(2):
            s = int(seeds[r, k])
            e_y = max(P.reference(n, s, +1)[1], P.reference(n, s, -1)[1])
            # E of the forward transform is an error of E sqrt(n) rms per bin; the reverse transform of that error, with
            # its own, divided by n, is at most 2 x 4 E_y rms per sample
            err = float(np.abs(z[r, k * n:(k + 1) * n].astype(P.CLD) / n - x[r, k]).max())
            bound = 2 * P.MARGIN * e_y * P.k1_bins.rms(x[r, k])
            print("round trip n=%d: %.3g of the allowed %.3g" % (n, err, bound))
            assert err <= bound, (n, r, k, err, bound)


# 5 ---- the four-step form's frame groups
@pytest.mark.parametrize("n", [P.FOUR_STEP[0], P.FOUR_STEP[-1]])
def test_four_step_group_boundary(ca, n):
    fb = batch(ca, 3, n)
    g = fb.plain_group64()
    assert g == 64 // 3, g
    x, seeds = frames_of(n, 3, g + 1, pool=8)
    out, _ = run(ca, fb, x, +1, out_stride=(g + 1) * n + 8)
    check_all(out, seeds, n, +1, "groups")
    assert (P.words(out[:, (g + 1) * n:]) == P.words(np.full((3, 8), SENT))).all()
    alone, _ = run(ca, fb, x[:, g:], +1)
    assert (P.words(alone) == P.words(out[:, g * n:(g + 1) * n])).all(), "the second group's frames differ from a call of their own"


def test_group_is_zero_below_the_four_step_sizes(ca):
    for n in P.SIZES:
        g = batch(ca, 3, n).plain_group64()
        assert (g == 21) if n in P.FOUR_STEP else (g == 0), (n, g)


# 6 ---- a short last workgroup
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", [512, 1024, 2048])
def test_short_last_workgroup(ca, n, sign):
    x, seeds = frames_of(n, 3, 3)
    assert (3 * 3) % (4 if n <= 1024 else 2), "the last workgroup must be short"
    out, (back, hin) = run(ca, batch(ca, 3, n), x, sign, out_stride=3 * n + 8)
    check_all(out, seeds, n, sign, "short workgroup")
    assert (P.words(out[:, 3 * n:]) == P.words(np.full((3, 8), SENT))).all()
    assert (P.words(back) == P.words(hin)).all()


# 7 ---- nothing else moves
def test_nothing_else_moves(ca):
    fb = ca.FftBatch(2)
    fb.set_params(4096, False, 0.0, P.FS)
    fb.set_ave(2)
    x32 = np.stack([np.stack([P32.probe(4096, P32.seed_of(4096, 3 * r + k)) for k in range(3)]) for r in range(2)])
    fb.put_display(x32.reshape(2, -1))

    def state():
        ov, pix = fb.screen_all(100, 300, 0.0, -120.0, -20000, 20000)
        return [fb.ave_buf(0), fb.ave_buf(1), np.array([fb.total_count(0), fb.total_count(1)]), ov, pix]
    before = state()
    assert before[2].tolist() == [3, 3]
    fixed32 = fb.fwd(x32.reshape(2, -1))                       # the fp32 transform before anything fp64 exists
    x, seeds = frames_of(4096, 2, 3)
    fb.prepare64()
    assert (P32.words(fb.fwd(x32.reshape(2, -1))) == P32.words(fixed32)).all(), "fp32 words moved after prepare64"
    for sign in P.SIGNS:
        out, _ = run(ca, fb, x, sign)
        check_all(out, seeds, 4096, sign, "beside the display")
    assert (P32.words(fb.fwd(x32.reshape(2, -1))) == P32.words(fixed32)).all(), "fp32 words moved after an fp64 call"
    after = state()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for n in (32768, 512):                                     # set_params drops the fp64 state; the next call re-prepares
        fb.set_params(n, False, 0.0, P.FS)
        x, seeds = frames_of(n, 2, 1)
        for sign in P.SIGNS:
            out, _ = run(ca, fb, x, sign)
            check_all(out, seeds, n, sign, "after set_params")


# 8 ---- refusals
@pytest.mark.parametrize("n", [1024, 4096, 32768])
def test_refusals(ca, n):
    from cutesdr_amd import _capi
    L = _capi.lib()
    fb = batch(ca, 2, n)
    total = 2 * (2 * n + 16) + 2 * n
    fill = np.full(total, SENT, dtype=np.complex128)
    buf = ca.host.DeviceBuffer(fill.nbytes)
    other = ca.host.DeviceBuffer(fill.nbytes)
    buf.upload(fill)
    other.upload(fill)
    s = 2 * n + 16
    vp = C.c_void_p

    def call(f, d_in, in_stride, d_out, out_stride, nframes, fn):
        return fn(f, vp(d_in), in_stride, vp(d_out), out_stride, nframes, None)
    cases = {
        "NULL handle": (None, buf.ptr, s, other.ptr, s, 2),
        "NULL d_in": (fb.h, None, s, other.ptr, s, 2),
        "NULL d_out": (fb.h, buf.ptr, s, None, s, 2),
        "nframes < 0": (fb.h, buf.ptr, s, other.ptr, s, -1),
        "short in_stride": (fb.h, buf.ptr, 2 * n - 1, other.ptr, s, 2),
        "short out_stride": (fb.h, buf.ptr, s, other.ptr, 2 * n - 1, 2),
        "partial overlap": (fb.h, buf.ptr, s, buf.ptr + 16 * n, s, 2),
        "same base, other stride": (fb.h, buf.ptr, s, buf.ptr, s + 8, 2),
        "d_in 8-byte aligned": (fb.h, buf.ptr + 8, s, other.ptr, s, 2),
        "d_out 8-byte aligned": (fb.h, buf.ptr, s, other.ptr + 8, s, 2),
    }
    for fn in (L.csdr_fft_batch_fwd_f64, L.csdr_fft_batch_rev_f64):
        for what, args in cases.items():
            assert call(*args, fn=fn) == _capi.CSDR_EINVAL, what
        assert call(fb.h, buf.ptr, s, other.ptr, s, 0, fn=fn) == _capi.CSDR_OK
    assert L.csdr_fft_batch_prepare_f64(None) == _capi.CSDR_EINVAL and L.csdr_fft_batch_plain_group_f64(None) == _capi.CSDR_EINVAL
    assert L.csdr_fft_fwd_f64(None, vp(0)) == _capi.CSDR_EINVAL and L.csdr_fft_rev_f64(None, vp(0)) == _capi.CSDR_EINVAL
    ca.host.sync()
    for d in (buf, other):
        assert (P.words(d.download(np.complex128, total)) == P.words(fill)).all()
        d.free()


# 9 ---- one receiver: the host form on doubles
@pytest.mark.parametrize("n", [2048, 65536])
def test_one_receiver(ca, n):
    f = ca.CFft()
    f.SetFFTParams(n, False, 0.0, P.FS)
    seed = P.seed_of(n, 0)
    x = P.probe(n, seed)
    fp32_before = f.FwdFFT(x)
    e, _ = P.check_frame(f.fwd64(x), n, seed, +1, "host fwd64")
    e2, _ = P.check_frame(f.rev64(x), n, seed, -1, "host rev64")
    print("one receiver n=%d: E / E_y = %.2f forward, %.2f reverse" % (n, e, e2))
    # the fp32 form on the same input: the words it gave before anything fp64 existed ...
    fp32_after = f.FwdFFT(x)
    assert (P.words(fp32_after) == P.words(fp32_before)).all(), "csdr_fft_fwd moved"
    # ... which at 2048 ... 16384 points are FftBatch.fwd's of one row (both run fft_fwd_passes).  At the other sizes
    # csdr_fft_fwd is the multi-launch transform through HBM and the batch form the four-step one (moving it is
    # out of scope), 0.5 apart in words of 7.7e5 on this probe, so there is no such tie to hold it by: there, and at 2048
    # points too, the words of a fixed integer input are held to the digests recorded from the commit before K3q
    # (tests/golden/fft_fwd_fp32_words.json; tools/record_fft_fwd_words.py records it from a given library)
    if 2048 <= n <= 16384:
        row = batch(ca, 1, n).fwd(x.astype(np.complex64).reshape(1, n))[0].astype(np.complex128)
        assert (P.words(fp32_after) == P.words(row)).all(), "csdr_fft_fwd differs from csdr_fft_batch_fwd of one row"
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "fft_fwd_fp32_words.json")))
    xi = fixed_input(n)
    for name, fn in (("fwd", f.FwdFFT), ("rev", f.RevFFT)):
        assert hashlib.sha256(P.words(fn(xi)).tobytes()).hexdigest() == golden["%s_%d" % (name, n)], \
            "csdr_fft_%s at %d points no longer returns the words of the commit before K3q" % (name, n)


def fixed_input(n):
    """integers below 2001 in both parts, the same on every machine (tools/record_fft_fwd_words.py: fixed_input)"""
    i = np.arange(n, dtype=np.int64)
    return (((i * 7919) % 4001 - 2000) + 1j * ((i * 104729) % 3989 - 1994)).astype(np.complex128)


# 10 ---- against the reference's compiled CFft
@pytest.mark.parametrize("n", [2048, 16384])
def test_against_the_reference_code(ca, n):
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref is not built")
    x, seeds = frames_of(n, 3, 2)
    out, _ = run(ca, batch(ca, 3, n), x, +1)
    for r in range(3):
        for k in range(2):
            ref = oref.fft(np.array(x[r, k]), +1)
            e, _ = P.check_frame(out[r, k * n:(k + 1) * n], n, int(seeds[r, k]), +1, "reference code row %d frame %d" % (r, k), ref=ref)
            print("reference code n=%d row %d frame %d: E / E_y = %.2f" % (n, r, k, e))


# 11 ---- the drop-in class, with and without -DCSDR_CFFT_FP64
def build_cfft_host(tmp_path, tag, flags):
    from cutesdr_amd import _build
    _build.build()
    exe = str(tmp_path / ("cfft_host_" + tag))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "cutesdr_amd", "dropin"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cfft_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "cutesdr_amd"), "-lcutesdr_mi",
                           "-Wl,-rpath," + os.path.join(ROOT, "cutesdr_amd")])
    return exe


def test_dropin_cfft(ca, tmp_path):
    n = 4096
    seed = P.seed_of(n, 0)
    x = P.probe(n, seed)
    x32 = P32.probe(n, seed)
    np.array(x).tofile(tmp_path / "in64.bin")
    x32.astype(np.complex128).tofile(tmp_path / "in32.bin")
    outs = {}
    for tag, flags, src in (("fp64", ("-DCSDR_CFFT_FP64",), "in64.bin"), ("fp32", (), "in32.bin")):
        exe = build_cfft_host(tmp_path, tag, flags)
        r = subprocess.run([exe, str(tmp_path / src), str(tmp_path / (tag + ".bin"))], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        outs[tag] = np.fromfile(tmp_path / (tag + ".bin"), dtype=np.complex128)
        assert outs[tag].shape == (n,)
    e, _ = P.check_frame(outs["fp64"], n, seed, +1, "drop-in with CSDR_CFFT_FP64")
    e32 = P32.check_frame(outs["fp32"], n, seed, +1, "drop-in without the macro")
    assert (outs["fp32"].view(np.float64).astype(np.float32).astype(np.float64) == outs["fp32"].view(np.float64)).all(), "fp32 words expected"
    print("drop-in n=%d: E / E_y = %.2f with the macro (fp64 rule), %.2f without (fp32 rule)" % (n, e, e32))
