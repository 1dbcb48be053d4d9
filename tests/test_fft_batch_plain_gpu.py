"""csdr_fft_batch_fwd / _rev -- CFft::FwdFFT / RevFFT of every frame of every row on the device, 512 ... 65536 points --
held to the rule of fft_plain_ref.py: per frame E <= m E_y, E the per-bin relative error against the fp64 oracle on a
flat-spectrum probe, E_y the same figure of scipy's fp32 transform, m = 4 (6.43 at 16384 points).

Each size is a kernel configuration of its own (512 / 1024: several frames per workgroup; 2048 ... 16384: one workgroup per
frame; 32768 / 65536: the four-step form in two launches through the object's work buffer), so every test runs all eight."""
import ctypes as C

import numpy as np
import pytest

import fft_plain_ref as P

pytestmark = pytest.mark.gpu

SENT = np.complex64(-12345.5 + 54321.25j)


@pytest.fixture(scope="module")
def ca():
    import cutesdr_amd
    return cutesdr_amd


_objs = {}


def batch(ca, channels, n):
    """one object per channel count, set to n points"""
    if channels not in _objs:
        _objs[channels] = ca.FftBatch(channels)
    fb = _objs[channels]
    if fb.size() != n:
        fb.set_params(n, False, 0.0, P.FS)
    return fb


def frames_of(n, rows, nframes, pool=None):
    """(x [rows, nframes, n] complex64, seeds [rows, nframes]); pool: that many distinct probes, neighbours different"""
    seeds = np.array([[P.seed_of(n, (r * nframes + k) % pool if pool else r * nframes + k) for k in range(nframes)]
                      for r in range(rows)])
    x = np.stack([np.stack([P.probe(n, int(s)) for s in row]) for row in seeds])
    return x, seeds


def run(ca, fb, x, sign, in_stride=None, out_stride=None, in_place=False):
    """the call on rows of in_stride / out_stride samples -> (out rows [rows, out_stride], input rows after the call)"""
    rows, nframes, n = x.shape
    in_stride = in_stride or nframes * n
    out_stride = in_stride if in_place else (out_stride or nframes * n)
    hin = np.full((rows, in_stride), SENT, dtype=np.complex64)
    hin[:, :nframes * n] = x.reshape(rows, -1)
    din = ca.host.DeviceBuffer(hin.nbytes)
    din.upload(hin)
    dout = din
    if not in_place:
        dout = ca.host.DeviceBuffer(rows * out_stride * 8)
        dout.upload(np.full((rows, out_stride), SENT, dtype=np.complex64))
    (fb.fwd_ptr if sign > 0 else fb.rev_ptr)(din.ptr, in_stride, dout.ptr, out_stride, nframes)
    ca.host.sync()
    out = dout.download(np.complex64, rows * out_stride).reshape(rows, out_stride)
    back = din.download(np.complex64, rows * in_stride).reshape(rows, in_stride)
    din.free()
    if not in_place:
        dout.free()
    return out, (back, hin)


def check_all(out, seeds, n, sign, what):
    rows, nframes = seeds.shape
    worst = 0.0
    for r in range(rows):
        for k in range(nframes):
            worst = max(worst, P.check_frame(out[r, k * n:(k + 1) * n], n, int(seeds[r, k]), sign, "%s row %d frame %d" % (what, r, k)))
    print("%s n=%d sign=%+d: worst E / E_y = %.2f (m = %g)" % (what, n, sign, worst, P.margin(n)))
    return worst


# 1 ---- every size, both signs, out of place, padded rows
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_every_size_out_of_place(ca, n, sign):
    x, seeds = frames_of(n, 3, 2)
    out, (back, hin) = run(ca, batch(ca, 3, n), x, sign, in_stride=2 * n + 8, out_stride=2 * n + 24)
    check_all(out, seeds, n, sign, "out of place")
    assert (P.words(out[:, 2 * n:]) == P.words(np.full((3, 24), SENT))).all(), "the padding of d_out was written"
    assert (P.words(back) == P.words(hin)).all(), "d_in was changed"


# 2 ---- index order
def impulse_positions(n):
    return [1, n // 2 + 3, n - 1] + ([12345] if n >= 32768 else [])      # 12345: a multiple of neither 256 nor 128


@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_index_order(ca, n, sign):
    ms = impulse_positions(n)
    assert all(0 < m < n for m in ms) and (n < 32768 or (ms[-1] % 256 and ms[-1] % 128))
    x = np.zeros((len(ms), 1, n), dtype=np.complex64)
    for i, m in enumerate(ms):
        x[i, 0, m] = 3000.0
    out, _ = run(ca, batch(ca, len(ms), n), x, sign)
    _, e_y = P.reference(n, P.seed_of(n, 0), sign)
    for i, m in enumerate(ms):
        err = np.abs(out[i].astype(np.complex128) - P.impulse_ref(n, m, sign)).max()
        print("impulse n=%d m=%d sign=%+d: %.3g of the allowed %.3g" % (n, m, sign, err, P.margin(n) * e_y * 3000.0))
        assert err <= P.margin(n) * e_y * 3000.0, (n, m, sign, err)


# 3 ---- in place = out of place
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_in_place_equals_out_of_place(ca, n, sign):
    x, _ = frames_of(n, 2, 2)
    fb = batch(ca, 2, n)
    a, _ = run(ca, fb, x, sign)
    b, _ = run(ca, fb, x, sign, in_place=True)
    assert (P.words(a) == P.words(b)).all()


# 4 ---- position independence
@pytest.mark.parametrize("n", P.SIZES)
def test_position_independence(ca, n):
    x, _ = frames_of(n, 3, 2)
    many, _ = run(ca, batch(ca, 3, n), x, +1)
    one, _ = run(ca, batch(ca, 1, n), x[2:3, 1:2], +1)
    assert (P.words(one[0]) == P.words(many[2, n:])).all()


# 5 ---- workgroup tails and the work buffer's groups
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n,nframes", [(512, 67), (1024, 33)])
def test_workgroup_tails(ca, n, nframes, sign):
    x, seeds = frames_of(n, 5, nframes, pool=8)
    assert (5 * nframes) % 4, "the last workgroup must be short"
    out, (back, hin) = run(ca, batch(ca, 5, n), x, sign, out_stride=nframes * n + 8)
    check_all(out, seeds, n, sign, "tails")
    assert (P.words(out[:, nframes * n:]) == P.words(np.full((5, 8), SENT))).all()
    assert (P.words(back) == P.words(hin)).all()


def test_work_buffer_groups(ca):
    n = 32768
    fb = batch(ca, 4, n)
    g = fb.plain_group()
    assert 1 <= g <= 16, g
    x, seeds = frames_of(n, 4, g + 1, pool=8)
    out, _ = run(ca, fb, x, +1, out_stride=(g + 1) * n + 8)
    check_all(out, seeds, n, +1, "groups")
    assert (P.words(out[:, (g + 1) * n:]) == P.words(np.full((4, 8), SENT))).all()
    b, _ = run(ca, fb, x, +1, in_place=True)
    assert (P.words(b) == P.words(out[:, :(g + 1) * n])).all()


# 6 ---- round trip
@pytest.mark.parametrize("n", P.SIZES)
def test_round_trip(ca, n):
    x, seeds = frames_of(n, 2, 2)
    fb = batch(ca, 2, n)
    y, _ = run(ca, fb, x, +1)
    z, _ = run(ca, fb, y.reshape(2, 2, n), -1)
    for r in range(2):
        for k in range(2):
            s = int(seeds[r, k])
            e_y = max(P.reference(n, s, +1)[1], P.reference(n, s, -1)[1])
            err = np.abs(z[r, k * n:(k + 1) * n].astype(np.complex128) / n - x[r, k]).max()
            bound = 2 * P.margin(n) * e_y * P.k1_bins.rms(x[r, k])
            print("round trip n=%d: %.3g of the allowed %.3g" % (n, err, bound))
            assert err <= bound, (n, r, k, err, bound)


# 7 ---- the display state stays as it was, and the tables follow set_params
def test_display_state_untouched_and_tables_follow_set_params(ca):
    fb = ca.FftBatch(2)
    fb.set_params(4096, False, 0.0, P.FS)
    fb.set_ave(2)
    x, seeds = frames_of(4096, 2, 3)
    fb.put_display(x.reshape(2, -1))

    def state():
        ov, pix = fb.screen_all(100, 300, 0.0, -120.0, -20000, 20000)
        return [fb.ave_buf(0), fb.ave_buf(1), np.array([fb.total_count(0), fb.total_count(1)]), ov, pix]
    before = state()
    assert before[2].tolist() == [3, 3]
    for sign in P.SIGNS:
        out, _ = run(ca, fb, x, sign)
        check_all(out, seeds, 4096, sign, "beside the display")
    after = state()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for n in (32768, 512):
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
    fill = np.full(total, SENT, dtype=np.complex64)
    buf = ca.host.DeviceBuffer(fill.nbytes)
    other = ca.host.DeviceBuffer(fill.nbytes)
    buf.upload(fill)
    other.upload(fill)
    s = 2 * n + 16
    vp = C.c_void_p

    def call(f, d_in, in_stride, d_out, out_stride, nframes, fn=L.csdr_fft_batch_fwd):
        return fn(f, vp(d_in), in_stride, vp(d_out), out_stride, nframes, None)
    cases = {
        "NULL handle": (None, buf.ptr, s, other.ptr, s, 2),
        "NULL d_in": (fb.h, None, s, other.ptr, s, 2),
        "NULL d_out": (fb.h, buf.ptr, s, None, s, 2),
        "nframes < 0": (fb.h, buf.ptr, s, other.ptr, s, -1),
        "short in_stride": (fb.h, buf.ptr, 2 * n - 1, other.ptr, s, 2),
        "short out_stride": (fb.h, buf.ptr, s, other.ptr, 2 * n - 1, 2),
        "partial overlap": (fb.h, buf.ptr, s, buf.ptr + 8 * n, s, 2),
        "same base, other stride": (fb.h, buf.ptr, s, buf.ptr, s + 8, 2),
    }
    for fn in (L.csdr_fft_batch_fwd, L.csdr_fft_batch_rev):
        for what, args in cases.items():
            assert call(*args, fn=fn) == _capi.CSDR_EINVAL, what
        assert call(fb.h, buf.ptr, s, other.ptr, s, 0, fn=fn) == _capi.CSDR_OK
    ca.host.sync()
    for d in (buf, other):
        assert (P.words(d.download(np.complex64, total)) == P.words(fill)).all()
        d.free()


# 9 ---- against the reference's compiled code
@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", [512, 4096, 65536])
def test_against_the_reference_code(ca, n, sign):
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref is not built")
    x, seeds = frames_of(n, 3, 2)
    out, _ = run(ca, batch(ca, 3, n), x, sign)
    for r in range(3):
        for k in range(2):
            ref = oref.fft(x[r, k].astype(np.complex128), sign)
            P.check_frame(out[r, k * n:(k + 1) * n], n, int(seeds[r, k]), sign, "reference code row %d frame %d" % (r, k), ref=ref)


# ---- the host form
def test_host_form(ca):
    n = 1024
    fb = batch(ca, 3, n)
    x, seeds = frames_of(n, 3, 2)
    y = fb.fwd(x.reshape(3, -1))
    assert y.dtype == np.complex64 and y.shape == (3, 2 * n)
    check_all(y, seeds, n, +1, "host form")
    check_all(fb.rev(x.reshape(3, -1)), seeds, n, -1, "host form")
