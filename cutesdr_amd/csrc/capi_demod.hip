// capi_demod.hip -- C ABI of the full receive chain, CDemodulator (dsp/demodulator.h:56-100), as the single-channel host
// object that mirrors CDemodulator::ProcessData call for call.  The chain itself: chain_core.hpp; the batched
// multi-channel form: capi_demod_batch.hip.
#include "chain_core.hpp"
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <vector>

using namespace csdr;

/* =================== single-channel host form: CDemodulator drop-in =================== */
struct csdr_demod {
    ChainCore k;
    ChanCfg c;
    double in_rate = 0.0;
    int limit = 1000;                   // m_InBufLimit (demodulator.cpp:54)
    // m_pDemodInBuf as fp32 pairs in PINNED memory, two windows used in turn: while window w is on its way to the
    // device and through the chain (asynchronous, on the object's stream), the caller's next samples are converted
    // into window w^1.  The host waits for the GPU only when a pass is due to RETURN samples (a whole hop of audio),
    // as the reference's call pattern demands; passes that only fill the filter return at once.
    // ZERO COPY (round 5): the pinned windows are mapped into the device's address space and the down-converter reads
    // them over PCIe in its own loads, the post-chain writes the audio into the pinned output buffer -- no copy engine, no
    // cross-engine dependency between a copy and the kernel behind it (9 us of copy + 10 us until the kernel started, per
    // pass, and a 4 us copy kernel on the way back).  CSDR_HOST_ZEROCOPY=0 restores the copies (d_in / d_out).
    bool zero_copy = true;
    PinnedBuf win[2], pin_out, pin_out2;
    // DEFERRED output (csdr_demod_set_deferred): a pass that is due to return samples returns the PREVIOUS such pass's
    // instead -- already complete, so the call does not wait -- and leaves its own in the other pinned buffer: the chain's
    // pass runs while the caller converts the next window (host-form throughput x1.4-1.6), every sample comes out one
    // window (10 ms at 2 MSPS) later, the last window's by csdr_demod_flush_*.
    bool deferred = false;
    int out_cur = 0;
    int pend_k = 0, pend_buf = 0; bool pend_stereo = false;
    hipEvent_t ev_out[2] = {nullptr, nullptr};
    int cur = 0;
    bool win_busy[2] = {false, false};
    hipEvent_t ev_win[2] = {nullptr, nullptr};   // window w's copy to the device has left the pinned buffer
    hipStream_t s = nullptr;
    int pos = 0;
    float *d_in = nullptr, *d_out = nullptr;
    size_t cap_in = 0, cap_out = 0;
    // stage taps (csdr_demod_set_taps): per pass either the callback or the per-profile accumulators
    csdr_tap_fn tap_fn = nullptr; void *tap_user = nullptr;
    std::vector<double> tap_acc[4];
    std::vector<float> tap_tmp;
    ~csdr_demod()
    {
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        for (hipEvent_t e : ev_win) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_out) if (e) (void)hipEventDestroy(e);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
    }
};

extern "C" {

csdr_demod *csdr_demod_create(int device, int fastfir_n)
{
    if (!device_ok(device)) return nullptr;
    csdr_demod *d = new csdr_demod();
    if (d->k.init(device, 1, fastfir_n) != CSDR_OK) { delete d; return nullptr; }
    bool ok = hipStreamCreateWithFlags(&d->s, hipStreamNonBlocking) == hipSuccess;
    for (auto &e : d->ev_win) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    for (auto &e : d->ev_out) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!ok) { fail(CSDR_EHIP, "stream / event creation failed"); delete d; return nullptr; }
    csdr_downconvert_batch_set_cw_offset(d->k.dc, 0, 0.0);      // ctor: SetDemodFreq(0.0)
    csdr_downconvert_batch_set_frequency(d->k.dc, 0, 0.0);
    d->zero_copy = !(getenv("CSDR_HOST_ZEROCOPY") && atoi(getenv("CSDR_HOST_ZEROCOPY")) == 0);
    return d;
}
void csdr_demod_destroy(csdr_demod *d) { delete d; }

/* CDemodulator::SetInputSampleRate (demodulator.cpp:92-99) */
int csdr_demod_set_input_rate(csdr_demod *d, double rate)
{
    if (!d) return fail(CSDR_EINVAL, "bad handle");
    if (d->s) CSDR_HIP(hipStreamSynchronize(d->s));   // control plane: a pass that returned no samples may still be in flight
    if (!(rate > 0.0) || !std::isfinite(rate)) return fail(CSDR_EINVAL, "input rate %g", rate);
    if (d->in_rate != rate) {
        const double r = csdr_downconvert_batch_set_data_rate(d->k.dc, 0, rate, d->c.want_bw);
        if (r < 0) return CSDR_EHIP;                      // (in_rate keeps its old value: the same call again is not a no-op)
        d->in_rate = rate;
        d->c.out_rate = r;
        // Everything else stays as it is until the next SetDemod: filter taps, AGC constants and rings, m_InBufLimit and
        // the demodulator object (built for the OLD output rate; a same-mode SetDemod does not rebuild it,
        // demodulator.cpp:111-137).  Only the S-meter follows at once: it is handed m_OutputRate with every pass (:183)
        int rc = d->k.pc.smeter_rate_set(0, r);
        if (rc) return rc;
    }
    return CSDR_OK;
}
/* CDemodulator::SetDemod (demodulator.cpp:107-157) */
int csdr_demod_set_demod(csdr_demod *d, int mode, const csdr_demod_info *info)
{
    if (!d || !info || mode < 0 || mode > 6) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(d->k.device)) return CSDR_EHIP;
    if (d->s) CSDR_HIP(hipStreamSynchronize(d->s));   // control plane: a pass that returned no samples may still be in flight
    DemodInfo di;
    memcpy(&di, info, sizeof(di));
    int rc = apply_set_demod(d->k, 0, d->c, d->in_rate, mode, di);
    if (rc) return rc;
    d->limit = (int)((d->c.out_rate / 100.0) * d->in_rate / d->c.out_rate);
    d->limit &= 0xFFFFFF00;
    return CSDR_OK;
}
/* CDemodulator::SetDemodFreq (demodulator.h:68-69) */
int csdr_demod_set_freq(csdr_demod *d, double freq)
{
    if (!d) return fail(CSDR_EINVAL, "bad handle");
    csdr_downconvert_batch_set_cw_offset(d->k.dc, 0, d->c.cw_off);
    return csdr_downconvert_batch_set_frequency(d->k.dc, 0, freq);
}
double csdr_demod_get_output_rate(csdr_demod *d) { return d ? d->c.out_rate : 0.0; }
double csdr_demod_get_smeter_peak(csdr_demod *d) { return d ? d->k.pc.smeter_peak(0) : 0.0; }
double csdr_demod_get_smeter_ave(csdr_demod *d) { return d ? d->k.pc.smeter_ave(0) : 0.0; }
int csdr_demod_get_buf_limit(csdr_demod *d) { return d ? d->limit : fail(CSDR_EINVAL, "bad handle"); }
/* the chain's test points (dsp/demodulator.cpp:175,180,187,208): see include/cutesdr_mi.h */
int csdr_demod_set_taps(csdr_demod *d, int mask, csdr_tap_fn fn, void *user)
{
    if (d && mask && d->deferred) return fail(CSDR_ESTATE, "stage taps and deferred output exclude each other");
    if (!d || mask < 0 || mask > 15) return fail(CSDR_EINVAL, "bad argument");
    if (d->s) CSDR_HIP(hipStreamSynchronize(d->s));
    d->k.taps = mask; d->tap_fn = fn; d->tap_user = user;
    for (auto &a : d->tap_acc) a.clear();
    return CSDR_OK;
}
int csdr_demod_get_tap(csdr_demod *d, int profile, double *out, int cap)
{
    if (!d || profile < 1 || profile > 4 || cap < 0 || (cap && !out)) return fail(CSDR_EINVAL, "bad argument");
    std::vector<double> &a = d->tap_acc[profile - 1];
    if ((size_t)cap < a.size()) return fail(CSDR_EINVAL, "tap %d holds %zu doubles, room for %d", profile, a.size(), cap);
    const int n = (int)a.size();
    if (n) memcpy(out, a.data(), sizeof(double) * (size_t)n);
    a.clear();
    return n;
}

/* CDemodulator::ProcessData (demodulator.cpp:163-215 mono, :221-273 stereo).  Every inner pass
 * writes its output at out[0] and the return value is the SUM over the passes, exactly as the
 * reference does; append != 0 selects the batch-harness form that appends. */
// the stage taps of the pass that has just been issued (csdr_demod_set_taps): waits for it, then per profile the callback or
// the accumulator, in the reference's order (demodulator.cpp:175,180,187,208)
static int demod_emit_taps(csdr_demod *d, int k, bool stereo)
{
    ChainCore &c = d->k;
    CSDR_HIP(hipStreamSynchronize(d->s));
    auto emit = [&](int profile, const float *dev_or_host, bool on_device, int n, bool cpx) -> int {
        if (!(c.taps & (1 << (profile - 1)))) return CSDR_OK;
        const size_t nf = (size_t)n * (cpx ? 2 : 1);
        d->tap_tmp.resize(nf ? nf : 1);
        if (nf) {
            if (on_device) CSDR_HIP(hipMemcpy(d->tap_tmp.data(), dev_or_host, nf * 4, hipMemcpyDeviceToHost));
            else memcpy(d->tap_tmp.data(), dev_or_host, nf * 4);
        }
        if (d->tap_fn) {
            std::vector<double> v(nf ? nf : 1);
            for (size_t i = 0; i < nf; i++) v[i] = (double)d->tap_tmp[i];
            d->tap_fn(d->tap_user, profile, n, v.data(), cpx ? 1 : 0, d->c.out_rate);
        } else {
            std::vector<double> &a = d->tap_acc[profile - 1];
            for (size_t i = 0; i < nf; i++) a.push_back((double)d->tap_tmp[i]);
        }
        return CSDR_OK;
    };
    int rc;
    if ((rc = emit(1, c.d_tap1, true, c.tap1_n, true))) return rc;
    if ((rc = emit(2, c.d_filt, true, k, true))) return rc;
    if ((rc = emit(3, c.d_agc, true, k, true))) return rc;
    const float *audio = d->zero_copy ? d->pin_out.p : d->d_out;
    return emit(4, audio, !d->zero_copy, k, stereo);
}
// deferred mode: the pending pass's samples (if any) to `out`; returns their count and clears the slot
static int demod_take_pending(csdr_demod *d, double *out)
{
    const int k = d->pend_k;
    if (k <= 0) return 0;
    CSDR_HIP(hipEventSynchronize(d->ev_out[d->pend_buf]));
    const PinnedBuf &pb = d->pend_buf ? d->pin_out2 : d->pin_out;
    cvt_to_f64(out, pb.p, d->pend_stereo ? 2 * (size_t)k : (size_t)k);
    d->pend_k = 0;
    return k;
}
static int demod_process(csdr_demod *d, int n, const double *in_iq, double *out, bool stereo, bool append)
{
    if (!d || n < 0 || (n && (!in_iq || !out))) return fail(CSDR_EINVAL, "bad argument");
    if (d->limit <= 0 || d->limit > refc::DEMOD_MAX_INBUFSIZE) return fail(CSDR_ESTATE, "input buffer limit %d out of range", d->limit);
    if (!device_ok(d->k.device)) return CSDR_EHIP;
    int ret = 0;
    for (int i = 0; i < n; ) {
        PinnedBuf &w = d->win[d->cur];
        // the samples that fit before the window is full (at least one: a limit lowered by SetDemod below the fill
        // runs the pass at the next sample, as `if (m_InBufPos >= m_InBufLimit)` does, demodulator.cpp:169-174)
        int take = d->limit - d->pos;
        if (take < 1) take = 1;
        if (take > n - i) take = n - i;
        if (d->win_busy[d->cur]) { CSDR_HIP(hipEventSynchronize(d->ev_win[d->cur])); d->win_busy[d->cur] = false; }
        // (a whole window at once: grown step by step, a window filled in 256-sample calls was reallocated -- pinned
        // malloc, copy, free -- some ten times during its first fill, on the per-datagram path)
        const size_t fill = (size_t)d->pos + take;
        const size_t want = 2 * (fill > (size_t)d->limit ? fill : (size_t)d->limit);
        if (want > w.cap && d->zero_copy) CSDR_HIP(hipStreamSynchronize(d->s));   // nothing may still be reading the old buffer
        int rc = w.reserve(want);
        if (rc) return rc;
        cvt_to_f32(w.p + 2 * (size_t)d->pos, in_iq + 2 * (size_t)i, 2 * (size_t)take);
        d->pos += take; i += take;
        if (d->pos < d->limit) break;                     // the call's samples are in; the window is not full yet
        const int len = d->pos;
        d->pos = 0;
        const size_t need_out = (size_t)len + d->k.L;
        const float *chain_in = nullptr;
        float *chain_out = nullptr;
        size_t out_stride = 0;
        // (deferred: the two output buffers in turn -- the one written now last held the pass before the pending one)
        const int ob = d->deferred ? d->out_cur : 0;
        PinnedBuf &pout = ob ? d->pin_out2 : d->pin_out;
        if (d->zero_copy) {
            if (2 * need_out > pout.cap) {
                CSDR_HIP(hipStreamSynchronize(d->s));
                if ((rc = pout.reserve(2 * need_out))) return rc;
            }
            void *pi = nullptr, *po = nullptr;
            CSDR_HIP(hipHostGetDevicePointer(&pi, w.p, 0));
            CSDR_HIP(hipHostGetDevicePointer(&po, pout.p, 0));
            chain_in = (const float *)pi; chain_out = (float *)po; out_stride = pout.cap / 2;
        } else {
            if ((size_t)len > d->cap_in) {
                CSDR_HIP(hipStreamSynchronize(d->s));
                if (d->d_in) (void)hipFree(d->d_in);
                d->d_in = nullptr; d->cap_in = 0;
                CSDR_HIP(hipMalloc((void **)&d->d_in, (size_t)len * 8));
                d->cap_in = len;
            }
            if (need_out > d->cap_out) {
                CSDR_HIP(hipStreamSynchronize(d->s));
                if (d->d_out) (void)hipFree(d->d_out);
                d->d_out = nullptr; d->cap_out = 0;
                CSDR_HIP(hipMalloc((void **)&d->d_out, need_out * 8));
                d->cap_out = need_out;
            }
            // window -> device -> chain, all on the object's stream (d_in is reused in stream order)
            CSDR_HIP(hipMemcpyAsync(d->d_in, w.p, (size_t)len * 8, hipMemcpyHostToDevice, d->s));
            chain_in = d->d_in; chain_out = d->d_out; out_stride = d->cap_out;
        }
        const int wcur = d->cur;
        d->cur ^= 1;
        const int k = d->k.step(ChainIn{chain_in, len, nullptr, len, nullptr, 0, nullptr},
                                ChainOut{chain_out, (long)out_stride, nullptr, stereo}, d->s);
        // the window is free again when the down-converter (zero copy) / the copy has read it: the whole pass, here
        CSDR_HIP(hipEventRecord(d->ev_win[wcur], d->s));
        d->win_busy[wcur] = true;
        if (k < 0) return k;
        if (d->k.taps) { const int rct = demod_emit_taps(d, k, stereo); if (rct) return rct; }
        if (k > 0 && d->deferred) {
            // this pass's samples stay where they are; the pending pass's -- complete, or nearly -- are handed over
            const size_t nf = stereo ? 2 * (size_t)k : (size_t)k;
            if (!d->zero_copy) {
                if (nf > pout.cap) { CSDR_HIP(hipStreamSynchronize(d->s)); if ((rc = pout.reserve(nf))) return rc; }
                CSDR_HIP(hipMemcpyAsync(pout.p, d->d_out, nf * 4, hipMemcpyDeviceToHost, d->s));
            }
            CSDR_HIP(hipEventRecord(d->ev_out[ob], d->s));
            const int got = demod_take_pending(d, append ? out + (d->pend_stereo ? 2 : 1) * (size_t)ret : out);
            if (got < 0) return got;
            d->pend_k = k; d->pend_buf = ob; d->pend_stereo = stereo;
            d->out_cur ^= 1;
            ret += got;
            continue;
        }
        if (k > 0) {                                      // a pass that returns samples: the one wait of this call
            const size_t nf = stereo ? 2 * (size_t)k : (size_t)k;
            if (!d->zero_copy) {
                if ((rc = d->pin_out.reserve(nf))) return rc;
                CSDR_HIP(hipMemcpyAsync(d->pin_out.p, d->d_out, nf * 4, hipMemcpyDeviceToHost, d->s));
            }
            CSDR_HIP(hipStreamSynchronize(d->s));             // (polling hipStreamQuery first: measured +-0)
            cvt_to_f64(append ? out + (stereo ? 2 : 1) * (size_t)ret : out, d->pin_out.p, nf);
        }
        ret += k;
    }
    return ret;
}
int csdr_demod_process_mono(csdr_demod *d, int n, const double *in_iq, double *out)
{ return demod_process(d, n, in_iq, out, false, false); }
int csdr_demod_process_stereo(csdr_demod *d, int n, const double *in_iq, double *out_iq)
{ return demod_process(d, n, in_iq, out_iq, true, false); }
int csdr_demod_process_mono_append(csdr_demod *d, int n, const double *in_iq, double *out)
{ return demod_process(d, n, in_iq, out, false, true); }
int csdr_demod_set_deferred(csdr_demod *d, int on)
{
    if (!d) return fail(CSDR_EINVAL, "bad handle");
    if (on && d->k.taps) return fail(CSDR_ESTATE, "stage taps and deferred output exclude each other");
    if (!on && d->pend_k > 0) return fail(CSDR_ESTATE, "a pass is pending: csdr_demod_flush first");
    d->deferred = on != 0;
    return CSDR_OK;
}
int csdr_demod_flush(csdr_demod *d, double *out, int cap)
{
    if (!d || cap < 0 || (cap && !out)) return fail(CSDR_EINVAL, "bad argument");
    const int need = d->pend_stereo ? 2 * d->pend_k : d->pend_k;
    if (need > cap) return fail(CSDR_EINVAL, "the pending pass holds %d values, room for %d", need, cap);
    if (!device_ok(d->k.device)) return CSDR_EHIP;
    return demod_take_pending(d, out);
}

/* internal (bench.py `host_form`, tests; not in the public header): the reference's call pattern in one C loop --
 * n_total samples handed over in calls of call_len (one datagram: 240 / 256 samples, interface/sdrinterface.cpp:903),
 * every call's audio appended at out.  Returns the audio samples produced.  Saves the measurement the per-call cost
 * of the Python binding, nothing else. */
int csdr__demod_process_calls(csdr_demod *d, int n_total, int call_len, const double *in_iq, double *out)
{
    if (!d || call_len < 1 || n_total < 0 || (n_total && (!in_iq || !out))) return fail(CSDR_EINVAL, "bad argument");
    int total = 0;
    for (int i = 0; i < n_total; i += call_len) {
        const int n = n_total - i < call_len ? n_total - i : call_len;
        const int k = demod_process(d, n, in_iq + 2 * (size_t)i, out + total, false, true);
        if (k < 0) return k;
        total += k;
    }
    return total;
}

}  // extern "C"
