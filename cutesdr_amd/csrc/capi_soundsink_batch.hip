// capi_soundsink_batch.hip -- C ABI of the batch sound sink: C independent CSoundOut sinks (reference
// interface/soundout.cpp:155-468, non-blocking mode) behind the batched chain, resampled together on the device.
// Every receiver keeps its own user rate, volume, resampler state (time accumulator and 28-sample history, on the
// device), queue and rate loop (soundsink_queue.hpp, the single sink's rules).  A put builds each receiver's rate and
// gain under that receiver's lock, makes one launch on the caller's stream (soundsink_batch_kernels.hip) that writes
// int16 and the per-row counts straight into pinned, device-mapped staging, waits on that stream, and pushes each
// receiver's samples into its queue under its lock.  One producer thread puts; any number of consumer threads get,
// at most one per receiver at a time.  Blocking mode is left out: one full queue would stall every receiver.
#include "capi_common.hpp"
#include "resampler_kernels.h"
#include "soundsink_batch_kernels.h"
#include "soundsink_queue.hpp"
#include <memory>
#include <mutex>
#include <vector>

using namespace csdr;
using csdr::sinkq::kQ;

namespace {
struct Receiver {
    SinkQueue qs;
    std::mutex mu;                       // m_Mutex of this receiver: queue, rate loop, rate and gain
};
}

struct csdr_soundsink_batch {
    int device = 0, channels = 0, stereo = 0;
    std::unique_ptr<Receiver[]> rx;
    std::mutex mu_put;                   // one put at a time owns the device state and the staging
    float *d_sinc = nullptr, *d_hist = nullptr;      // hist: [channels][RS_PERIODS * w]
    double *d_t = nullptr;               // [channels] m_FloatTime
    SinkBatchParam *h_par = nullptr, *d_par = nullptr;   // pinned, device-mapped: [channels]
    short *h_out = nullptr, *d_out = nullptr;        // pinned, device-mapped: [channels][kQ * w]
    int *h_cnt = nullptr, *d_cnt = nullptr;          // pinned, device-mapped: [channels]
    bool tapped = false;                 // a put has filled the staging (get_tap)
};

static int sb_mapped(void **h, void **d, size_t bytes)
{
    if (hipHostMalloc(h, bytes, hipHostMallocDefault) != hipSuccess)
        return fail(CSDR_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
    memset(*h, 0, bytes);
    CSDR_HIP(hipHostGetDevicePointer(d, *h, 0));
    return CSDR_OK;
}

static int sb_alloc(csdr_soundsink_batch *s)
{
    const int w = s->stereo ? 2 : 1;
    const size_t hb = sizeof(float) * (size_t)s->channels * RS_PERIODS * w;
    if (rs_build_sinc(&s->d_sinc) != CSDR_OK) return CSDR_EHIP;
    CSDR_HIP(hipMalloc((void **)&s->d_hist, hb));
    CSDR_HIP(hipMemset(s->d_hist, 0, hb));
    CSDR_HIP(hipMalloc((void **)&s->d_t, sizeof(double) * s->channels));
    CSDR_HIP(hipMemset(s->d_t, 0, sizeof(double) * s->channels));
    int rc;
    if ((rc = sb_mapped((void **)&s->h_par, (void **)&s->d_par, sizeof(SinkBatchParam) * s->channels)) != CSDR_OK) return rc;
    if ((rc = sb_mapped((void **)&s->h_out, (void **)&s->d_out, sizeof(short) * (size_t)s->channels * kQ * w)) != CSDR_OK) return rc;
    if ((rc = sb_mapped((void **)&s->h_cnt, (void **)&s->d_cnt, sizeof(int) * s->channels)) != CSDR_OK) return rc;
    CSDR_HIP(hipDeviceSynchronize());    // creation only: the zeroed state is on the device before the first put
    return CSDR_OK;
}

static Receiver *sb_rx(csdr_soundsink_batch *s, int channel)
{
    if (!s || channel < 0 || channel >= s->channels) { fail(CSDR_EINVAL, "bad handle or channel"); return nullptr; }
    return &s->rx[channel];
}

extern "C" {

/* C x CSoundOut::CSoundOut (soundout.cpp:60-76) */
csdr_soundsink_batch *csdr_soundsink_batch_create(int device, int channels, int stereo)
{
    if (channels < 1) { fail(CSDR_EINVAL, "channels >= 1"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_soundsink_batch *s = new csdr_soundsink_batch();
    s->device = device; s->channels = channels; s->stereo = stereo != 0;
    s->rx.reset(new Receiver[channels]);
    for (int c = 0; c < channels; c++) s->rx[c].qs.init(s->stereo);
    if (sb_alloc(s) != CSDR_OK) {
        const std::string e = last_error_ref();
        csdr_soundsink_batch_destroy(s);
        fail(CSDR_EHIP, "%s", e.c_str());
        return nullptr;
    }
    return s;
}
void csdr_soundsink_batch_destroy(csdr_soundsink_batch *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->d_sinc) (void)hipFree(s->d_sinc);
    if (s->d_hist) (void)hipFree(s->d_hist);
    if (s->d_t) (void)hipFree(s->d_t);
    if (s->h_par) (void)hipHostFree(s->h_par);
    if (s->h_out) (void)hipHostFree(s->h_out);
    if (s->h_cnt) (void)hipHostFree(s->h_cnt);
    delete s;
}
/* CSoundOut::ChangeUserDataRate (:155-175) of one receiver, or of every receiver for channel < 0 */
int csdr_soundsink_batch_change_user_data_rate(csdr_soundsink_batch *s, int channel, double rate)
{
    if (!s || !(rate > 0.0) || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    for (int c = channel < 0 ? 0 : channel; c < (channel < 0 ? s->channels : channel + 1); c++) {
        std::lock_guard<std::mutex> lock(s->rx[c].mu);
        s->rx[c].qs.change_user_data_rate(rate);
    }
    return CSDR_OK;
}
/* CSoundOut::SetVolume (:180-189) of one receiver, or of every receiver for channel < 0 */
int csdr_soundsink_batch_set_volume(csdr_soundsink_batch *s, int channel, int vol)
{
    if (!s || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    for (int c = channel < 0 ? 0 : channel; c < (channel < 0 ? s->channels : channel + 1); c++) {
        std::lock_guard<std::mutex> lock(s->rx[c].mu);
        s->rx[c].qs.set_volume(vol);
    }
    return CSDR_OK;
}
/* CSoundOut::PutOutQueue, non-blocking branch (:196-305), for every receiver in one launch */
int csdr_soundsink_batch_put(csdr_soundsink_batch *s, const float *d_in, long long in_stride, const int *n_in,
                             int *n_out, void *stream)
{
    if (!s || !n_in || in_stride < 0) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> producer(s->mu_put);
    bool any = false;
    for (int c = 0; c < s->channels; c++) {
        const int n = n_in[c];
        if (n < 0 || n > sinkq::kMaxIn) return fail(CSDR_EINVAL, "row %d: %d samples (0..%d)", c, n, sinkq::kMaxIn);
        if (n > in_stride) return fail(CSDR_EINVAL, "row %d: %d samples > in_stride %lld", c, n, in_stride);
        any |= n > 0;
    }
    if (any && !d_in) return fail(CSDR_EINVAL, "bad argument");
    // the staging is free: the previous put waited for its launch
    for (int c = 0; c < s->channels; c++) {
        double rate, gain;
        {   // the rate and the gain as they are now: get() and the setters change them under the same mutex
            std::lock_guard<std::mutex> lock(s->rx[c].mu);
            rate = s->rx[c].qs.rate();
            gain = s->rx[c].qs.gain;
        }
        const int n = n_in[c];
        if (n > 0 && (double)n / rate + 8.0 > (double)kQ)
            return fail(CSDR_EINVAL, "row %d: call too long for the %d-entry queue", c, kQ);
        s->h_par[c].rate = rate; s->h_par[c].gain = (float)gain; s->h_par[c].n = n;
    }
    if (!any) {
        for (int c = 0; c < s->channels; c++) { s->h_cnt[c] = 0; if (n_out) n_out[c] = 0; }    // (the tap of an empty put is empty)
        s->tapped = true;
        return CSDR_OK;
    }
    const int w = s->stereo ? 2 : 1;
    CSDR_HIP(hipSetDevice(s->device));
    SinkBatchArgs a;
    a.in = d_in; a.in_stride = (long)in_stride * w; a.hist = s->d_hist; a.t = s->d_t; a.sinc = s->d_sinc; a.par = s->d_par;
    a.out = s->d_out; a.out_stride = (long)kQ * w; a.count = s->d_cnt; a.out_cap = kQ; a.channels = s->channels;
    CSDR_HIP(soundsink_batch_launch(a, s->stereo, (hipStream_t)stream));
    CSDR_HIP(hipStreamSynchronize((hipStream_t)stream));
    s->tapped = true;
    for (int c = 0; c < s->channels; c++) {
        if (n_in[c] == 0) { if (n_out) n_out[c] = 0; continue; }
        const int k = s->h_cnt[c];
        {
            std::lock_guard<std::mutex> lock(s->rx[c].mu);
            s->rx[c].qs.push(s->h_out + (size_t)c * kQ * w, 0, k);
        }
        if (n_out) n_out[c] = k;
    }
    return CSDR_OK;
}
/* PROFILE_5 (soundout.cpp:207, :265): the staging the last put filled, as it is -- nothing is copied */
int csdr_soundsink_batch_get_tap(csdr_soundsink_batch *s, const short **d_rows, long long *stride, const int **d_counts)
{
    if (!s || !d_rows || !stride || !d_counts) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> producer(s->mu_put);
    if (!s->tapped) return fail(CSDR_ESTATE, "get_tap: no put yet");
    *d_rows = s->d_out; *stride = kQ; *d_counts = s->d_cnt;
    return CSDR_OK;
}
/* CSoundOut::GetOutQueue (:311-375 mono, :381-445 stereo) of one receiver: n samples, or n L/R pairs */
int csdr_soundsink_batch_get(csdr_soundsink_batch *s, int channel, int n, short *out)
{
    Receiver *r = sb_rx(s, channel);
    if (!r || n < 0 || (n > 0 && !out)) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(r->mu);
    r->qs.get(n, out);
    return n;
}
double csdr_soundsink_batch_get_rate_correction(csdr_soundsink_batch *s, int channel)
{
    Receiver *r = sb_rx(s, channel);
    if (!r) return 0.0;
    std::lock_guard<std::mutex> lock(r->mu);
    return r->qs.rate_corr;
}
double csdr_soundsink_batch_get_ave_level(csdr_soundsink_batch *s, int channel)
{
    Receiver *r = sb_rx(s, channel);
    if (!r) return 0.0;
    std::lock_guard<std::mutex> lock(r->mu);
    return r->qs.ave_level;
}
int csdr_soundsink_batch_get_level(csdr_soundsink_batch *s, int channel)
{
    Receiver *r = sb_rx(s, channel);
    if (!r) return CSDR_EINVAL;
    std::lock_guard<std::mutex> lock(r->mu);
    return r->qs.level;
}
int csdr_soundsink_batch_get_ppm_error(csdr_soundsink_batch *s, int channel)
{
    Receiver *r = sb_rx(s, channel);
    if (!r) return 0;
    std::lock_guard<std::mutex> lock(r->mu);
    return r->qs.ppm;
}

}  // extern "C"
