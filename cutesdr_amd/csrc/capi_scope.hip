// capi_scope.hip -- C ABI of the batch test-bench scope: the time view of CTestBench::DisplayData with ChkForTrigger
// (reference gui/testbench.cpp:583-695, :819-898; slots :247-299; Reset :541-548, :555-565, :574; DrawTimePlot
// :973-999), one oscilloscope per receiver on the device.  The settings (sc::Chan) live on the host: a setter touches
// no device memory and waits for nothing; what it changes, a Reset and the re-arm included, travels with the next put
// in stream order.  Everything that depends on the data (positions, previous sample, trigger state and counters, skip
// counter, ring, screen, emit counter) lives on the device.  put() writes the settings of the call into one slot of a
// small ring of pinned buffers, copies the slot on the caller's stream and launches scope_kernels.hip behind it, as
// capi_testgen.hip does; the readers wait for the event of the last put only, on a stream of the object's own.
//
// The FFT view (the frequency branch of DisplayData :594-611 / :654-672, DrawFftPlot :1005-1068, OnEnablePeak :334-343,
// OnTimeDisplay :282-286) is per receiver too: set_time_display(..., 0) moves a receiver into it.  Its frame logic does
// not depend on the data, so position, skip counter and carry buffer of such a receiver are kept here on the host
// (sc::Chan) and the put hands the kernel the arithmetic progression of the call's used frames.
#include "capi_common.hpp"
#include "scope_kernels.h"
#include "ref_constants.hpp"
#include <cmath>
#include <mutex>
#include <vector>

using namespace csdr;
using sc::Chan;
using sc::ChanParam;
using sc::ChanState;

namespace {
constexpr int kRing = 16;
constexpr int kMaxN = 1 << 24;
}

struct csdr_scope_batch {
    int device = 0, channels = 0;
    int w = 100, h = 100;                // m_Rect, :94
    std::vector<Chan> ch;
    std::mutex mu;                       // setters, put and the readers exclude each other
    ChanParam *h_par[kRing] = {};        // pinned
    ChanParam *d_par[kRing] = {};
    hipEvent_t ev[kRing] = {};
    bool busy[kRing] = {};
    int next = 0, last = -1;             // last: the slot whose event marks the end of the latest launch
    ChanState *d_state = nullptr;
    int *d_ring = nullptr, *d_screen = nullptr;
    hipStream_t rd = nullptr;            // the readers' stream
    // the FFT view
    sc::FftState *d_fst = nullptr;
    float *d_carry = nullptr, *d_bels = nullptr, *d_tab = nullptr;     // d_tab: window [2048], W_2048^i [1024], W_1024^(i k) [32][32]
    int *d_fscreen = nullptr, *d_peak = nullptr;
    double kc = 0.0, kb = 0.0;
};

static int scb_alloc(csdr_scope_batch *s)
{
    const size_t bytes = sizeof(ChanParam) * (size_t)s->channels;
    for (int i = 0; i < kRing; i++) {
        if (hipHostMalloc((void **)&s->h_par[i], bytes, hipHostMallocDefault) != hipSuccess)
            return fail(CSDR_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        CSDR_HIP(hipMalloc((void **)&s->d_par[i], bytes));
        CSDR_HIP(hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming));
    }
    const size_t words = (size_t)s->channels * 2 * sc::kMaxW;
    CSDR_HIP(hipMalloc((void **)&s->d_state, sizeof(ChanState) * (size_t)s->channels));
    CSDR_HIP(hipMalloc((void **)&s->d_ring, words * sizeof(int)));
    CSDR_HIP(hipMalloc((void **)&s->d_screen, words * sizeof(int)));
    CSDR_HIP(hipStreamCreateWithFlags(&s->rd, hipStreamNonBlocking));
    std::vector<ChanState> st((size_t)s->channels);
    for (auto &x : st) { memset(&x, 0, sizeof(x)); x.skipcounter = -2; }        // as after Reset(); m_TrigState WAIT, :117
    CSDR_HIP(hipMemcpy(s->d_state, st.data(), sizeof(ChanState) * st.size(), hipMemcpyHostToDevice));
    CSDR_HIP(hipMemset(s->d_ring, 0, words * sizeof(int)));
    CSDR_HIP(hipMemset(s->d_screen, 0, words * sizeof(int)));
    // the FFT view: two carries, the bels, screen and peak per receiver; CFft's tables at 2048 points (SetFFTParams(2048,
    // FALSE, 0.0, fs), :535; dsp/fft.cpp:186-198, K_B and K_C :171-176 with a dB compensation of 0)
    const size_t C = (size_t)s->channels, N = sc::kFftN;
    CSDR_HIP(hipMalloc((void **)&s->d_fst, sizeof(sc::FftState) * C));
    CSDR_HIP(hipMalloc((void **)&s->d_carry, C * 2 * N * 2 * sizeof(float)));
    CSDR_HIP(hipMalloc((void **)&s->d_bels, C * N * sizeof(float)));
    CSDR_HIP(hipMalloc((void **)&s->d_fscreen, C * sc::kMaxW * sizeof(int)));
    CSDR_HIP(hipMalloc((void **)&s->d_peak, C * sc::kMaxW * sizeof(int)));
    CSDR_HIP(hipMalloc((void **)&s->d_tab, (N + 2048 + 2048) * sizeof(float)));
    CSDR_HIP(hipMemset(s->d_fst, 0, sizeof(sc::FftState) * C));
    CSDR_HIP(hipMemset(s->d_carry, 0, C * 2 * N * 2 * sizeof(float)));
    CSDR_HIP(hipMemset(s->d_bels, 0, C * N * sizeof(float)));
    CSDR_HIP(hipMemset(s->d_fscreen, 0, C * sc::kMaxW * sizeof(int)));
    std::vector<int> pk(C * sc::kMaxW, s->h);                                    // m_FftPkBuf as Reset leaves it, :557
    CSDR_HIP(hipMemcpy(s->d_peak, pk.data(), pk.size() * sizeof(int), hipMemcpyHostToDevice));
    const double two_pi = 8.0 * std::atan(1.0);
    std::vector<float> tab(N + 4096);
    for (size_t i = 0; i < N; i++) tab[i] = (float)(2.0 * (.5 - .5 * std::cos((two_pi * (double)i) / (double)(N - 1))));
    for (size_t i = 0; i < 1024; i++) {
        const double a = two_pi * (double)i / (double)N;
        tab[N + 2 * i] = (float)std::cos(a); tab[N + 2 * i + 1] = (float)std::sin(a);
    }
    for (size_t k = 0; k < 32; k++)
        for (size_t i = 0; i < 32; i++) {
            const double a = two_pi * (double)(i * k) / 1024.0;
            tab[N + 2048 + 2 * (k * 32 + i)] = (float)std::cos(a); tab[N + 2048 + 2 * (k * 32 + i) + 1] = (float)std::sin(a);
        }
    CSDR_HIP(hipMemcpy(s->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    s->kb = 0.0 - 20 * std::log10((double)N * refc::FFT_K_AMPMAX / 2.0);
    s->kc = std::pow(10.0, (refc::FFT_K_MINDB - s->kb) / 10.0);
    s->kb = s->kb / 10.0;
    return CSDR_OK;
}

template <class F> static int scb_each_locked(csdr_scope_batch *s, int channel, F f);
template <class F> static int scb_each(csdr_scope_batch *s, int channel, F f)
{
    if (!s || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    return scb_each_locked(s, channel, f);
}
template <class F> static int scb_each_locked(csdr_scope_batch *s, int channel, F f)
{
    for (int c = channel < 0 ? 0 : channel; c < (channel < 0 ? s->channels : channel + 1); c++) f(s->ch[c]);
    return CSDR_OK;
}

// a free slot of the pinned ring: waits, on that launch's event only, when the launch kRing before has not finished
static int scb_slot(csdr_scope_batch *s, int *slot)
{
    *slot = s->next;
    if (s->busy[*slot]) { CSDR_HIP(hipEventSynchronize(s->ev[*slot])); s->busy[*slot] = false; }
    return CSDR_OK;
}
static int scb_sent(csdr_scope_batch *s, int slot, hipStream_t st)
{
    CSDR_HIP(hipEventRecord(s->ev[slot], st));
    s->busy[slot] = true;
    s->last = slot;
    s->next = (slot + 1) % kRing;
    return CSDR_OK;
}

// kind: SCOPE_REAL .. SCOPE_STEREO16 (scope_kernels.h); d_rows points at rows of that kind
static int scb_put(csdr_scope_batch *s, const void *d_rows, long long stride, const int *n, const double *sample_rate,
                   void *stream, int kind)
{
    const int cpx = scope_kind_cpx(kind);
    const unsigned align = kind == SCOPE_CPX ? 7u : kind == SCOPE_MONO16 ? 1u : 3u;
    if (!have_device()) return CSDR_EHIP;
    if (!s || !n || !sample_rate || stride < 0) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    bool any = false;
    for (int c = 0; c < s->channels; c++) {
        if (n[c] < 0 || n[c] > kMaxN || n[c] > stride) return fail(CSDR_EINVAL, "n[%d] = %d: 0..2^24 and <= stride", c, n[c]);
        if (n[c] == 0) continue;
        const double fs = sample_rate[c];
        if (!(fs > 0.0) || !std::isfinite(fs)) return fail(CSDR_EINVAL, "sample_rate[%d] must be positive", c);
        if (s->ch[c].view == sc::VIEW_FFT) {
            if (!(fs < sc::kFftMaxRate)) return fail(CSDR_EINVAL, "receiver %d: the FFT view needs a sample rate below 2^31 - 16", c);
        } else if (!((double)s->ch[c].span * fs / 1000.0 <= sc::kMaxSweep))
            return fail(CSDR_EINVAL, "receiver %d: a sweep of more than 2^30 samples", c);
        any = true;
    }
    if (any && (!d_rows || ((uintptr_t)d_rows & align) != 0)) return fail(CSDR_EINVAL, "rows missing or misaligned");
    bool work = any;
    for (int c = 0; c < s->channels; c++) work |= s->ch[c].flags != 0;
    if (!work) return CSDR_OK;
    CSDR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;
    if (int rc = scb_slot(s, &slot)) return rc;
    ChanParam *hp = s->h_par[slot];
    int max_count = 0;
    for (int c = 0; c < s->channels; c++) {
        s->ch[c].prepare(n[c], sample_rate[c], s->w, hp[c], s->h, cpx);
        if (hp[c].count > max_count) max_count = hp[c].count;
    }
    if (s->last >= 0) CSDR_HIP(hipStreamWaitEvent(st, s->ev[s->last], 0));     // the state follows the previous put, whatever its stream
    CSDR_HIP(hipMemcpyAsync(s->d_par[slot], hp, sizeof(ChanParam) * (size_t)s->channels, hipMemcpyHostToDevice, st));
    ScopeArgs a;
    a.rows = (const float *)d_rows; a.stride = stride; a.par = s->d_par[slot]; a.state = s->d_state; a.ring = s->d_ring;
    a.screen = s->d_screen; a.w = s->w; a.channels = s->channels;
    a.fst = s->d_fst; a.carry = s->d_carry; a.bels = s->d_bels; a.fscreen = s->d_fscreen; a.peak = s->d_peak;
    a.win = s->d_tab; a.tw1 = s->d_tab + sc::kFftN; a.tw2 = s->d_tab + sc::kFftN + 2048;
    a.kc = (float)s->kc; a.kb = s->kb; a.max_count = max_count;
    CSDR_HIP(scope_put_launch(a, kind, st));
    return scb_sent(s, slot, st);
}

// device -> host behind the last put only
static int scb_read(csdr_scope_batch *s, void *dst, const void *src, size_t bytes)
{
    CSDR_HIP(hipSetDevice(s->device));
    if (s->last >= 0) CSDR_HIP(hipStreamWaitEvent(s->rd, s->ev[s->last], 0));
    CSDR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->rd));
    CSDR_HIP(hipStreamSynchronize(s->rd));
    return CSDR_OK;
}

extern "C" {

csdr_scope_batch *csdr_scope_batch_create(int device, int channels)
{
    if (channels < 1 || channels > 4096) { fail(CSDR_EINVAL, "channels 1..4096"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_scope_batch *s = new csdr_scope_batch();
    s->device = device; s->channels = channels;
    s->ch.resize((size_t)channels);
    for (auto &k : s->ch) k.derive(s->w);
    if (scb_alloc(s) != CSDR_OK) {
        const std::string e = last_error_ref();
        csdr_scope_batch_destroy(s);
        fail(CSDR_EHIP, "%s", e.c_str());
        return nullptr;
    }
    return s;
}
void csdr_scope_batch_destroy(csdr_scope_batch *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (int i = 0; i < kRing; i++) {
        if (s->busy[i]) (void)hipEventSynchronize(s->ev[i]);          // its launch still reads the slot
        if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
        if (s->h_par[i]) (void)hipHostFree(s->h_par[i]);
        if (s->d_par[i]) (void)hipFree(s->d_par[i]);
    }
    if (s->rd) { (void)hipStreamSynchronize(s->rd); (void)hipStreamDestroy(s->rd); }
    if (s->d_state) (void)hipFree(s->d_state);
    if (s->d_ring) (void)hipFree(s->d_ring);
    if (s->d_screen) (void)hipFree(s->d_screen);
    void *fft[] = {s->d_fst, s->d_carry, s->d_bels, s->d_tab, s->d_fscreen, s->d_peak};
    for (void *p : fft)
        if (p) (void)hipFree(p);
    delete s;
}
int csdr_scope_batch_set_screen(csdr_scope_batch *s, int w, int h)
{
    if (!s || w < 1 || w > sc::kMaxW || h < 2) return fail(CSDR_EINVAL, "screen: 1 <= w <= 2048, h >= 2");
    std::lock_guard<std::mutex> lock(s->mu);
    s->w = w; s->h = h;
    for (auto &k : s->ch) k.reset(w);
    return CSDR_OK;
}
int csdr_scope_batch_set_horz_span(csdr_scope_batch *s, int channel, int ms)
{
    if (ms < 1) return fail(CSDR_EINVAL, "span >= 1 ms");
    return scb_each(s, channel, [=](Chan &k) { k.on_horz_span(ms, s->w); });
}
int csdr_scope_batch_set_display_rate(csdr_scope_batch *s, int channel, int rate)
{
    if (rate < 1) return fail(CSDR_EINVAL, "display rate >= 1");
    return scb_each(s, channel, [=](Chan &k) { k.on_display_rate(rate); });
}
int csdr_scope_batch_set_trigger_mode(csdr_scope_batch *s, int channel, int mode)
{
    if (mode < sc::TRIG_OFF || mode > sc::TRIG_NSINGLE) return fail(CSDR_EINVAL, "trigger mode 0..4");
    return scb_each(s, channel, [=](Chan &k) { k.on_trigger_mode(mode, s->w); });
}
int csdr_scope_batch_set_trig_level(csdr_scope_batch *s, int channel, int level)
{ return scb_each(s, channel, [=](Chan &k) { k.level = level; }); }
int csdr_scope_batch_set_vert_range(csdr_scope_batch *s, int channel, int range)
{ return scb_each(s, channel, [=](Chan &k) { k.vert = range; }); }
int csdr_scope_batch_reset(csdr_scope_batch *s, int channel)
{ return scb_each(s, channel, [=](Chan &k) { k.reset(s->w); }); }
int csdr_scope_batch_time_plot_done(csdr_scope_batch *s, int channel)
{ return scb_each(s, channel, [](Chan &k) { k.time_plot_done(); }); }
int csdr_scope_batch_set_time_display(csdr_scope_batch *s, int channel, int timemode)
{
    if (!s || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    for (int c = channel < 0 ? 0 : channel; c < (channel < 0 ? s->channels : channel + 1); c++) {   // before any state changes
        const Chan &k = s->ch[c];
        if (!timemode && !(k.sr < sc::kFftMaxRate)) return fail(CSDR_EINVAL, "receiver %d: the FFT view needs a sample rate below 2^31 - 16", c);
        if (timemode && !((double)k.span * k.sr / 1000.0 <= sc::kMaxSweep)) return fail(CSDR_EINVAL, "receiver %d: a sweep of more than 2^30 samples", c);
    }
    return scb_each_locked(s, channel, [=](Chan &k) { k.on_time_display(timemode, s->w); });
}
int csdr_scope_batch_enable_peak(csdr_scope_batch *s, int channel, int on)
{ return scb_each(s, channel, [=](Chan &k) { k.on_enable_peak(on != 0); }); }

int csdr_scope_batch_put_real(csdr_scope_batch *s, const float *d_rows, long long stride, const int *n,
                              const double *sample_rate, void *stream)
{ return scb_put(s, d_rows, stride, n, sample_rate, stream, SCOPE_REAL); }
int csdr_scope_batch_put_cpx(csdr_scope_batch *s, const float *d_rows, long long stride, const int *n,
                             const double *sample_rate, void *stream)
{ return scb_put(s, d_rows, stride, n, sample_rate, stream, SCOPE_CPX); }
int csdr_scope_batch_put_mono16(csdr_scope_batch *s, const short *d_rows, long long stride, const int *n,
                                const double *sample_rate, void *stream)
{ return scb_put(s, d_rows, stride, n, sample_rate, stream, SCOPE_MONO16); }
int csdr_scope_batch_put_stereo16(csdr_scope_batch *s, const short *d_rows, long long stride, const int *n,
                                  const double *sample_rate, void *stream)
{ return scb_put(s, d_rows, stride, n, sample_rate, stream, SCOPE_STEREO16); }

int csdr_scope_batch_get_emits(csdr_scope_batch *s, int *h_emits)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || !h_emits) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    std::vector<ChanState> st((size_t)s->channels);
    if (int rc = scb_read(s, st.data(), s->d_state, sizeof(ChanState) * st.size())) return rc;
    for (int c = 0; c < s->channels; c++) {
        h_emits[c] = (int)(st[c].emits - s->ch[c].seen);
        s->ch[c].seen = st[c].emits;
    }
    return CSDR_OK;
}
int csdr_scope_batch_get_state(csdr_scope_batch *s, int channel, long long *state8)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel < 0 || channel >= s->channels || !state8) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    ChanState st;
    if (int rc = scb_read(s, &st, s->d_state + channel, sizeof(st))) return rc;
    state8[0] = st.inpos; state8[1] = st.pos; state8[2] = st.prev; state8[3] = st.trigstate; state8[4] = st.trigcounter;
    state8[5] = st.trigbufpos; state8[6] = st.skipcounter; state8[7] = st.emits;
    return CSDR_OK;
}
int csdr_scope_batch_get_screen(csdr_scope_batch *s, int channel, int *re, int *im)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel < 0 || channel >= s->channels || !re || !im) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    const int *src = s->d_screen + (size_t)channel * 2 * sc::kMaxW;
    if (int rc = scb_read(s, re, src, sizeof(int) * (size_t)s->w)) return rc;
    return scb_read(s, im, src + sc::kMaxW, sizeof(int) * (size_t)s->w);
}
int csdr_scope_batch_get_fft_screen(csdr_scope_batch *s, int channel, int *screen, int *peak)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel < 0 || channel >= s->channels || !screen || !peak) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    sc::FftState f;
    if (int rc = scb_read(s, screen, s->d_fscreen + (size_t)channel * sc::kMaxW, sizeof(int) * (size_t)s->w)) return rc;
    if (int rc = scb_read(s, peak, s->d_peak + (size_t)channel * sc::kMaxW, sizeof(int) * (size_t)s->w)) return rc;
    if (int rc = scb_read(s, &f, s->d_fst + channel, sizeof(f))) return rc;
    return f.cpx ? 1 : 0;
}
int csdr_scope_batch_get_fft_ave(csdr_scope_batch *s, int channel, float *out2048)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel < 0 || channel >= s->channels || !out2048) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    return scb_read(s, out2048, s->d_bels + (size_t)channel * sc::kFftN, sizeof(float) * sc::kFftN);
}
int csdr_scope_batch_get_fft_state(csdr_scope_batch *s, int channel, long long *state4)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel < 0 || channel >= s->channels || !state4) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    sc::FftState f;
    ChanState st;
    if (int rc = scb_read(s, &f, s->d_fst + channel, sizeof(f))) return rc;
    if (int rc = scb_read(s, &st, s->d_state + channel, sizeof(st))) return rc;
    state4[0] = f.pos; state4[1] = st.skipcounter; state4[2] = s->ch[channel].skip; state4[3] = f.total;
    return CSDR_OK;
}
int csdr_scope_batch_get_fft_screens_all(csdr_scope_batch *s, int *d_out, long long out_stride, void *stream)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || !d_out) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    if (out_stride < s->w) return fail(CSDR_EINVAL, "out_stride must be >= w = %d", s->w);
    CSDR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (s->last >= 0) CSDR_HIP(hipStreamWaitEvent(st, s->ev[s->last], 0));
    int slot;                                            // the views travel as a put's settings do
    if (int rc = scb_slot(s, &slot)) return rc;
    for (int c = 0; c < s->channels; c++) { memset(&s->h_par[slot][c], 0, sizeof(ChanParam)); s->h_par[slot][c].view = s->ch[c].view; }
    CSDR_HIP(hipMemcpyAsync(s->d_par[slot], s->h_par[slot], sizeof(ChanParam) * (size_t)s->channels, hipMemcpyHostToDevice, st));
    ScopeFftScreenArgs a;
    a.fscreen = s->d_fscreen; a.peak = s->d_peak; a.par = s->d_par[slot]; a.out = d_out; a.out_stride = out_stride;
    a.w = s->w; a.channels = s->channels;
    CSDR_HIP(scope_fft_screens_launch(a, st));
    return scb_sent(s, slot, st);
}
int csdr_scope_batch_get_screens_all(csdr_scope_batch *s, int *d_out, long long out_stride, int *d_y, long long vert_stride,
                                     void *stream)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || !d_out) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    if (out_stride < s->w || (d_y && vert_stride < s->w)) return fail(CSDR_EINVAL, "strides must be >= w = %d", s->w);
    CSDR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (s->last >= 0) CSDR_HIP(hipStreamWaitEvent(st, s->ev[s->last], 0));
    ScopeScreenArgs a;
    a.screen = s->d_screen; a.par = nullptr; a.out = d_out; a.out_stride = out_stride; a.y = d_y; a.y_stride = vert_stride;
    a.w = s->w; a.h = s->h; a.channels = s->channels;
    int slot;                                            // the vertical ranges travel as a put's settings do
    if (int rc = scb_slot(s, &slot)) return rc;
    for (int c = 0; c < s->channels; c++) { memset(&s->h_par[slot][c], 0, sizeof(ChanParam)); s->h_par[slot][c].vert = s->ch[c].vert; }
    CSDR_HIP(hipMemcpyAsync(s->d_par[slot], s->h_par[slot], sizeof(ChanParam) * (size_t)s->channels, hipMemcpyHostToDevice, st));
    a.par = s->d_par[slot];
    CSDR_HIP(scope_screens_launch(a, st));
    return scb_sent(s, slot, st);
}

}  // extern "C"
