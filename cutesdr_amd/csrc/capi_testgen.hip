// capi_testgen.hip -- C ABI of the batch signal generator: C independent CTestBench generators (reference
// gui/testbench.cpp:352-517; slots :225-244, :307-332; Reset :527-532, :575), one per receiver, writing the batch
// chain's fp32 input rows on the device.  All state lives on the host (testgen_host.hpp): a setter touches no device
// memory and waits for nothing.  generate() advances every receiver's state machine by n samples, writes the words of
// the launch into one slot of a small ring of pinned buffers, copies the slot to the device on the caller's stream
// and launches testgen_kernels.hip behind it.  A slot is reused only after the launch that read it has finished
// (one event per slot), so any number of calls may be queued; nothing waits on the whole device.
#include "capi_common.hpp"
#include "testgen_kernels.h"
#include <cmath>
#include <mutex>
#include <vector>

using namespace csdr;
using tg::ChanParam;
using tg::Gen;

namespace {
constexpr int kRing = 16;
constexpr long long kMaxN = 1ll << 30;
}

struct csdr_testgen_batch {
    int device = 0, channels = 0;
    std::vector<Gen> gen;
    unsigned long long seed = 0;
    std::mutex mu;                       // setters and generate exclude each other
    ChanParam *h_par[kRing] = {};        // pinned
    ChanParam *d_par[kRing] = {};
    hipEvent_t ev[kRing] = {};
    bool busy[kRing] = {};
    int next = 0;
};

static int tgb_alloc(csdr_testgen_batch *t)
{
    const size_t bytes = sizeof(ChanParam) * (size_t)t->channels;
    for (int i = 0; i < kRing; i++) {
        if (hipHostMalloc((void **)&t->h_par[i], bytes, hipHostMallocDefault) != hipSuccess)
            return fail(CSDR_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        CSDR_HIP(hipMalloc((void **)&t->d_par[i], bytes));
        CSDR_HIP(hipEventCreateWithFlags(&t->ev[i], hipEventDisableTiming));
    }
    return CSDR_OK;
}

template <class F> static int tgb_each(csdr_testgen_batch *t, int channel, double v, F f)
{
    if (!t || channel >= t->channels || !std::isfinite(v)) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(t->mu);
    for (int c = channel < 0 ? 0 : channel; c < (channel < 0 ? t->channels : channel + 1); c++) f(t->gen[c]);
    return CSDR_OK;
}

static int tgb_generate(csdr_testgen_batch *t, float *d_out, long long stride, int n, double fs, void *stream, int real)
{
    if (!have_device()) return CSDR_EHIP;
    if (!t || n < 0 || n > kMaxN || !(fs > 0.0) || !std::isfinite(fs)) return fail(CSDR_EINVAL, "bad argument");
    if (n == 0) return CSDR_OK;
    const int q = real ? 4 : 2;                          // samples per 16-byte store
    if (!d_out || stride < n || stride % q != 0 || ((uintptr_t)d_out & 15u) != 0)
        return fail(CSDR_EINVAL, "rows must be 16-byte aligned: stride %lld a multiple of %d and >= n", stride, q);
    std::lock_guard<std::mutex> lock(t->mu);
    CSDR_HIP(hipSetDevice(t->device));
    std::vector<unsigned> done((size_t)t->channels, 0u);
    bool first = true;
    for (;;) {
        const int slot = t->next;
        if (t->busy[slot]) { CSDR_HIP(hipEventSynchronize(t->ev[slot])); t->busy[slot] = false; }
        ChanParam *hp = t->h_par[slot];
        bool any = false;
        for (int c = 0; c < t->channels; c++) {
            Gen &g = t->gen[c];
            ChanParam &p = hp[c];
            p.nseg = 0;
            if (!g.on || done[c] == (unsigned)n) continue;            // testbench.cpp:359-360: the row is left alone
            if (first) {
                if (g.fs != fs) { g.fs = fs; g.pulse_valid = false; g.reset(); }      // :361-365, before the first sample
                g.pulse((unsigned)n, p);
                p.noise_on = g.noise_db > -160.0;
                p.noise_key = tg::noise_key(t->seed, c);
                p.count0 = g.count;
                p.amp = g.amp; p.noise_amp = g.noise_amp;
                g.count += (unsigned)n;
            } else {
                const ChanParam &o = t->h_par[(slot + kRing - 1) % kRing][c];          // the call's words, from its previous launch
                p.gate_on = o.gate_on; p.pos0 = o.pos0; p.wrap1 = o.wrap1; p.period = o.period; p.width = o.width;
                p.noise_on = o.noise_on; p.noise_key = o.noise_key; p.count0 = o.count0; p.amp = o.amp; p.noise_amp = o.noise_amp;
            }
            p.j_lo = done[c];
            done[c] += g.advance(done[c], (unsigned)n - done[c], p);
            p.j_hi = done[c];
            any = true;
        }
        if (!any) break;
        first = false;
        CSDR_HIP(hipMemcpyAsync(t->d_par[slot], hp, sizeof(ChanParam) * (size_t)t->channels, hipMemcpyHostToDevice,
                                (hipStream_t)stream));
        TestGenArgs a;
        a.out = d_out; a.stride = (long)stride; a.par = t->d_par[slot]; a.n = (unsigned)n; a.channels = t->channels;
        CSDR_HIP(testgen_launch(a, real, (hipStream_t)stream));
        CSDR_HIP(hipEventRecord(t->ev[slot], (hipStream_t)stream));
        t->busy[slot] = true;
        t->next = (slot + 1) % kRing;
        bool left = false;
        for (int c = 0; c < t->channels; c++) left |= t->gen[c].on && done[c] < (unsigned)n;
        if (!left) break;
    }
    return CSDR_OK;
}

extern "C" {

csdr_testgen_batch *csdr_testgen_batch_create(int device, int channels)
{
    if (channels < 1 || channels > 65535) { fail(CSDR_EINVAL, "channels 1..65535"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_testgen_batch *t = new csdr_testgen_batch();
    t->device = device; t->channels = channels;
    t->gen.resize((size_t)channels);
    for (auto &g : t->gen) g.reset();
    if (tgb_alloc(t) != CSDR_OK) {
        const std::string e = last_error_ref();
        csdr_testgen_batch_destroy(t);
        fail(CSDR_EHIP, "%s", e.c_str());
        return nullptr;
    }
    return t;
}
void csdr_testgen_batch_destroy(csdr_testgen_batch *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    for (int i = 0; i < kRing; i++) {
        if (t->busy[i]) (void)hipEventSynchronize(t->ev[i]);          // its launch still reads the slot
        if (t->ev[i]) (void)hipEventDestroy(t->ev[i]);
        if (t->h_par[i]) (void)hipHostFree(t->h_par[i]);
        if (t->d_par[i]) (void)hipFree(t->d_par[i]);
    }
    delete t;
}
int csdr_testgen_batch_set_on(csdr_testgen_batch *t, int channel, int on)
{ return tgb_each(t, channel, 0.0, [on](Gen &g) { g.on = on != 0; }); }
int csdr_testgen_batch_set_sweep_start(csdr_testgen_batch *t, int channel, double hz)
{ return tgb_each(t, channel, hz, [hz](Gen &g) { g.on_sweep_start(hz); }); }
int csdr_testgen_batch_set_sweep_stop(csdr_testgen_batch *t, int channel, double hz)
{ return tgb_each(t, channel, hz, [hz](Gen &g) { g.on_sweep_stop(hz); }); }
int csdr_testgen_batch_set_sweep_rate(csdr_testgen_batch *t, int channel, double hz_per_s)
{ return tgb_each(t, channel, hz_per_s, [hz_per_s](Gen &g) { g.on_sweep_rate(hz_per_s); }); }
int csdr_testgen_batch_set_pulse_width(csdr_testgen_batch *t, int channel, double seconds)
{ return tgb_each(t, channel, seconds, [seconds](Gen &g) { g.on_pulse_width(seconds); }); }
int csdr_testgen_batch_set_pulse_period(csdr_testgen_batch *t, int channel, double seconds)
{ return tgb_each(t, channel, seconds, [seconds](Gen &g) { g.on_pulse_period(seconds); }); }
int csdr_testgen_batch_set_signal_power(csdr_testgen_batch *t, int channel, double db)
{ return tgb_each(t, channel, db, [db](Gen &g) { g.on_signal_pwr(db); }); }
int csdr_testgen_batch_set_noise_power(csdr_testgen_batch *t, int channel, double db)
{ return tgb_each(t, channel, db, [db](Gen &g) { g.on_noise_pwr(db); }); }
int csdr_testgen_batch_reset(csdr_testgen_batch *t, int channel)
{ return tgb_each(t, channel, 0.0, [](Gen &g) { g.reset(); }); }
int csdr_testgen_batch_set_seed(csdr_testgen_batch *t, unsigned long long seed)
{
    if (!t) return fail(CSDR_EINVAL, "bad handle");
    std::lock_guard<std::mutex> lock(t->mu);
    t->seed = seed;
    for (auto &g : t->gen) g.count = 0;
    return CSDR_OK;
}
int csdr_testgen_batch_generate(csdr_testgen_batch *t, float *d_iq, long long stride, int n, double sample_rate, void *stream)
{ return tgb_generate(t, d_iq, stride, n, sample_rate, stream, 0); }
int csdr_testgen_batch_generate_real(csdr_testgen_batch *t, float *d_out, long long stride, int n, double sample_rate,
                                     void *stream)
{ return tgb_generate(t, d_out, stride, n, sample_rate, stream, 1); }

}  // extern "C"
