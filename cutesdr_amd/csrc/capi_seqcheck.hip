// capi_seqcheck.hip -- C ABI of the datagram sequence check: one seq::State per receiver on the device (reference
// interface/netiobase.cpp:433, :484-496), advanced by K12 (seqcheck_kernels.hip) over the datagrams of a put.
// Ordering: every launch of the object -- a put or a get_all on the caller's stream, a clear or a reset on the
// object's own -- first makes its stream wait for the event of the launch before it and then records that event
// itself, so the launches take effect in the order of the calls whatever streams they run on, and the host waits
// for nothing except in get, which waits for that event alone.
#include "capi_common.hpp"
#include "seqcheck_kernels.h"
#include <cstdint>
#include <mutex>
#include <vector>

using namespace csdr;
using seq::State;

struct csdr_seqcheck_batch {
    int device = 0, channels = 0;
    State *d_state = nullptr;
    std::mutex mu;
    hipStream_t own = nullptr;           // clear, reset and get
    hipEvent_t ev = nullptr;             // the end of the object's latest launch
    bool issued = false;
};

// `st` behind the object's latest launch
static int sq_follow(csdr_seqcheck_batch *s, hipStream_t st)
{
    if (s->issued) CSDR_HIP(hipStreamWaitEvent(st, s->ev, 0));
    return CSDR_OK;
}
static int sq_sent(csdr_seqcheck_batch *s, hipStream_t st)
{
    CSDR_HIP(hipEventRecord(s->ev, st));
    s->issued = true;
    return CSDR_OK;
}
static int sq_alloc(csdr_seqcheck_batch *s)
{
    CSDR_HIP(hipMalloc((void **)&s->d_state, sizeof(State) * (size_t)s->channels));
    std::vector<State> init((size_t)s->channels, State{0, 0, 0, -1});
    CSDR_HIP(hipMemcpy(s->d_state, init.data(), sizeof(State) * init.size(), hipMemcpyHostToDevice));
    CSDR_HIP(hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking));
    CSDR_HIP(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    return CSDR_OK;
}
static int sq_control(csdr_seqcheck_batch *s, int channel, int reset)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    CSDR_HIP(hipSetDevice(s->device));
    if (int rc = sq_follow(s, s->own)) return rc;
    CSDR_HIP(seq::seqcheck_control_launch(s->d_state, channel < 0 ? 0 : channel, channel < 0 ? s->channels : channel + 1, reset, s->own));
    return sq_sent(s, s->own);
}

extern "C" {

csdr_seqcheck_batch *csdr_seqcheck_batch_create(int device, int channels)
{
    if (channels < 1) { fail(CSDR_EINVAL, "channels >= 1"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_seqcheck_batch *s = new csdr_seqcheck_batch();
    s->device = device; s->channels = channels;
    if (sq_alloc(s) != CSDR_OK) {
        const std::string e = last_error_ref();
        csdr_seqcheck_batch_destroy(s);
        fail(CSDR_EHIP, "%s", e.c_str());
        return nullptr;
    }
    return s;
}
void csdr_seqcheck_batch_destroy(csdr_seqcheck_batch *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->issued) (void)hipEventSynchronize(s->ev);     // its launch still uses the records
    if (s->ev) (void)hipEventDestroy(s->ev);
    if (s->own) { (void)hipStreamSynchronize(s->own); (void)hipStreamDestroy(s->own); }
    if (s->d_state) (void)hipFree(s->d_state);
    delete s;
}

int csdr_seqcheck_batch_put(csdr_seqcheck_batch *s, const void *d_packets, int npackets, int pkt_len, void *stream)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || !d_packets || npackets < 0) return fail(CSDR_EINVAL, "bad argument");
    if (pkt_len != 1028 && pkt_len != 1444)
        return fail(CSDR_EINVAL, "packet length %d: the wire format has 1028-byte (16 bit) and 1444-byte (24 bit) datagrams", pkt_len);
    if ((uintptr_t)d_packets & 3) return fail(CSDR_EINVAL, "datagram buffer must be 4-byte aligned");
    if ((long long)npackets * pkt_len >= (1ll << 31)) return fail(CSDR_EINVAL, "a channel's datagrams of one call must stay below 2 GiB");
    if (npackets == 0) return 0;
    std::lock_guard<std::mutex> lock(s->mu);
    CSDR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sq_follow(s, st)) return rc;
    CSDR_HIP(seq::seqcheck_put_launch((const unsigned char *)d_packets, s->channels, npackets, pkt_len, s->d_state, st));
    return sq_sent(s, st);
}

int csdr_seqcheck_batch_clear(csdr_seqcheck_batch *s, int channel) { return sq_control(s, channel, 0); }
int csdr_seqcheck_batch_reset(csdr_seqcheck_batch *s, int channel) { return sq_control(s, channel, 1); }

int csdr_seqcheck_batch_get(csdr_seqcheck_batch *s, int channel, long long *missed, long long *events, int *first_gap, int *last)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s || channel < 0 || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    CSDR_HIP(hipSetDevice(s->device));
    if (int rc = sq_follow(s, s->own)) return rc;
    State r;
    CSDR_HIP(hipMemcpyAsync(&r, s->d_state + channel, sizeof(r), hipMemcpyDeviceToHost, s->own));
    CSDR_HIP(hipStreamSynchronize(s->own));
    if (missed) *missed = r.missed;
    if (events) *events = r.events;
    if (first_gap) *first_gap = r.first_gap;
    if (last) *last = r.last;
    return CSDR_OK;
}

int csdr_seqcheck_batch_get_all(csdr_seqcheck_batch *s, long long *d_missed, long long *d_events, int *d_first_gap, void *stream)
{
    if (!have_device()) return CSDR_EHIP;
    if (!s) return fail(CSDR_EINVAL, "bad handle");
    if (((uintptr_t)d_missed & 7) || ((uintptr_t)d_events & 7) || ((uintptr_t)d_first_gap & 3))
        return fail(CSDR_EINVAL, "get_all: 64-bit arrays 8-byte aligned, first_gap 4-byte aligned");
    std::lock_guard<std::mutex> lock(s->mu);
    CSDR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sq_follow(s, st)) return rc;
    CSDR_HIP(seq::seqcheck_gather_launch(s->d_state, s->channels, d_missed, d_events, d_first_gap, st));
    return sq_sent(s, st);               // a later put must not overwrite the records being read
}

int csdr__seqcheck_waves(void) { return seq::seqcheck_waves(); }

}  // extern "C"
