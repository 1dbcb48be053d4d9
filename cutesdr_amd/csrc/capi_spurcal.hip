// capi_spurcal.hip -- C ABI of the batch NCO-spur calibration: per receiver the offsets, count and active flag of
// CSdrInterface (reference interface/sdrinterface.cpp:791-848) on the device, commanded by spurcal_command and advanced
// by K13 (spurcal_kernels.hip) over the samples of a put.
// Ordering (capi_seqcheck.hip's): every launch of the object -- a put on the caller's stream, a command on the object's
// own -- first makes its stream wait for the event of the launch before it and then records that event itself, so
// commands and puts take effect in the order of the calls whatever streams they run on.  The host waits in read and
// get_state only, for that event alone.
#include "capi_common.hpp"
#include "capi_internal.hpp"
#include "downconv_kernels.h"
#include "spurcal_kernels.h"
#include <cstdint>
#include <mutex>
#include <vector>

using namespace csdr;
using spur::Rec;

struct csdr_spurcal_batch {
    int device = 0, channels = 0;
    double *d_dc = nullptr;              // [channels][2]: the d_dc of unpack and display calls
    Rec *d_rec = nullptr;
    double *d_part = nullptr;            // K13's tile partials, grown on demand
    size_t part_cap = 0;                 // doubles
    std::mutex mu;
    hipStream_t own = nullptr;           // commands and reads
    hipEvent_t ev = nullptr;             // the end of the object's latest launch
    bool issued = false;
};

static int sc_follow(csdr_spurcal_batch *s, hipStream_t st)
{
    if (s->issued) CSDR_HIP(hipStreamWaitEvent(st, s->ev, 0));
    return CSDR_OK;
}
static int sc_sent(csdr_spurcal_batch *s, hipStream_t st)
{
    CSDR_HIP(hipEventRecord(s->ev, st));
    s->issued = true;
    return CSDR_OK;
}
static int sc_alloc(csdr_spurcal_batch *s)
{
    CSDR_HIP(hipMalloc((void **)&s->d_dc, sizeof(double) * 2 * (size_t)s->channels));
    CSDR_HIP(hipMalloc((void **)&s->d_rec, sizeof(Rec) * (size_t)s->channels));
    CSDR_HIP(hipMemset(s->d_dc, 0, sizeof(double) * 2 * (size_t)s->channels));
    CSDR_HIP(hipMemset(s->d_rec, 0, sizeof(Rec) * (size_t)s->channels));
    CSDR_HIP(hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking));
    CSDR_HIP(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    return CSDR_OK;
}
// the command on channel (or on every receiver, channel < 0), on the object's stream; the lock is held
static int sc_command(csdr_spurcal_batch *s, int channel, int cmd, double vi, double vq)
{
    CSDR_HIP(hipSetDevice(s->device));
    if (int rc = sc_follow(s, s->own)) return rc;
    CSDR_HIP(spur::spurcal_command_launch(s->d_dc, s->d_rec, channel < 0 ? 0 : channel, channel < 0 ? s->channels : channel + 1,
                                          cmd, vi, vq, s->own));
    return sc_sent(s, s->own);
}
static int sc_control(csdr_spurcal_batch *s, int channel, int cmd, double vi, double vq)
{
    if (!s || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    return sc_command(s, channel, cmd, vi, vq);
}
// one put: src.n samples per receiver (0: only the ordering -- what was commanded is in front of `stream` afterwards)
static int sc_put(csdr_spurcal_batch *s, spur::Src src, void *stream)
{
    std::lock_guard<std::mutex> lock(s->mu);
    CSDR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (src.n > 0) {
        const size_t need = 2 * (size_t)s->channels * (size_t)spur::spurcal_tiles(src.n);
        if (need > s->part_cap) {
            if (s->issued) CSDR_HIP(hipEventSynchronize(s->ev));     // the put before may still read the old scratch
            if (s->d_part) { CSDR_HIP(hipFree(s->d_part)); s->d_part = nullptr; s->part_cap = 0; }
            if (hipMalloc((void **)&s->d_part, need * sizeof(double)) != hipSuccess)
                return fail(CSDR_ENOMEM, "hipMalloc(%zu) failed", need * sizeof(double));
            s->part_cap = need;
        }
    }
    if (int rc = sc_follow(s, st)) return rc;
    CSDR_HIP(spur::spurcal_put_launch(src, s->channels, s->d_dc, s->d_rec, s->d_part, st));
    return sc_sent(s, st);
}
static int sc_packet_args(const void *s, const void *d_packets, int npackets, int pkt_len)
{   // the datagram rules of csdr_fft_batch_put_display_packets
    if (!s || !d_packets || npackets < 0) return fail(CSDR_EINVAL, "bad argument");
    if (pkt_len != 1028 && pkt_len != 1444)
        return fail(CSDR_EINVAL, "packet length %d: the wire format has 1028-byte (16 bit) and 1444-byte (24 bit) datagrams", pkt_len);
    if ((long long)npackets * pkt_len >= (1ll << 31)) return fail(CSDR_EINVAL, "a channel's datagrams of one call must stay below 2 GiB");
    if ((uintptr_t)d_packets & 3) return fail(CSDR_EINVAL, "datagram buffer must be 4-byte aligned");
    return CSDR_OK;
}
static int sc_row_args(const void *s, const float *d_in, long long in_stride, int n, int call_len)
{
    if (!s || !d_in || n < 0 || in_stride < n || call_len < 1) return fail(CSDR_EINVAL, "bad argument");
    if ((uintptr_t)d_in & 7) return fail(CSDR_EINVAL, "d_in must be 8-byte aligned");
    return CSDR_OK;
}
static spur::Src sc_src(const float *d_in, long long in_stride, const void *d_packets, int npackets, int pkt_len, int n,
                        int call_len, const DcBlank *blank)
{
    const int per = pkt_len == 1444 ? 240 : 256;
    spur::Src a{};
    a.in = d_in; a.in_stride = (long)in_stride;
    if (d_packets) a.wire = WireIn{(const unsigned char *)d_packets, (long)npackets * pkt_len, pkt_len, per};
    a.n = d_packets ? npackets * per : n;
    a.call_len = d_packets ? per : call_len;
    if (blank) {
        a.nb_mask = blank->mask; a.nb_mask_stride = blank->mask_stride;
        a.nb_state = (const NbChan *)blank->state; a.nb_hist = blank->hist;
    }
    return a;
}

extern "C" {

csdr_spurcal_batch *csdr_spurcal_batch_create(int device, int channels)
{
    if (channels < 1) { fail(CSDR_EINVAL, "channels >= 1"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_spurcal_batch *s = new csdr_spurcal_batch();
    s->device = device; s->channels = channels;
    if (sc_alloc(s) != CSDR_OK) {
        const std::string e = last_error_ref();
        csdr_spurcal_batch_destroy(s);
        fail(CSDR_EHIP, "%s", e.c_str());
        return nullptr;
    }
    return s;
}
void csdr_spurcal_batch_destroy(csdr_spurcal_batch *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->issued) (void)hipEventSynchronize(s->ev);     // its launch still uses the records
    if (s->ev) (void)hipEventDestroy(s->ev);
    if (s->own) { (void)hipStreamSynchronize(s->own); (void)hipStreamDestroy(s->own); }
    if (s->d_part) (void)hipFree(s->d_part);
    if (s->d_rec) (void)hipFree(s->d_rec);
    if (s->d_dc) (void)hipFree(s->d_dc);
    delete s;
}

int csdr_spurcal_batch_set(csdr_spurcal_batch *s, int channel, double offset_i, double offset_q)
{
    return sc_control(s, channel, spur::CMD_SET, offset_i, offset_q);
}
int csdr_spurcal_batch_start_cal(csdr_spurcal_batch *s, int channel) { return sc_control(s, channel, spur::CMD_STARTCAL, 0.0, 0.0); }

static int sc_fetch(csdr_spurcal_batch *s, int channel, bool command, double *offset_i, double *offset_q, int *count, int *active)
{
    if (!s || channel < 0 || channel >= s->channels) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(s->mu);
    if (command) { if (int rc = sc_command(s, channel, spur::CMD_READ, 0.0, 0.0)) return rc; }
    else {
        CSDR_HIP(hipSetDevice(s->device));
        if (int rc = sc_follow(s, s->own)) return rc;
    }
    double off[2];
    Rec r;
    CSDR_HIP(hipMemcpyAsync(off, s->d_dc + 2 * channel, sizeof(off), hipMemcpyDeviceToHost, s->own));
    CSDR_HIP(hipMemcpyAsync(&r, s->d_rec + channel, sizeof(r), hipMemcpyDeviceToHost, s->own));
    CSDR_HIP(hipStreamSynchronize(s->own));
    if (offset_i) *offset_i = off[0];
    if (offset_q) *offset_q = off[1];
    if (count) *count = r.count;
    if (active) *active = r.active;
    return CSDR_OK;
}
int csdr_spurcal_batch_read(csdr_spurcal_batch *s, int channel, double *offset_i, double *offset_q)
{
    return sc_fetch(s, channel, true, offset_i, offset_q, nullptr, nullptr);
}
int csdr_spurcal_batch_get_state(csdr_spurcal_batch *s, int channel, double *offset_i, double *offset_q, int *count, int *active)
{
    return sc_fetch(s, channel, false, offset_i, offset_q, count, active);
}
const double *csdr_spurcal_batch_dc(csdr_spurcal_batch *s)
{
    if (!s) { fail(CSDR_EINVAL, "bad handle"); return nullptr; }
    return s->d_dc;
}

int csdr_spurcal_batch_put_packets(csdr_spurcal_batch *s, const void *d_packets, int npackets, int pkt_len, void *stream)
{
    if (int rc = sc_packet_args(s, d_packets, npackets, pkt_len)) return rc;
    return sc_put(s, sc_src(nullptr, 0, d_packets, npackets, pkt_len, 0, 0, nullptr), stream);
}
int csdr_spurcal_batch_put_stream(csdr_spurcal_batch *s, const float *d_in, long long in_stride, int n, int call_len, void *stream)
{
    if (int rc = sc_row_args(s, d_in, in_stride, n, call_len)) return rc;
    return sc_put(s, sc_src(d_in, in_stride, nullptr, 0, 0, n, call_len, nullptr), stream);
}
int csdr_spurcal_batch_put_packets_blanked(csdr_spurcal_batch *s, csdr_demod_batch *b, const void *d_packets, int npackets,
                                           int pkt_len, void *stream)
{
    if (!b) return fail(CSDR_EINVAL, "bad argument");
    if (int rc = sc_packet_args(s, d_packets, npackets, pkt_len)) return rc;
    const int per = pkt_len == 1444 ? 240 : 256;
    DcBlank blank;
    if (int rc = csdr__demod_batch_blank_for(b, "spur calibration", s->channels, s->device, BLANK_CALL_PACKETS, d_packets, pkt_len,
                                             npackets * per, &blank)) return rc;
    return sc_put(s, sc_src(nullptr, 0, d_packets, npackets, pkt_len, 0, 0, &blank), stream);
}
int csdr_spurcal_batch_put_stream_blanked(csdr_spurcal_batch *s, csdr_demod_batch *b, const float *d_in, long long in_stride,
                                          int n, int call_len, void *stream)
{
    if (!b) return fail(CSDR_EINVAL, "bad argument");
    if (int rc = sc_row_args(s, d_in, in_stride, n, call_len)) return rc;
    DcBlank blank;
    if (int rc = csdr__demod_batch_blank_for(b, "spur calibration", s->channels, s->device, BLANK_CALL_ROWS, d_in, in_stride, n,
                                             &blank)) return rc;
    return sc_put(s, sc_src(d_in, in_stride, nullptr, 0, 0, n, call_len, &blank), stream);
}

}  // extern "C"
