// chain_core.hpp -- the receive chain of the rows of one decimator plan, CDemodulator (dsp/demodulator.h:56-100):
// CDownConvert -> CFastFIR -> CSMeter -> CAgc -> AM/SAM/FM/SSB demodulator, device resident between the stages.  Shared
// by the single-channel host object (capi_demod.hip) and the batched form (capi_demod_batch.hip).
#pragma once
#include "capi_common.hpp"
#include "capi_internal.hpp"
#include "pc_unit.hpp"
#include "dc_host.hpp"
#include "stream_pool.hpp"
#include <cstdlib>
#include <vector>

#pragma GCC visibility push(hidden)                     // the library's own: nothing here is part of the ABI
namespace {
// move the not-yet-filtered tail of every row to the front of the staging buffer (dst == src)
__global__ void shift_rows_kernel(float *dst, const float *src, long stride, int src_off, int count)
{
    float2 *drow = reinterpret_cast<float2 *>(dst) + (long)blockIdx.x * stride;
    const float2 *srow = reinterpret_cast<const float2 *>(src) + (long)blockIdx.x * stride;
    // src_off >= count whenever at least one hop was consumed, so the ranges do not overlap
    for (int i = threadIdx.x; i < count; i += blockDim.x) drow[i] = srow[src_off + i];
}
}  // namespace

namespace csdr {

// one call's input: fp32 rows (d_in) or datagrams the down-converter decodes in its own loads (pk), optionally with the
// noise blanker's mask to apply; d_in_rows = the input row each row of the core reads (nullptr: its own)
struct ChainIn {
    const float *d_in; long in_stride; const int *d_in_rows; int n;
    const void *pk; int pk_len;
    const DcBlank *blank;
};
// ... and its output: d_out_rows = the output row of each row of the core (nullptr: its own, -1: muted)
struct ChainOut { float *d_out; long out_stride; const int *d_out_rows; bool stereo; };

// `rows` channels that share one decimator plan: staging, pending counts, the three stage objects
struct ChainCore {
    int device = 0, rows = 0, fft_n = 2048, L = 1024;
    csdr_downconvert_batch *dc = nullptr;
    csdr_fastfir_batch *ff = nullptr;
    PcUnit pc;
    // ---- the plain pass (strict mode, and the chained pipeline on top of it)
    float *d_stage = nullptr, *d_filt = nullptr, *d_agc = nullptr;
    long cap = 0;                       // capacity of every staging row (complex samples)
    int pending = 0;                    // decimated samples waiting for a full hop (same in every row)
    int last_out = 0;
    // stage taps (csdr_demod_set_taps / csdr_demod_batch_set_taps): bit k-1 = PROFILE_k.  Tap 1 -- this call's down-converter
    // output -- is copied to d_tap1 before the staging shift; tap 2 is d_filt; with tap 3 on the post-chain runs as
    // S-meter + AGC into d_agc, then the demodulator from there (the words are those of the fused walk)
    int taps = 0;
    float *d_tap1 = nullptr; long tap1_cap = 0; int tap1_n = 0;

    // ---- Chained pipeline (csdr_demod_batch_set_pipelined, round 6): filter + shift stay in the down-converter's stream,
    // the post-chain goes to a second one; the filter's output alternates between d_filt and d_agc
    struct Chained {
        Event ev_filt;                  // this call's filter output written
        Event ev_post_done[2];          // post-chain has finished with filter output buffer i
        bool post_busy[2] = {false, false};
        int filt_cur = 0;
        int init()
        {
            CSDR_HIP(ev_filt.create());
            for (auto &e : ev_post_done) CSDR_HIP(e.create());
            return CSDR_OK;
        }
    } ch;

    ~ChainCore()
    {
        if (dc) csdr_downconvert_batch_destroy(dc);
        if (ff) csdr_fastfir_batch_destroy(ff);
        for (float *p : {d_stage, d_filt, d_agc, d_tap1}) if (p) (void)hipFree(p);
    }
    int init(int dev, int nrows, int n)
    {
        device = dev; rows = nrows; fft_n = n; L = n / 2;
        dc = csdr_downconvert_batch_create(dev, nrows);
        ff = csdr_fastfir_batch_create(dev, nrows, n);
        if (!dc || !ff) return CSDR_EHIP;
        return pc.init(dev, nrows);
    }
    int ensure(long need)
    {
        if (need <= cap) return CSDR_OK;
        need = (need + L + 1023) / 1024 * 1024;
        // growing the staging (rare): the pending samples may still be in flight on a non-blocking stream
        CSDR_HIP(hipDeviceSynchronize());
        float *ns = nullptr, *nf = nullptr, *na = nullptr;
        CSDR_HIP(hipMalloc((void **)&ns, (size_t)rows * need * 8));
        CSDR_HIP(hipMalloc((void **)&nf, (size_t)rows * need * 8));
        CSDR_HIP(hipMalloc((void **)&na, (size_t)rows * need * 8));
        if (d_stage && pending > 0)
            CSDR_HIP(hipMemcpy2D(ns, (size_t)need * 8, d_stage, (size_t)cap * 8, (size_t)pending * 8, rows,
                                 hipMemcpyDeviceToDevice));
        for (float *p : {d_stage, d_filt, d_agc}) if (p) (void)hipFree(p);
        d_stage = ns; d_filt = nf; d_agc = na; cap = need;
        return CSDR_OK;
    }
    // One pass of the chain over in.n input samples per row (demodulator.cpp:172-207), strict mode: everything in stream s.
    // Returns the audio samples produced per row (0 or a multiple of the FastFIR hop).  dc_after: the down-converter waits
    // for it; dc_done: recorded behind the down-converter.
    int step(const ChainIn &in, const ChainOut &out, hipStream_t s, hipEvent_t dc_after = nullptr, hipEvent_t dc_done = nullptr)
    {
        const int m = step_dc(in, s, dc_after, dc_done);
        if (m < 0) return m;
        const int total = pending + m, nb = total / L;
        if (taps & 1) {                 // PROFILE_1: what the down-converter appended in this call, before the staging moves
            if (m > tap1_cap) {
                CSDR_HIP(hipStreamSynchronize(s));
                if (d_tap1) (void)hipFree(d_tap1);
                d_tap1 = nullptr; tap1_cap = 0;
                const long want = ((long)m + 1023) / 1024 * 1024;
                CSDR_HIP(hipMalloc((void **)&d_tap1, (size_t)rows * want * 8));
                tap1_cap = want;
            }
            if (m > 0)
                CSDR_HIP(hipMemcpy2DAsync(d_tap1, (size_t)tap1_cap * 8, d_stage + 2 * (size_t)pending, (size_t)cap * 8,
                                          (size_t)m * 8, rows, hipMemcpyDeviceToDevice, s));
            tap1_n = m;
        }
        last_out = 0;
        if (nb == 0) { pending = total; return 0; }
        int rc = csdr_fastfir_batch_process(ff, d_stage, cap, nb * L, d_filt, cap, s, 0);
        if (rc) return rc;
        if ((rc = post(d_filt, out, nb, s))) return rc;
        if ((rc = shift_tail(nb * L, total - nb * L, s))) return rc;
        pending = total - nb * L;
        last_out = nb * L;
        return last_out;
    }
    // The chained pipeline's pass: the down-converter, the filter and the staging shift in stream s -- so that the filter
    // reaches the chip in queue order behind its down-converter, BEFORE the next group's down-converter, which waits for an
    // event between two streams (HISTORY, round 6 (d): the other order starves the filter for a whole launch) -- and the
    // post-chain in stream sp, where it may run on into the next call: s is free for the next call's down-converter as soon
    // as the filter has left.  The filter's output alternates between d_filt and d_agc (idle without the stage taps): with one
    // buffer the next call's filter waited for this call's walk, and a first group's post-chain -- 1.5 ms when its peaks
    // kernel is starved beside the down-converters -- set the period.  *joined: the stream the call's last work is in.
    int step_split(const ChainIn &in, const ChainOut &out, hipStream_t s, hipStream_t sp, hipEvent_t dc_after,
                   hipEvent_t dc_done, hipStream_t *joined)
    {
        if (taps) return fail(CSDR_ESTATE, "stage taps need the strict mode");
        if (!ch.ev_filt) { const int rci = ch.init(); if (rci) return rci; }
        *joined = s;
        const int m = step_dc(in, s, dc_after, dc_done);
        if (m < 0) return m;
        const int total = pending + m, nb = total / L;
        last_out = 0;
        if (nb == 0) { pending = total; return 0; }
        const int fc = ch.filt_cur;
        ch.filt_cur ^= 1;
        float *fb = fc ? d_agc : d_filt;
        if (ch.post_busy[fc]) { CSDR_HIP(hipStreamWaitEvent(s, ch.ev_post_done[fc], 0)); ch.post_busy[fc] = false; }
        int rc = csdr_fastfir_batch_process(ff, d_stage, cap, nb * L, fb, cap, s, 0);
        if (rc) return rc;
        CSDR_HIP(hipEventRecord(ch.ev_filt, s));
        if ((rc = shift_tail(nb * L, total - nb * L, s))) return rc;
        pending = total - nb * L;
        CSDR_HIP(hipStreamWaitEvent(sp, ch.ev_filt, 0));
        if ((rc = post(fb, out, nb, sp))) return rc;
        CSDR_HIP(hipEventRecord(ch.ev_post_done[fc], sp));
        ch.post_busy[fc] = true;
        *joined = sp;
        last_out = nb * L;
        return last_out;
    }

private:
    // the move of the tail no hop has taken yet to the front of the staging rows
    int shift_tail(int from, int count, hipStream_t s)
    {
        if (count <= 0) return CSDR_OK;
        hipLaunchKernelGGL(shift_rows_kernel, dim3(rows), dim3(256), 0, s, d_stage, d_stage, cap, from, count);
        CSDR_HIP(hipGetLastError());
        return CSDR_OK;
    }
    // S-meter, AGC and demodulator of nb bursts: one fused launch
    int post(const float *filt, const ChainOut &out, int nb, hipStream_t s)
    {
        const int st = out.stereo ? PC_STEREO : 0;
        // parameters set since the last call: applied HERE, on the stream every launch below is ordered behind
        { const int rcp = pc.patches.flush(s); if (rcp) return rcp; }
        if (taps & 4) {                 // PROFILE_3: the AGC's output through device memory
            int rc = pc.run(PC_DO_SMETER | PC_DO_AGC, filt, cap, d_agc, cap, nb, L, s, nullptr);
            if (rc) return rc;
            return pc.run(PC_DO_DEMOD | st, d_agc, cap, out.d_out, out.out_stride, nb, L, s, out.d_out_rows);
        }
        return pc.run(PC_DO_SMETER | PC_DO_AGC | PC_DO_DEMOD | st, filt, cap, out.d_out, out.out_stride, nb, L, s, out.d_out_rows);
    }
    // both passes' first half: the down-converter of this call, appending to the pending samples of the staging rows, with
    // room made for what it appends; returns that count (< 0: error)
    int step_dc(const ChainIn &in, hipStream_t s, hipEvent_t dc_after, hipEvent_t dc_done)
    {
        const int m = csdr_downconvert_batch_out_count(dc, 0, in.n);
        if (m < 0) return m;
        { const int rce = ensure((long)pending + m); if (rce) return rce; }
        // the down-converters of the groups run one after the other (each fills the chip on its own);
        // what follows a group's down-converter overlaps with the next group's
        if (dc_after) CSDR_HIP(hipStreamWaitEvent(s, dc_after, 0));
        const int rc = csdr__downconvert_batch_process_rows(dc, in.d_in, in.in_stride, in.d_in_rows, in.n,
                                                            d_stage + 2 * (size_t)pending, cap, s, in.pk, in.pk_len, in.blank);
        if (rc) return rc;
        if (dc_done) CSDR_HIP(hipEventRecord(dc_done, s));
        return m;
    }
};

struct DemodInfo {                      // csdr_demod_info
    int HiCut, HiCutmin, HiCutmax, LowCut, LowCutmin, LowCutmax, FilterClickResolution, Offset, SquelchValue;
    int AgcSlope, AgcThresh, AgcManualGain, AgcDecay, AgcOn, AgcHangOn, Symetric;
};

// per-channel CDemodulator bookkeeping (host side)
struct ChanCfg {
    int mode = -1;
    int pending = -1;                   // batch form: mode requested before commit
    DemodInfo info{};
    double out_rate = 48000.0, want_bw = 48000.0, cw_off = 0.0;
    double demod_rate = 48000.0;        // m_SampleRate of the demodulator OBJECT: the output rate at the time the mode was
                                        // set (amdemod.cpp:50, fmdemod.cpp:62); an input-rate change does not touch it
};

// The filter set-ups of one csdr_demod_batch_set_demod_many call, gathered per filter object (= plan group) so that each
// object gets ONE csdr_fastfir_batch_setup_many -- its filters are then designed on the device, not on the caller's thread.
struct FilterDefer {
    struct Group { csdr_fastfir_batch *ff; std::vector<int> ch; std::vector<double> flo, fhi, off, fs; };
    std::vector<Group> groups;
    std::vector<int> status;
    void add(csdr_fastfir_batch *ff, int channel, double flo, double fhi, double off, double fs)
    {
        Group *g = nullptr;
        for (Group &q : groups) if (q.ff == ff) g = &q;
        if (!g) { groups.push_back(Group{ff, {}, {}, {}, {}, {}}); g = &groups.back(); }
        g->ch.push_back(channel); g->flo.push_back(flo); g->fhi.push_back(fhi); g->off.push_back(off); g->fs.push_back(fs);
    }
    int flush()          // (a rejected entry keeps its old taps, like the reference's "parameter error")
    {
        int err = CSDR_OK;
        for (Group &g : groups) {
            status.resize(g.ch.size());
            const int rc = csdr_fastfir_batch_setup_many(g.ff, (int)g.ch.size(), g.ch.data(), g.flo.data(), g.fhi.data(),
                                                         g.off.data(), g.fs.data(), status.data());
            if (rc < 0 && !err) err = rc;
        }
        groups.clear();
        return err;
    }
};

// CDemodulator::SetDemod (dsp/demodulator.cpp:107-157) for row r of core k; defer: the filter goes to the gather above
inline int apply_set_demod(ChainCore &k, int r, ChanCfg &c, double in_rate, int mode, const DemodInfo &info, FilterDefer *defer = nullptr)
{
    c.info = info;
    int rc;
    if (c.mode != mode) {
        // pull() first: it waits for the device, so that the down-converter's history reset below (on the null stream)
        // and the queued patches it flushes land behind every call still in flight (a pipelined batch's), not inside it
        if ((rc = k.pc.pull(r))) return rc;
        c.mode = mode;
        if (mode == PC_MODE_LSB || mode == PC_MODE_CWL) c.want_bw = -info.LowCutmin;
        else c.want_bw = info.HiCutmax;
        c.out_rate = csdr_downconvert_batch_set_data_rate(k.dc, r, in_rate, c.want_bw);
        if (c.out_rate < 0) return CSDR_EHIP;
        PcChannel &h = k.pc.h[r];
        h.mode = mode;
        c.demod_rate = c.out_rate;
        switch (mode) {                 // new demodulator object = fresh state
        case PC_MODE_AM:  am_init(h.am, k.pc.fir_am[r], c.demod_rate); break;
        case PC_MODE_SAM: sam_init(h.sam, k.pc.fir_sam[r], c.demod_rate); break;
        case PC_MODE_FM:  fm_init(h.fm, k.pc.fir_fm[r], c.demod_rate); break;
        default: break;
        }
        if ((rc = k.pc.push(r))) return rc;
    }
    c.cw_off = info.Offset;
    csdr_downconvert_batch_set_cw_offset(k.dc, r, c.cw_off);
    if (defer) defer->add(k.ff, k.rows == 1 ? -1 : r, info.LowCut, info.HiCut, c.cw_off, c.out_rate);
    else {
        rc = csdr_fastfir_batch_setup(k.ff, k.rows == 1 ? -1 : r, info.LowCut, info.HiCut, c.cw_off, c.out_rate);
        if (rc < 0 && rc != CSDR_EINVAL) return rc;      // EINVAL = reference's "parameter error": keep old taps
    }
    rc = k.pc.agc_set(r, info.AgcOn, info.AgcHangOn, info.AgcThresh, info.AgcManualGain, info.AgcSlope,
                      info.AgcDecay, c.out_rate);
    if (rc) return rc;
    if ((rc = k.pc.smeter_rate_set(r, c.out_rate))) return rc;
    // (parameter patches: nothing is read back from the device, nothing waits -- pc_unit.hpp)
    if (mode == PC_MODE_FM) rc = k.pc.fm_params_set(r, info.SquelchValue, c.demod_rate, (double)info.HiCut);   // fmdemod.cpp:95-98, :160-164 (the object's own rate)
    else if (mode == PC_MODE_AM) rc = k.pc.am_bandwidth_set(r, c.demod_rate, (info.HiCut - info.LowCut) / 2.0);   // amdemod.cpp:56-60
    return rc;
}

// CDemodulator::SetInputSampleRate (dsp/demodulator.cpp:92-99) for row r of core k.
// The down-converter is rebuilt for the new input rate (CDownConvert::SetDataRate, downconvert.cpp:114-173: new stage
// list from zeroed histories, the oscillator keeps phase and amplitude, the CW offset is added once more, :169),
// m_OutputRate follows -- and nothing else: filter taps and overlap, AGC constants and rings and the demodulator object
// stay as they are until the next SetDemod (which, for the same mode, keeps the demodulator built for the OLD output rate:
// ChanCfg::demod_rate).  The S-meter is handed m_OutputRate with every pass (demodulator.cpp:183), so its time constants
// follow at once.
inline int apply_input_rate(ChainCore &k, int r, ChanCfg &c, double rate)
{
    const double out = csdr_downconvert_batch_set_data_rate(k.dc, r, rate, c.want_bw);
    if (out < 0) return CSDR_EHIP;
    c.out_rate = out;
    return k.pc.smeter_rate_set(r, out);
}

}  // namespace csdr
#pragma GCC visibility pop
