// capi_demod_batch.hip -- C ABI of the batched, device-resident form of the receive chain (CDemodulator for many
// receivers at once): plan groups of receivers that decimate alike, each a ChainCore (chain_core.hpp), and the two
// schedules a process call runs them in.  The single-channel host form: capi_demod.hip.
#include "chain_core.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

using namespace csdr;

namespace {
// Everything a plan group owns: the chain of its rows, which receiver sits in which row, and its place in the
// schedules -- the groups are independent: each runs on its own stream, forked from and joined to the caller's.
struct PlanGroup {
    ChainCore core;
    std::vector<int> members;                         // channel ids in row order, -1 = muted row (its receiver has moved
                                                      // to another plan group: csdr_demod_batch_set_demod)
    std::vector<int> row_in_last;                     // input row of each row as last uploaded
    int *d_rows = nullptr;                            // device array of the rows' input rows
    int *d_out_rows = nullptr;                        // ... and of their output rows (= channel ids), -1 = muted
    hipStream_t stream = nullptr;
    hipStream_t post_stream = nullptr;                // pipelined mode: its post-chain's stream
    Event join;                                       // the group's part of a call has been issued
    Event dc_done;                                    // its down-converter has been issued and finished
    bool prev_join = false;                           // pipelined: `join` of the previous call not yet waited for
    ~PlanGroup()
    {
        if (d_rows) (void)hipFree(d_rows);
        if (d_out_rows) (void)hipFree(d_out_rows);
        if (stream) stream_pool().put(core.device, stream);
        if (post_stream) stream_pool().put(core.device, post_stream);
    }
    // the stream (at `prio`) and the two events, whatever is still missing
    int plumbing(int prio)
    {
        if (!stream) CSDR_HIP(stream_pool().get(core.device, prio, &stream));
        CSDR_HIP(join.create());
        CSDR_HIP(dc_done.create());
        return CSDR_OK;
    }
    int post_plumbing(int prio)
    {
        if (!post_stream) CSDR_HIP(stream_pool().get(core.device, prio, &post_stream, STREAM_POST));
        return CSDR_OK;
    }
    // pipelined mode: `caller` waits for what the previous call left in flight here -- its join event, recorded behind the
    // call's last work (the input has been consumed, the output rows are complete)
    int late_join(hipStream_t caller)
    {
        if (prev_join) { CSDR_HIP(hipStreamWaitEvent(caller, join, 0)); prev_join = false; }
        return CSDR_OK;
    }
};
}  // namespace

struct csdr_demod_batch {
    int device, channels, fft_n;
    double in_rate = 0.0;
    std::vector<ChanCfg> cfg;
    std::vector<int> core_of, row_of;                 // channel -> (group, row)
    std::vector<int> in_row;                          // channel -> row of the caller's input it reads (csdr_demod_batch_set_input_rows)
    std::vector<std::unique_ptr<PlanGroup>> groups;   // one per distinct decimator plan (addresses stay: set_input_rate)
    std::vector<int> order;                           // groups, heaviest post-chain first
    Event fork;
    bool pipelined = false;                           // csdr_demod_batch_set_pipelined
    bool have_last_dc = false;                        // pipelined mode: dc_done of order.back() holds the previous call's record
    int taps = 0;                                     // csdr_demod_batch_set_taps (new groups inherit it: batch_move_row)
    bool rate_change_failed = false;                  // csdr_demod_batch_set_input_rate stopped half way: no processing until one succeeds
    float *d_blank = nullptr;                         // blanked input of process_packets (two-pass form)
    long raw_cap = 0;
    unsigned *d_mask = nullptr; long mask_cap = 0;    // the blanker's mask of process_packets (fused form): [channels][mask_cap] words
    DcBlank blank{};
    // the last blanked call, for the display behind it (csdr__demod_batch_last_blank): `blank` still describes what its
    // mask pass left.  Dropped by every other process call, a commit and a rate change.
    BlankCall last_blank{BLANK_CALL_NONE, nullptr, 0, 0};
    bool last_two_pass = false;                       // ... and that call ran the two-pass form (CSDR_BLANK_FUSED=0): no mask
    ~csdr_demod_batch()
    {
        if (d_blank) (void)hipFree(d_blank);
        if (d_mask) (void)hipFree(d_mask);
    }
    ChainCore &core(int channel) { return groups[core_of[channel]]->core; }
};

// The group whose post-chain is the longest pole (FM: PLL + squelch filters, at the highest decimated rate) goes
// first: its down-converter should not share the chip with the other groups' while its demodulators wait.
static void batch_order(csdr_demod_batch *b)
{
    b->have_last_dc = false;                            // (the pipelined mode's link to the previous call's last group)
    std::vector<double> weight(b->groups.size(), 0.0);
    for (int c = 0; c < b->channels; c++) {
        if (b->core_of[c] < 0) continue;
        const int m = b->cfg[c].mode;
        const double w = (m == PC_MODE_FM ? 3.0 : m == PC_MODE_SAM ? 2.5 : m == PC_MODE_AM ? 1.5 : 1.0) * b->cfg[c].out_rate;
        weight[b->core_of[c]] = std::max(weight[b->core_of[c]], w);
    }
    b->order.resize(b->groups.size());
    for (size_t i = 0; i < b->order.size(); i++) b->order[i] = (int)i;
    std::stable_sort(b->order.begin(), b->order.end(), [&](int x, int y) { return weight[x] > weight[y]; });
}
// The fork event and every group's stream and events, whatever is still missing.  ranked: the heaviest group on the
// highest-priority stream (commit, set_pipelined); else -- a move is about to add `extra` -- the lowest priority, until
// batch_order and the next ranked pass.  Nothing of `extra` is published here.
static int batch_plumbing(csdr_demod_batch *b, bool ranked, PlanGroup *extra = nullptr)
{
    CSDR_HIP(b->fork.create());
    int pr_lo = 0, pr_hi = 0;                          // numerically lower = higher priority
    CSDR_HIP(hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi));
    for (size_t ki = 0; ki < b->groups.size(); ki++) {
        const size_t rank = std::find(b->order.begin(), b->order.end(), (int)ki) - b->order.begin();
        const int rc = b->groups[ki]->plumbing(ranked ? std::min(pr_hi + (int)rank, pr_lo) : pr_lo);
        if (rc) return rc;
    }
    return extra ? extra->plumbing(pr_lo) : CSDR_OK;
}
// the record of the last blanked call goes with whatever changes what `blank` describes, or runs the chain on other input
static void batch_forget_blank(csdr_demod_batch *b)
{
    b->last_blank = BlankCall{BLANK_CALL_NONE, nullptr, 0, 0};
    b->last_two_pass = false;
}
// pipelined mode: `stream` waits for what the previous call left in flight (PlanGroup::late_join), in every group.
// (The display behind a blanked call -- csdr_fft_batch_put_display_stream_blanked / _packets_blanked -- needs no join of
// its own, in either mode: it only READS, on the caller's stream, the mask, the blanker's state and history half and the
// input that the call's mask pass -- issued on that same stream before it -- wrote or read; the down-converters that
// read the same buffers on the batch's streams do not write them.  The NEXT blanked call's mask pass, which overwrites
// mask and history half, is issued on the caller's stream too, hence behind the display's reads -- and, by the join
// below, behind the down-converters'.  The caller refills the input only behind that next call, as the pipelined
// contract says.)
static int batch_late_join(csdr_demod_batch *b, void *stream)
{
    for (auto &g : b->groups) { const int rc = g->late_join((hipStream_t)stream); if (rc) return rc; }
    return CSDR_OK;
}

// a plan group none of whose rows has a receiver any more (all moved away) leaves the batch: no more launches for it
static void batch_drop_core(csdr_demod_batch *b, int ki)
{
    b->groups.erase(b->groups.begin() + ki);
    b->have_last_dc = false;
    for (int &c : b->core_of) if (c > ki) c--;
}

/* CDemodulator::SetDemod with a NEW MODE whose decimator chain has another number of stages -- hence another output
 * rate, hop count and staging fill -- on a committed batch (dsp/demodulator.cpp:107-157).  The receiver leaves its plan
 * group (whose rows share one decimation) with everything the reference keeps across SetDemod: the down-converter's
 * oscillator, the filter's overlap AND its partly filled input (samples at the OLD rate: fastfir.cpp:278-285 never
 * resets m_InBufInPos), AGC and S-meter objects; the new demodulator starts fresh and the rebuilt decimator from zero
 * histories, as there.  It continues in a muted row of a group that already has the new decimation and the same
 * staging fill (a receiver that left earlier: retuning back and forth does not grow the batch), else in a group of
 * its own.  Its old row stays behind muted (no output, no S-meter; the group still filters it) and a group left with
 * muted rows only is dropped.  Transactional: the new row is complete before anything of the batch changes, and any
 * failure leaves the batch as it was.  A receiver already alone in its group changes in place, exactly like the
 * single-channel object. */
template <class Apply>                                // apply(core, row, cfg): what makes the receiver's chain the new one
static int batch_move_row(csdr_demod_batch *b, int channel, int new_stages, Apply apply)
{
    CSDR_HIP(hipDeviceSynchronize());                  // control plane: nothing of this batch in flight from here on
    const int ka = b->core_of[channel], r = b->row_of[channel];
    PlanGroup &GA = *b->groups[ka];
    ChainCore &A = GA.core;
    if (A.rows == 1) return apply(A, 0, b->cfg[channel]);
    // ---- where to: a muted row of a group with the new decimation and the same staging fill, else a new group
    int kb = -1, rb = -1;
    for (size_t ki = 0; ki < b->groups.size() && kb < 0; ki++) {
        PlanGroup &G = *b->groups[ki];
        if ((int)ki == ka || G.core.pending != A.pending || G.core.rows < 2) continue;
        // (the muted row's own chain is its group's: a muted row follows its group through every rate change, while row 0
        // may be a receiver that is itself about to leave)
        for (size_t q = 0; q < G.members.size(); q++)
            if (G.members[q] < 0 && csdr_downconvert_batch_out_count(G.core.dc, (int)q, 1 << 12) == (1 << 12) >> new_stages) {
                kb = (int)ki; rb = (int)q; break;
            }
    }
    std::unique_ptr<PlanGroup> fresh;                  // the new group, complete on the side; dropped whole on failure
    int rc = CSDR_OK;
    auto hip = [&](hipError_t e) { if (e != hipSuccess && rc == CSDR_OK) rc = fail(CSDR_EHIP, "%s", hipGetErrorString(e)); return e == hipSuccess; };
    if (kb < 0) {
        fresh.reset(new PlanGroup());
        rc = fresh->core.init(b->device, 1, b->fft_n);
        fresh->core.taps = b->taps;                    // the batch's stage taps hold for its new groups too
        // (a pipelined batch's new group gets its post-chain stream in run_chained)
        if (rc == CSDR_OK) rc = fresh->core.ensure((long)A.pending + 1);
        if (rc == CSDR_OK) { hip(hipMalloc((void **)&fresh->d_rows, sizeof(int))) && hip(hipMalloc((void **)&fresh->d_out_rows, sizeof(int))); }
        if (rc == CSDR_OK) rc = batch_plumbing(b, false, fresh.get());
    }
    PlanGroup &GT = kb < 0 ? *fresh : *b->groups[kb];
    ChainCore &T = GT.core;
    const int tr = kb < 0 ? 0 : rb;
    ChanCfg cfg = b->cfg[channel];                     // committed only when everything has worked
    if (rc == CSDR_OK) rc = csdr__downconvert_batch_copy_channel(T.dc, tr, A.dc, r);
    if (rc == CSDR_OK) rc = csdr__fastfir_batch_copy_row(T.ff, tr, A.ff, r);
    if (rc == CSDR_OK) rc = T.pc.import_channel(tr, A.pc, r);
    if (rc == CSDR_OK && A.pending > 0)
        hip(hipMemcpy(T.d_stage + (size_t)tr * T.cap * 2, A.d_stage + (size_t)r * A.cap * 2, (size_t)A.pending * 8,
                      hipMemcpyDeviceToDevice));
    if (rc == CSDR_OK) rc = apply(T, tr, cfg);
    const int muted = -1;
    if (rc == CSDR_OK) hip(hipMemcpy(GT.d_rows + tr, &b->in_row[channel], sizeof(int), hipMemcpyHostToDevice));
    if (rc == CSDR_OK) hip(hipMemcpy(GT.d_out_rows + tr, &channel, sizeof(int), hipMemcpyHostToDevice));
    if (rc == CSDR_OK) hip(hipMemcpy(GA.d_out_rows + r, &muted, sizeof(int), hipMemcpyHostToDevice));
    if (rc != CSDR_OK) {                               // nothing published: the batch is as it was (`fresh` goes with all
        // it holds, its stream back to the pool; a reused muted row holds copied state nobody reads)
        if (kb >= 0) (void)hipMemcpy(GT.d_out_rows + rb, &muted, sizeof(int), hipMemcpyHostToDevice);
        return rc;
    }
    // ---- publish (host bookkeeping only from here on: cannot fail)
    b->cfg[channel] = cfg;
    GA.members[r] = -1;
    if (kb < 0) {
        fresh->core.pending = A.pending;
        fresh->members.assign(1, channel);
        fresh->row_in_last.assign(1, b->in_row[channel]);
        b->groups.push_back(std::move(fresh));
        b->core_of[channel] = (int)b->groups.size() - 1; b->row_of[channel] = 0;
    } else {
        GT.members[rb] = channel;
        if ((size_t)rb < GT.row_in_last.size()) GT.row_in_last[rb] = b->in_row[channel];
        b->core_of[channel] = kb; b->row_of[channel] = rb;
    }
    if (std::all_of(GA.members.begin(), GA.members.end(), [](int m) { return m < 0; })) batch_drop_core(b, ka);
    batch_order(b);
    return CSDR_OK;
}
static int batch_move_channel(csdr_demod_batch *b, int channel, int mode, const DemodInfo &di, int new_stages)
{
    const double in_rate = b->in_rate;
    return batch_move_row(b, channel, new_stages, [&](ChainCore &k, int row, ChanCfg &cfg) {
        return apply_set_demod(k, row, cfg, in_rate, mode, di);
    });
}

extern "C" {

csdr_demod_batch *csdr_demod_batch_create(int device, int channels, int fastfir_n)
{
    if (channels < 1) { fail(CSDR_EINVAL, "channels >= 1"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_demod_batch *b = new csdr_demod_batch();
    b->device = device; b->channels = channels; b->fft_n = fastfir_n;
    b->cfg.assign(channels, ChanCfg());
    b->core_of.assign(channels, -1); b->row_of.assign(channels, -1);
    b->in_row.resize(channels);
    for (int c = 0; c < channels; c++) b->in_row[c] = c;
    return b;
}
void csdr_demod_batch_destroy(csdr_demod_batch *b) { delete b; }
/* CDemodulator::SetInputSampleRate (dsp/demodulator.cpp:92-99) for every receiver of the batch, at any time -- the host
 * calls it on every bandwidth switch of the radio (interface/sdrinterface.cpp:753-754).  Before the commit it only
 * records the rate.  On a committed batch every receiver's down-converter is rebuilt for the new rate with what the
 * reference keeps (apply_input_rate); receivers stay in their rows as long as the rows of a plan group still share
 * one decimation (they do whenever they share one bandwidth limit, which is how the commit groups them); a receiver whose
 * new chain has another number of stages than its group's leaves for a matching muted row or a group of its own, exactly
 * as after a mode change (batch_move_row).  Control plane: synchronises the device; a failure in the planning phase
 * leaves the batch as it was. */
int csdr_demod_batch_set_input_rate(csdr_demod_batch *b, double rate)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (!(rate > 0.0) || !std::isfinite(rate)) return fail(CSDR_EINVAL, "input rate %g", rate);     // before anything records it
    batch_forget_blank(b);
    if (b->groups.empty() || (rate == b->in_rate && !b->rate_change_failed)) { b->in_rate = rate; return CSDR_OK; }
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());                  // control plane: nothing of this batch in flight from here on
    // ---- plan (nothing changes yet): every receiver's new stage count, every group's (its first live row's)
    std::vector<int> stages(b->channels, -1);
    for (int c = 0; c < b->channels; c++) {
        if (b->core_of[c] < 0) continue;
        const DcPlan p = dc_make_plan(rate, b->cfg[c].want_bw);
        if (p.nstages < 0 || p.nstages > DC_MAX_STAGES) return fail(CSDR_EINVAL, "no decimator chain for rate %g", rate);
        stages[c] = p.nstages;
    }
    // (a group keeps the decimation MOST of its live rows get -- the first of them on a tie -- so that as few receivers as
    // possible have to move; rows grouped at the commit share one bandwidth limit and all agree)
    std::vector<int> group_stages(b->groups.size(), -1);
    std::vector<double> group_bw(b->groups.size(), 0.0);
    for (size_t ki = 0; ki < b->groups.size(); ki++) {
        const std::vector<int> &members = b->groups[ki]->members;
        int votes[DC_MAX_STAGES + 1] = {0}, best = -1;
        for (int c : members) if (c >= 0) votes[stages[c]]++;
        for (int c : members) if (c >= 0 && (best < 0 || votes[stages[c]] > votes[best])) best = stages[c];
        group_stages[ki] = best;
        for (int c : members) if (c >= 0 && stages[c] == best) { group_bw[ki] = b->cfg[c].want_bw; break; }
    }
    // ---- the rows that keep their group: in place (a muted row follows its group, it only has to decimate alike)
    std::vector<int> movers;
    for (size_t ki = 0; ki < b->groups.size(); ki++) {
        PlanGroup &G = *b->groups[ki];
        for (size_t q = 0; q < G.members.size(); q++) {
            const int c = G.members[q];
            if (c >= 0 && stages[c] != group_stages[ki]) { movers.push_back(c); continue; }
            // (from the first row that has taken the new rate a failure leaves the groups' rows on DIFFERENT decimations while
            // the staging is sized from row 0: the batch refuses to process until a set_input_rate has gone through -- the
            // same call again finishes the job, every step above is idempotent)
            if (c >= 0) { const int rc = apply_input_rate(G.core, (int)q, b->cfg[c], rate); if (rc) { b->rate_change_failed = true; return rc; } }
            else if (group_stages[ki] >= 0 && csdr_downconvert_batch_set_data_rate(G.core.dc, (int)q, rate, group_bw[ki]) < 0) { b->rate_change_failed = true; return CSDR_EHIP; }
        }
    }
    b->in_rate = rate;
    b->rate_change_failed = false;
    // ---- the others move, with all their state, like a receiver whose new mode decimates differently; the row each
    // leaves behind is muted and takes its old group's new chain
    int err = CSDR_OK;
    std::map<PlanGroup *, double> bw_of;               // (group indices shift when a move empties a group)
    for (size_t ki = 0; ki < b->groups.size(); ki++) bw_of[b->groups[ki].get()] = group_bw[ki];
    for (int c : movers) {
        const int r = b->row_of[c];
        PlanGroup *GA = b->groups[b->core_of[c]].get();
        const bool alone = GA->core.rows == 1;
        const double bw = bw_of[GA];
        const int rc = batch_move_row(b, c, stages[c], [&](ChainCore &k, int row, ChanCfg &cfg) { return apply_input_rate(k, row, cfg, rate); });
        if (rc) { if (!err) err = rc; continue; }
        // (batch_move_row may have dropped the group -- then GA is gone; it drops a group only when every row is muted)
        bool still = false;
        for (auto &g : b->groups) still = still || g.get() == GA;
        if (!alone && still && csdr_downconvert_batch_set_data_rate(GA->core.dc, r, rate, bw) < 0 && !err) err = CSDR_EHIP;
    }
    batch_order(b);
    if (err) b->rate_change_failed = true;               // a receiver that should have moved did not: see above
    return err;
}
/* Configure every channel, then call csdr_demod_batch_commit() once: channels that decimate by
 * the same chain are grouped and run together. */
int csdr_demod_batch_set_demod(csdr_demod_batch *b, int channel, int mode, const csdr_demod_info *info)
{
    if (!b || !info || channel < 0 || channel >= b->channels || mode < 0 || mode > 6)
        return fail(CSDR_EINVAL, "bad argument");
    ChanCfg &c = b->cfg[channel];
    if (b->core_of[channel] >= 0) {
        // already committed.  The reference rebuilds the down-converter only when the MODE changes
        // (demodulator.cpp:111-121); a new mode whose chain has as many stages as the old one stays in its row (the
        // down-converter object holds a plan per row), one with another decimation moves (batch_move_channel)
        DemodInfo di; memcpy(&di, info, sizeof(di));
        if (!device_ok(b->device)) return CSDR_EHIP;
        ChainCore &k = b->core(channel);
        if (c.mode != mode) {
            const double bw = (mode == PC_MODE_LSB || mode == PC_MODE_CWL) ? -di.LowCutmin : di.HiCutmax;
            const int new_stages = dc_make_plan(b->in_rate, bw).nstages;
            int codes[DC_MAX_STAGES];
            const int old_stages = csdr_downconvert_batch_get_stages(k.dc, b->row_of[channel], codes, DC_MAX_STAGES);
            if (new_stages != old_stages) return batch_move_channel(b, channel, mode, di, new_stages);
        }
        return apply_set_demod(k, b->row_of[channel], c, b->in_rate, mode, di);
    }
    memcpy(&c.info, info, sizeof(DemodInfo));
    c.pending = mode;                    // applied at commit
    c.want_bw = (mode == PC_MODE_LSB || mode == PC_MODE_CWL) ? -c.info.LowCutmin : c.info.HiCutmax;
    return CSDR_OK;
}
/* csdr_demod_batch_set_demod for each entry, in array order (include/cutesdr_mi.h).  Same-mode entries on a committed
 * batch gather their filters per plan group; an entry that takes the one-receiver path (a new mode, or any entry before
 * the commit) first sends the gather out, so that the filter objects see the calls in array order as well -- a mover's
 * copy_row and a later host design of a slot both find the earlier entries' jobs queued. */
int csdr_demod_batch_set_demod_many(csdr_demod_batch *b, int n, const int *channel, const int *mode,
                                    const csdr_demod_info *info, int *status)
{
    if (!have_device()) return CSDR_EHIP;
    if (!b || n < 0 || (n > 0 && (!channel || !mode || !info))) return fail(CSDR_EINVAL, "bad handle, negative count or null array");
    for (int i = 0; i < n; i++)
        if (channel[i] < 0 || channel[i] >= b->channels || mode[i] < 0 || mode[i] > 6)
            return fail(CSDR_EINVAL, "entry %d: channel %d, mode %d", i, channel[i], mode[i]);
    if (n == 0) return CSDR_OK;
    if (!device_ok(b->device)) return CSDR_EHIP;
    FilterDefer defer;
    int err = CSDR_OK;
    for (int i = 0; i < n; i++) {
        const int c = channel[i];
        ChanCfg &cfg = b->cfg[c];
        int rc;
        if (b->core_of[c] >= 0 && cfg.mode == mode[i]) {
            DemodInfo di; memcpy(&di, &info[i], sizeof(di));
            rc = apply_set_demod(b->core(c), b->row_of[c], cfg, b->in_rate, mode[i], di, &defer);
        } else {
            rc = defer.flush();
            if (rc == CSDR_OK) rc = csdr_demod_batch_set_demod(b, c, mode[i], &info[i]);
        }
        if (status) status[i] = rc;
        if (rc < 0 && !err) err = rc;
    }
    const int rc = defer.flush();
    return err ? err : rc;
}
// device copies of every group's input-row list, from its members and in_row[]
static int batch_upload_input_rows(csdr_demod_batch *b)
{
    for (auto &g : b->groups) {
        g->row_in_last.resize(g->members.size(), 0);
        for (size_t q = 0; q < g->members.size(); q++)          // (a muted row keeps reading the row it last had)
            if (g->members[q] >= 0) g->row_in_last[q] = b->in_row[g->members[q]];
        CSDR_HIP(hipMemcpy(g->d_rows, g->row_in_last.data(), sizeof(int) * g->row_in_last.size(), hipMemcpyHostToDevice));
    }
    return CSDR_OK;
}
int csdr_demod_batch_set_input_rows(csdr_demod_batch *b, const int *input_row)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (input_row)
        for (int c = 0; c < b->channels; c++)
            if (input_row[c] < 0 || input_row[c] >= b->channels) return fail(CSDR_EINVAL, "input row %d of receiver %d", input_row[c], c);
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());                  // control plane: a call in flight still reads the old lists
    for (int c = 0; c < b->channels; c++) b->in_row[c] = input_row ? input_row[c] : c;
    return b->groups.empty() ? CSDR_OK : batch_upload_input_rows(b);
}
int csdr_demod_batch_commit(csdr_demod_batch *b)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    batch_forget_blank(b);
    if (!device_ok(b->device)) return CSDR_EHIP;
    if (!b->groups.empty()) return fail(CSDR_ESTATE, "already committed");
    std::map<long long, std::vector<int>> by_bw;
    for (int c = 0; c < b->channels; c++) {
        if (b->cfg[c].pending < 0)
            return fail(CSDR_ESTATE, "channel %d has no demodulator configured", c);
        by_bw[(long long)llround(b->cfg[c].want_bw * 1000.0)].push_back(c);
    }
    for (auto &kv : by_bw) {
        const std::vector<int> &chans = kv.second;
        std::unique_ptr<PlanGroup> fresh(new PlanGroup());
        if (fresh->core.init(b->device, (int)chans.size(), b->fft_n) != CSDR_OK) return CSDR_EHIP;
        const int ki = (int)b->groups.size();
        b->groups.push_back(std::move(fresh));
        PlanGroup &g = *b->groups.back();
        g.members = chans;
        CSDR_HIP(hipMalloc((void **)&g.d_rows, sizeof(int) * chans.size()));        // filled by batch_upload_input_rows below
        CSDR_HIP(hipMalloc((void **)&g.d_out_rows, sizeof(int) * chans.size()));
        CSDR_HIP(hipMemcpy(g.d_out_rows, chans.data(), sizeof(int) * chans.size(), hipMemcpyHostToDevice));
        for (size_t r = 0; r < chans.size(); r++) {
            const int c = chans[r];
            b->core_of[c] = ki; b->row_of[c] = (int)r;
            const int mode = b->cfg[c].pending;
            DemodInfo di = b->cfg[c].info;
            csdr_downconvert_batch_set_frequency(g.core.dc, (int)r, 0.0);
            int rc = apply_set_demod(g.core, (int)r, b->cfg[c], b->in_rate, mode, di);
            if (rc) return rc;
        }
    }
    {
        int rc = batch_upload_input_rows(b);
        if (rc) return rc;
    }
    batch_order(b);                                    // heaviest post-chain first, and on the highest-priority stream
    return b->groups.size() > 1 ? batch_plumbing(b, true) : CSDR_OK;
}
/* Pipelined mode.  on != 0 (1, 2 and 3 mean the same): a process call only enqueues on internal streams -- the strict
 * mode's schedule, one down-converter at a time and each group's filter in queue order behind it, carried across calls:
 * the first group's next down-converter follows the last group's, the post-chains run in streams of their own
 * (run_chained).  In the caller's stream order the INPUT buffer and the OUTPUT rows of call k are complete after process
 * call k+1 (everything after csdr_demod_batch_flush).  Results are identical to the strict mode. */
int csdr_demod_batch_set_pipelined(csdr_demod_batch *b, int on)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (b->groups.empty()) return fail(CSDR_ESTATE, "commit first");
    if (on && b->taps) return fail(CSDR_ESTATE, "stage taps need the strict mode (csdr_demod_batch_set_taps(b, 0) first)");
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());
    if (on) {                                          // a single plan group normally runs on the caller's stream
        int rc = batch_plumbing(b, true);
        if (rc) return rc;
    }
    for (auto &g : b->groups) {
        g->prev_join = false;
        g->core.ch.post_busy[0] = g->core.ch.post_busy[1] = false;
    }
    b->have_last_dc = false;
    b->pipelined = on != 0;
    return CSDR_OK;
}
/* stream-orders the caller's stream behind everything the batch has in flight (pipelined mode: the post-chain
 * of the last call) */
int csdr_demod_batch_flush(csdr_demod_batch *b, void *stream)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (!device_ok(b->device)) return CSDR_EHIP;
    return batch_late_join(b, stream);
}
/* internal (csdr_demod_shard_process_shared): orders `stream` behind the batch's reads of the INPUT of its previous
 * call.  Strict mode: nothing to do (a process call joins the caller's stream itself).  Pipelined mode: the previous
 * call's down-converters run on the batch's own streams and the caller's stream joins them only inside the NEXT process
 * call -- too late for a caller that refills the input buffer on that stream first. */
int csdr__demod_batch_wait_input_free(csdr_demod_batch *b, void *stream)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (!b->pipelined) return CSDR_OK;
    if (!device_ok(b->device)) return CSDR_EHIP;
    return batch_late_join(b, stream);
}
int csdr_demod_batch_set_freq(csdr_demod_batch *b, int channel, double freq)
{
    if (!b || channel < 0 || channel >= b->channels) return fail(CSDR_EINVAL, "bad argument");
    if (b->core_of[channel] < 0) return fail(CSDR_ESTATE, "commit first");
    ChainCore &k = b->core(channel);
    csdr_downconvert_batch_set_cw_offset(k.dc, b->row_of[channel], b->cfg[channel].cw_off);
    return csdr_downconvert_batch_set_frequency(k.dc, b->row_of[channel], freq);
}
double csdr_demod_batch_get_output_rate(csdr_demod_batch *b, int channel)
{
    if (!b || channel < 0 || channel >= b->channels) return 0.0;
    return b->cfg[channel].out_rate;
}
double csdr_demod_batch_get_smeter_ave(csdr_demod_batch *b, int channel)
{
    if (!b || channel < 0 || channel >= b->channels || b->core_of[channel] < 0) return 0.0;
    return b->core(channel).pc.smeter_ave(b->row_of[channel]);
}
/* CSMeter::GetAve / GetPeak of every channel into device arrays indexed by channel (either may be NULL);
 * reading the peak resets it, as GetPeak does (smeter.cpp:98-103).  Asynchronous on `stream`. */
int csdr_demod_batch_get_smeter_all(csdr_demod_batch *b, float *d_ave, float *d_peak, void *stream)
{
    if (!b || (!d_ave && !d_peak)) return fail(CSDR_EINVAL, "bad argument");
    if (b->groups.empty()) return fail(CSDR_ESTATE, "commit first");
    if (!device_ok(b->device)) return CSDR_EHIP;
    int rcf = csdr_demod_batch_flush(b, stream);         // pipelined mode: behind the last call's post-chain
    if (rcf) return rcf;
    for (auto &g : b->groups)
        CSDR_HIP(smeter_collect_launch(g->core.pc.d_chan, g->core.rows, g->d_out_rows, d_ave, d_peak, (hipStream_t)stream));
    return CSDR_OK;
}
}  // extern "C"

// Strict mode, several groups: every down-converter behind the first starts while the previous group's filter, S-meter,
// peaks and walk hold part of the chip, and its workgroups are long (one wave walks its whole segment: 350 us) -- the
// ones that do not fit at once start only when the first ones END, a second round that costs a whole workgroup time
// for a few hundred stragglers (tools/wg_trace.py: 4031 of 4080 at once for the second group, 3277 of 4042 for the
// third).  Alone the kernel loses 4-7 % at 13 / 12 waves per CU instead of 16 (tools/experiments/r6_k2_grid.sh), so the
// later groups are cut into 13 x CUs and 12 x CUs workgroups and run as ONE round: strict C4 step 1.75-1.78 -> 1.67 ms.
// CSDR_DC_WGS_CORUN="a[,b]" overrides (second group's, later groups' workgroups; 0 = one full round for all).
// Returns the workgroups of the group at place `oi` (> 0) of the launch order; read once, sized from the first batch's device.
static long corun_wgs(int device, size_t oi)
{
    static long wgs[2] = {-1, -1};
    if (wgs[0] < 0) {
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        const char *e = getenv("CSDR_DC_WGS_CORUN");
        wgs[1] = e && strchr(e, ',') ? atol(strchr(e, ',') + 1) : (e ? atol(e) : 12L * cus);
        wgs[0] = e ? atol(e) : 13L * cus;
    }
    return wgs[oi > 1 ? 1 : 0];
}

// The pipelined schedule (csdr_demod_batch_set_pipelined): one down-converter at a time, across calls; every group's
// post-chain in a stream of its own, joined by the NEXT call.
static int run_chained(csdr_demod_batch *b, ChainIn in, ChainOut out, hipStream_t caller)
{
    int pr_lo = 0, pr_hi = 0;
    CSDR_HIP(hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi));
    for (auto &g : b->groups) { const int rc = g->post_plumbing(pr_hi); if (rc) return rc; }
    // the first group's down-converter runs beside the previous call's last walks: the co-run grid for it too
    static const long first_wgs = getenv("CSDR_PIPE_FIRST_WGS") ? atol(getenv("CSDR_PIPE_FIRST_WGS")) : -1;
    const size_t ng = b->groups.size();
    int err = 0;
    for (size_t oi = 0; oi < ng; oi++) {
        PlanGroup &g = *b->groups[b->order[oi]];
        ChainCore &k = g.core;
        long wgs = 0;
        if (ng > 1 && oi > 0) wgs = corun_wgs(b->device, oi);
        else if (ng > 1 && b->have_last_dc) wgs = first_wgs >= 0 ? first_wgs : corun_wgs(b->device, 2);
        csdr__downconvert_batch_set_wgs(k.dc, wgs);
        CSDR_HIP(hipStreamWaitEvent(g.stream, b->fork, 0));
        // the caller's stream catches up with the PREVIOUS call behind this call's fork event (the pipelined contract)
        { const int rcj = g.late_join(caller); if (rcj) return rcj; }
        // one down-converter at a time, across calls: behind the previous group's, the first behind the previous call's last
        hipEvent_t after = nullptr;
        if (oi > 0) after = b->groups[b->order[oi - 1]]->dc_done;
        else if (b->have_last_dc) after = b->groups[b->order[ng - 1]]->dc_done;
        k.pc.sm_borrow = nullptr; k.pc.sm_own_side = false;
        in.d_in_rows = g.d_rows; out.d_out_rows = g.d_out_rows;
        hipStream_t joined = g.stream;
        const int rc = k.step_split(in, out, g.stream, g.post_stream, after, g.dc_done, &joined);
        if (rc < 0 && !err) err = rc;
        CSDR_HIP(hipEventRecord(g.join, joined));
        g.prev_join = true;
    }
    b->have_last_dc = !err;
    return err ? err : CSDR_OK;
}

// The strict schedule: the groups' down-converters run one after the other (each fills the chip on its own) and what
// follows a group's down-converter overlaps the next group's.  Several groups run forked, each on its own stream; one
// group runs on the caller's.
static int run_strict(csdr_demod_batch *b, ChainIn in, ChainOut out, hipStream_t caller)
{
    const size_t ng = b->groups.size();
    const bool forked = ng > 1;
    int err = 0;
    for (size_t oi = 0; oi < ng; oi++) {
        PlanGroup &g = *b->groups[b->order[oi]];
        ChainCore &k = g.core;
        hipStream_t st = forked ? g.stream : caller;
        csdr__downconvert_batch_set_wgs(k.dc, oi > 0 ? corun_wgs(b->device, oi) : 0);
        if (forked) CSDR_HIP(hipStreamWaitEvent(st, b->fork, 0));
        hipEvent_t prev_dc = oi > 0 ? (hipEvent_t)b->groups[b->order[oi - 1]]->dc_done : nullptr;
        in.d_in_rows = g.d_rows; out.d_out_rows = g.d_out_rows;
        // several groups: the LAST group's filter, S-meter, peaks and walk are the end of the call, and its S-meter -- which
        // nothing in the call waits for -- goes to the first group's stream, long idle by then: 30 us less on the critical path
        k.pc.sm_borrow = oi > 0 && oi + 1 == ng ? b->groups[b->order[0]]->stream : nullptr;
        // ONE group (a single receiver, or receivers of one plan): the call is that group's walk from end to end, and the
        // S-meter scan beside it on a side stream of its own is 6 % of a C2 / C5 call
        k.pc.sm_own_side = !forked;
        const int rc = k.step(in, out, st, prev_dc, forked ? (hipEvent_t)g.dc_done : nullptr);
        k.pc.sm_borrow = nullptr;
        if (rc < 0 && !err) err = rc;
        if (forked) {                                   // join even after an error: the caller's stream stays ordered
            CSDR_HIP(hipEventRecord(g.join, st));
            CSDR_HIP(hipStreamWaitEvent(caller, g.join, 0));
        }
    }
    return err ? err : CSDR_OK;
}

/* d_in: [channels][in_stride] complex fp32; d_out: [channels][out_stride] fp32 mono audio.
 * Chunking: one call = one pass of the chain over n_per_channel samples (the host form uses
 * m_InBufLimit-sized passes; decimator, filter and post-chain do not depend on the chunking, word for word, for calls
 * of whole 512-sample tiles -- the decimator re-anchors its oscillator on an absolute grid --, the squelch
 * decision is taken once per FastFIR hop either way).  Asynchronous. */
static int demod_batch_run(csdr_demod_batch *b, const float *d_in, long long in_stride, int n_per_channel,
                           float *d_out, long long out_stride, void *stream, bool stereo,
                           const void *d_packets = nullptr, int pkt_len = 0, const DcBlank *blank = nullptr)
{
    if (!b || (!d_in && !d_packets) || !d_out) return fail(CSDR_EINVAL, "bad argument");
    batch_forget_blank(b);                               // (the blanked entry points record their call behind this)
    if (b->groups.empty()) return fail(CSDR_ESTATE, "commit first");
    if (b->rate_change_failed)
        return fail(CSDR_ESTATE, "a csdr_demod_batch_set_input_rate failed half way (rows of one group decimate differently): call it again");
    if (!device_ok(b->device)) return CSDR_EHIP;
    hipStream_t caller = (hipStream_t)stream;
    if (b->groups.size() > 1 || b->pipelined) CSDR_HIP(hipEventRecord(b->fork, caller));      // the groups run on their own streams
    const ChainIn in{d_in, (long)in_stride, nullptr, n_per_channel, d_packets, pkt_len, blank};
    const ChainOut out{d_out, (long)out_stride, nullptr, stereo};
    return b->pipelined ? run_chained(b, in, out, caller) : run_strict(b, in, out, caller);
}
// the caller's blanker must be as wide as the chain and on its device: the mask has one row per receiver, and the
// down-converter indexes the blanker's state and history by input row
static int batch_blanker_fits(csdr_demod_batch *b, csdr_noiseproc_batch *nb)
{
    int ch = 0, dev = -1;
    const int rc = csdr__noiseproc_batch_shape(nb, &ch, &dev);
    if (rc) return rc;
    if (ch != b->channels || dev != b->device)
        return fail(CSDR_EINVAL, "blanker of %d channels on device %d given to a chain of %d on device %d", ch, dev,
                    b->channels, b->device);
    return CSDR_OK;
}
// the blanker's mask rows of a call of n samples per channel (fused form): [channels][mask_cap] words, grown when needed
static int batch_mask_rows(csdr_demod_batch *b, long n)
{
    const long words = (n + 31) / 32 + 64;
    if (words > b->mask_cap) {
        CSDR_HIP(hipDeviceSynchronize());
        if (b->d_mask) (void)hipFree(b->d_mask);
        b->d_mask = nullptr; b->mask_cap = 0;
        CSDR_HIP(hipMalloc((void **)&b->d_mask, (size_t)b->channels * words * sizeof(unsigned)));
        b->mask_cap = words;
    }
    b->blank.mask = b->d_mask; b->blank.mask_stride = b->mask_cap;
    return CSDR_OK;
}

extern "C" {

int csdr_demod_batch_process(csdr_demod_batch *b, const float *d_in, long long in_stride, int n_per_channel,
                             float *d_out, long long out_stride, void *stream)
{ return demod_batch_run(b, d_in, in_stride, n_per_channel, d_out, out_stride, stream, false); }
/* the stereo overload of CDemodulator::ProcessData (demodulator.cpp:221-273) for every channel:
 * d_out_iq [channels][out_stride] complex fp32 (out_stride in complex samples) */
int csdr_demod_batch_process_stereo(csdr_demod_batch *b, const float *d_in, long long in_stride, int n_per_channel,
                                    float *d_out_iq, long long out_stride, void *stream)
{ return demod_batch_run(b, d_in, in_stride, n_per_channel, d_out_iq, out_stride, stream, true); }
int csdr_demod_batch_process_packets(csdr_demod_batch *b, const void *d_packets, int npackets, int pkt_len,
                                     struct csdr_noiseproc_batch *nb, float *d_out, long long out_stride,
                                     void *stream)
{
    if (!b || !d_packets || !d_out || npackets < 0) return fail(CSDR_EINVAL, "bad argument");
    if (pkt_len != 1028 && pkt_len != 1444) return fail(CSDR_EINVAL, "packet length %d", pkt_len);
    if (b->groups.empty()) return fail(CSDR_ESTATE, "commit first");
    if (npackets == 0) return CSDR_OK;
    if (!device_ok(b->device)) return CSDR_EHIP;
    const long n = (long)npackets * (pkt_len == 1444 ? 240 : 256);
    if (n > 0x7fffffffL) return fail(CSDR_EINVAL, "%d datagrams are more samples than one call can take", npackets);
    if (!nb)        // the down-converter decodes the datagrams in its own loads: no unpacked copy, no extra pass
        return demod_batch_run(b, nullptr, 0, (int)n, d_out, out_stride, stream, false, d_packets, pkt_len);
    { const int rcs = batch_blanker_fits(b, nb); if (rcs) return rcs; }
    batch_forget_blank(b);                               // the mask and the blanker's halves are about to change
    // With the blanker.  The internal buffers below (mask / blanked samples) are single-buffered, and the blanker's
    // history halves alternate per call: in pipelined mode the down-converters of the PREVIOUS call (on the batch's own
    // streams) may still be reading them, and the caller's stream -- on which the blanker of this call runs -- has not
    // joined them yet (demod_batch_run does that, later)
    if (b->pipelined) { const int rcj = batch_late_join(b, stream); if (rcj) return rcj; }
    // FUSED (default): the blanker decides, the down-converter applies -- noiseblank_kernel leaves one bit per sample,
    // downconv_kernel<.., BLK> reads the datagram sample delay_n + 1 behind and zeroes it under the mask in its own
    // load.  No blanked copy of the input: 8 B written + 8 B read back per sample less, and one input stream less in
    // the blanker ("fuses naturally into the NCO kernel's load").  CSDR_BLANK_FUSED=0: the two-pass form.
    static const bool fused = !(getenv("CSDR_BLANK_FUSED") && atoi(getenv("CSDR_BLANK_FUSED")) == 0);
    if (fused) {
        { const int rcm = batch_mask_rows(b, n); if (rcm) return rcm; }
        int rc = csdr__noiseproc_batch_mask(nb, nullptr, 0, d_packets, npackets, pkt_len, (int)n, b->d_mask, b->mask_cap,
                                            &b->blank.state, &b->blank.hist, stream);
        if (rc < 0) return rc;
        rc = demod_batch_run(b, nullptr, 0, (int)n, d_out, out_stride, stream, false, d_packets, pkt_len, &b->blank);
        if (rc == CSDR_OK) b->last_blank = BlankCall{BLANK_CALL_PACKETS, d_packets, pkt_len, (int)n};
        return rc;
    }
    // two passes: the blanker decodes the datagrams in ITS loads and leaves blanked fp32 samples for the chain
    if (n > b->raw_cap) {
        CSDR_HIP(hipDeviceSynchronize());
        if (b->d_blank) (void)hipFree(b->d_blank);
        b->d_blank = nullptr; b->raw_cap = 0;
        CSDR_HIP(hipMalloc((void **)&b->d_blank, (size_t)b->channels * n * 8));
        b->raw_cap = n;
    }
    int rc = csdr__noiseproc_batch_process_packets(nb, d_packets, npackets, pkt_len, b->d_blank, b->raw_cap, stream);
    if (rc < 0) return rc;
    rc = demod_batch_run(b, b->d_blank, b->raw_cap, (int)n, d_out, out_stride, stream, false);
    b->last_two_pass = rc == CSDR_OK;
    return rc;
}
/* The strict / pipelined pass on fp32 rows with CNoiseProc's blanker in front (what CSdrInterface::ProcessIQData runs in
 * place before the chain, sdrinterface.cpp:884), FUSED like the datagram form: the blanker kernel leaves one bit per sample,
 * the down-converter takes the delayed sample from d_in itself and zeroes it under the mask -- no blanked copy of the
 * input is written or read. */
int csdr_demod_batch_process_blanked(csdr_demod_batch *b, const float *d_in, long long in_stride, int n_per_channel,
                                     struct csdr_noiseproc_batch *nb, float *d_out, long long out_stride, void *stream)
{
    if (!b || !d_in || !d_out || !nb || n_per_channel < 0) return fail(CSDR_EINVAL, "bad argument");
    if (b->groups.empty()) return fail(CSDR_ESTATE, "commit first");
    if (n_per_channel == 0) return CSDR_OK;
    if (!device_ok(b->device)) return CSDR_EHIP;
    for (auto &g : b->groups)                                // rows shared between receivers would be blanked once per reader
        for (int c : g->members)
            if (c >= 0 && b->in_row[c] != c)
                return fail(CSDR_ESTATE, "process_blanked: every receiver reads its own row (csdr_demod_batch_set_input_rows is off)");
    { const int rcs = batch_blanker_fits(b, nb); if (rcs) return rcs; }
    const long n = n_per_channel;
    batch_forget_blank(b);
    // (the single-buffered mask, as in process_packets)
    if (b->pipelined) { const int rcj = batch_late_join(b, stream); if (rcj) return rcj; }
    { const int rcm = batch_mask_rows(b, n); if (rcm) return rcm; }
    int rc = csdr__noiseproc_batch_mask(nb, d_in, in_stride, nullptr, 0, 0, (int)n, b->d_mask, b->mask_cap,
                                        &b->blank.state, &b->blank.hist, stream);
    if (rc < 0) return rc;
    rc = demod_batch_run(b, d_in, in_stride, (int)n, d_out, out_stride, stream, false, nullptr, 0, &b->blank);
    if (rc == CSDR_OK) b->last_blank = BlankCall{BLANK_CALL_ROWS, d_in, in_stride, (int)n};
    return rc;
}
/* internal (capi_fft.hip: the display behind a blanked chain call): what the LAST blanked call's mask pass left -- mask,
 * blanker state and the history half it read -- with the record of that call's input, the batch's width and device.
 * CSDR_ESTATE when the last process call was not a fused blanked one. */
int csdr__demod_batch_last_blank(csdr_demod_batch *b, DcBlank *blank, BlankCall *call, int *channels, int *device)
{
    if (!b || !blank || !call) return fail(CSDR_EINVAL, "bad argument");
    if (b->last_two_pass)
        return fail(CSDR_ESTATE, "the chain's last call ran the two-pass blanker (CSDR_BLANK_FUSED=0): it left no mask");
    if (b->last_blank.form == BLANK_CALL_NONE)
        return fail(CSDR_ESTATE, "the chain's last call was not a blanked one (csdr_demod_batch_process_blanked, or _process_packets with a blanker)");
    *blank = b->blank; *call = b->last_blank;
    if (channels) *channels = b->channels;
    if (device) *device = b->device;
    return CSDR_OK;
}
/* internal (capi_fft.hip, capi_spurcal.hip): the same for a reader `what` of `channels` receivers on `device` that is
 * handed the input (form, src, stride, n) -- it must be THAT call's input, and the reader the chain's width on its
 * device.  CSDR_ESTATE as above, CSDR_EINVAL when anything differs; nothing changed either way. */
int csdr__demod_batch_blank_for(csdr_demod_batch *b, const char *what, int channels, int device, int form, const void *src,
                                long long stride, int n, DcBlank *blank)
{
    BlankCall call;
    int b_channels = 0, b_device = -1;
    const int rc = csdr__demod_batch_last_blank(b, blank, &call, &b_channels, &b_device);
    if (rc) return rc;
    if (b_channels != channels || b_device != device)
        return fail(CSDR_EINVAL, "%s of %d channels on device %d behind a chain of %d on device %d", what, channels, device,
                    b_channels, b_device);
    if (call.form != form)
        return fail(CSDR_EINVAL, "the chain's last blanked call took %s", call.form == BLANK_CALL_PACKETS ? "datagrams" : "fp32 rows");
    if (call.src != src || call.stride != stride || call.n != n)
        return fail(CSDR_EINVAL, "not the input of the chain's last blanked call (buffer, %s or count differ)",
                    form == BLANK_CALL_PACKETS ? "packet length" : "stride");
    return CSDR_OK;
}
/* internal (diagnostics: tools/experiments/r6_repro_mode3.py): how fast each plan group's own buffers stream -- a
 * device-to-device copy of the filter-output rows into the spare rows, timed with events, per group in the batch's launch
 * order; us_out[k] = microseconds of the k-th group's copy, bytes_out[k] its size.  Synchronises. */
int csdr__demod_batch_probe(csdr_demod_batch *b, double *us_out, double *bytes_out, int cap)
{
    if (!b || !us_out || !bytes_out) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CSDR_HIP(hipEventCreate(&e0)); CSDR_HIP(hipEventCreate(&e1));
    int n = 0;
    for (size_t oi = 0; oi < b->groups.size() && n < cap; oi++, n++) {
        ChainCore &k = b->groups[b->order[oi]]->core;
        const size_t bytes = (size_t)k.rows * (size_t)k.cap * 8;
        us_out[n] = 0.0; bytes_out[n] = (double)bytes;
        if (!k.d_filt || !k.d_agc || !bytes) continue;
        for (int rep = 0; rep < 3; rep++) CSDR_HIP(hipMemcpyAsync(k.d_agc, k.d_filt, bytes, hipMemcpyDeviceToDevice, nullptr));
        CSDR_HIP(hipEventRecord(e0, nullptr));
        for (int rep = 0; rep < 10; rep++) CSDR_HIP(hipMemcpyAsync(k.d_agc, k.d_filt, bytes, hipMemcpyDeviceToDevice, nullptr));
        CSDR_HIP(hipEventRecord(e1, nullptr));
        CSDR_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        CSDR_HIP(hipEventElapsedTime(&ms, e0, e1));
        us_out[n] = ms * 100.0;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return n;
}
/* internal (tests): the batch's form -- 3 pipelined (bit 0 pipelined, bit 1 the chained schedule: the only one), 0 strict */
int csdr__demod_batch_form(csdr_demod_batch *b)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    return b->pipelined ? 3 : 0;
}
/* stage taps of a batch's receivers: see include/cutesdr_mi.h */
int csdr_demod_batch_set_taps(csdr_demod_batch *b, int mask)
{
    if (!b || mask < 0 || mask > 15) return fail(CSDR_EINVAL, "bad argument");
    if (b->groups.empty()) return fail(CSDR_ESTATE, "commit first");
    if (mask && b->pipelined) return fail(CSDR_ESTATE, "stage taps need the strict mode");
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());
    for (auto &g : b->groups) { g->core.taps = mask; g->core.tap1_n = 0; }
    b->taps = mask;
    return CSDR_OK;
}
int csdr_demod_batch_get_tap(csdr_demod_batch *b, int channel, int profile, float *out, int cap)
{
    if (!b || channel < 0 || channel >= b->channels || profile < 1 || profile > 3 || cap < 0 || (cap && !out))
        return fail(CSDR_EINVAL, "bad argument (PROFILE_4 is the caller's own output row)");
    if (b->core_of[channel] < 0) return fail(CSDR_ESTATE, "commit first");
    ChainCore &k = b->core(channel);
    if (!(k.taps & (1 << (profile - 1)))) return fail(CSDR_ESTATE, "tap %d is not switched on", profile);
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());
    const int r = b->row_of[channel];
    const int n = profile == 1 ? k.tap1_n : k.last_out;
    if (2 * n > cap) return fail(CSDR_EINVAL, "tap %d holds %d floats, room for %d", profile, 2 * n, cap);
    const float *src = profile == 1 ? k.d_tap1 + 2 * (size_t)r * k.tap1_cap
                                    : (profile == 2 ? k.d_filt : k.d_agc) + 2 * (size_t)r * k.cap;
    if (n) CSDR_HIP(hipMemcpy(out, src, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 2 * n;
}
int csdr_demod_batch_group_count(csdr_demod_batch *b, int *rows)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (rows) { *rows = 0; for (auto &g : b->groups) *rows += g->core.rows; }
    return (int)b->groups.size();
}
/* audio samples channel `channel` received in the last process call */
int csdr_demod_batch_out_count(csdr_demod_batch *b, int channel)
{
    if (!b || channel < 0 || channel >= b->channels || b->core_of[channel] < 0) return fail(CSDR_EINVAL, "bad argument");
    return b->core(channel).last_out;
}

}  // extern "C"
