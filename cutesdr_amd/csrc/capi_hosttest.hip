// capi_hosttest.hip -- test-only exports of the HOST-side setup math (no GPU needed), so that the
// CPU test suite can check filter design, stage selection and the spectrum-order bookkeeping
// against the test-side checker.  Not part of the public ABI (csdr__ prefix, absent from cutesdr_mi.h).
#include "capi_common.hpp"
#include "host_math.hpp"
#include "dc_host.hpp"
#include "pc_host.hpp"
#include "display_plan.hpp"
#include "testgen_host.hpp"
#include "fastfir_kernels.h"
#include <cstring>

using namespace csdr;

extern "C" {

int csdr__host_fastfir_design(int n, double flo, double fhi, double off, double fs, double *h_out)
{
    std::vector<cd> H;
    if (!fastfir_design(n, flo, fhi, off, fs, H)) return -1;
    memcpy(h_out, H.data(), sizeof(cd) * n);
    return 0;
}
// what csdr_fastfir_batch_setup_many does per entry on the host: 0 and the two doubles of the design job, or -1 (rejected)
int csdr__host_design_job(double flo, double fhi, double off, double fs, double *nfc, double *nfs)
{
    return fastfir_design_job(flo, fhi, off, fs, *nfc, *nfs) ? 0 : -1;
}
int csdr__host_fastfir_bin_of(int log2n, int t, int r) { return fastfir_bin_of(log2n, t, r); }

int csdr__host_dc_plan(double in_rate, double bw, int *codes, double *out_rate, int *warmup)
{
    DcPlan p = dc_make_plan(in_rate, bw);
    for (int i = 0; i < p.nstages; i++) codes[i] = p.kind[i];
    *out_rate = p.out_rate; *warmup = p.W;
    return p.nstages;
}
// expanded taps of stage s as the dense vector h[0..L-1] (float precision as uploaded)
int csdr__host_dc_stage_taps(double in_rate, double bw, int s, double *h)
{
    DcPlan p = dc_make_plan(in_rate, bw);
    if (s < 0 || s >= p.nstages) return -1;
    const DcStage &st = p.st[s];
    const int L = st.hist + (p.kind[s] == 3 ? 2 : 1);
    for (int i = 0; i < L; i++) h[i] = 0;
    if (st.center >= 0) h[st.center] = st.ccoef;
    for (int q = 0; q < st.npairs; q++) { h[st.a[q]] = st.c[q]; h[st.b[q]] = st.c[q]; }
    return L;
}
void csdr__host_dc_nco(double freq, double cw, double in_rate, unsigned long long *inc, double *stored)
{
    DcHostChan c;
    c.in_rate = in_rate; c.cw_offset = cw;
    c.set_frequency(freq);
    *inc = c.inc; *stored = c.nco_freq;
}
int csdr__host_fir_design(int kind, double scale, double astop, double fpass, double fstop, double fs,
                          double hilbert_off, double *coef, double *icoef, double *qcoef)
{
    HostFir f;
    if (kind == 0) f.init_lp(scale, astop, fpass, fstop, fs);
    else f.init_hp(scale, astop, fpass, fstop, fs);
    if (hilbert_off != 0.0) f.gen_hilbert(hilbert_off);
    for (int i = 0; i < f.ntaps; i++) { coef[i] = f.coef[i]; icoef[i] = f.icoef[i]; qcoef[i] = f.qcoef[i]; }
    return f.ntaps;
}
void csdr__host_iir_design(int kind, double f0, double q, double fs, double *c5)
{
    PcIir f;
    iir_design(f, kind, f0, q, fs);
    c5[0] = f.b0; c5[1] = f.b1; c5[2] = f.b2; c5[3] = f.a1; c5[4] = f.a2;
}
// CAgc::SetParameters derived values: knee, slope, fixed gain, manual gain, 4 alphas, delay, window, hang time
void csdr__host_agc_params(int on, int hang, int thresh, int manual, int slope, int decay, double fs, double *out12)
{
    HostAgc h;
    PcAgc d;
    memset(&d, 0, sizeof(d));
    h.set(d, on != 0, hang != 0, thresh, manual, slope, decay, fs);
    out12[0] = d.knee; out12[1] = d.gain_slope; out12[2] = d.fixed_gain; out12[3] = d.manual_gain;
    out12[4] = d.att_rise; out12[5] = d.att_fall; out12[6] = d.dec_rise; out12[7] = d.dec_fall;
    out12[8] = d.dly_n; out12[9] = d.win_n; out12[10] = d.hang_time; out12[11] = 0;
}

// the display stream's frame planner (display_plan.hpp): state in = {pos, skip, counter, gated, ready};
// out = {start, step, count, pos, skip, counter, gated, ready}
void csdr__host_display_plan(const int *state5, long long n, int N, long long *out8)
{
    DisplayState s;
    s.pos = state5[0]; s.skip = state5[1]; s.counter = state5[2]; s.gated = state5[3]; s.ready = state5[4];
    const DisplayPlan p = display_plan(s, n, N);
    out8[0] = p.start; out8[1] = p.step; out8[2] = p.count;
    out8[3] = p.next.pos; out8[4] = p.next.skip; out8[5] = p.next.counter; out8[6] = p.next.gated; out8[7] = p.next.ready;
}
int csdr__host_display_skip_value(double sample_rate, int fft_size, int max_display_rate)
{
    return display_skip_value(sample_rate, fft_size, max_display_rate);
}

// the batch signal generator's host logic (testgen_host.hpp): the crossing helper, the pulse pattern, and one
// generator's state machine evaluated on the CPU with the kernel's integer formulas
unsigned long long csdr__host_tg_first_crossing(double x0, double d, double limit, int strict, double *value)
{
    return tg::first_crossing(x0, d, limit, strict != 0, value);
}
double csdr__host_tg_value_at(double x0, double d, unsigned long long index) { return tg::value_at(x0, d, index); }
void csdr__host_tg_pulse_pattern(double fs, double period, double width, unsigned long long *K, unsigned long long *W)
{
    tg::Gen g;
    g.fs = fs; g.period = period; g.width = width;
    g.pulse_pattern();
    *K = g.K; *W = g.W;
}
void *csdr__host_tg_create(void) { tg::Gen *g = new tg::Gen(); g->reset(); g->on = true; return g; }
void csdr__host_tg_destroy(void *h) { delete (tg::Gen *)h; }
// what: 0 start, 1 stop, 2 rate, 3 width, 4 period, 5 signal power, 6 noise power, 7 reset
void csdr__host_tg_slot(void *h, int what, double v)
{
    tg::Gen &g = *(tg::Gen *)h;
    switch (what) {
    case 0: g.on_sweep_start(v); break;
    case 1: g.on_sweep_stop(v); break;
    case 2: g.on_sweep_rate(v); break;
    case 3: g.on_pulse_width(v); break;
    case 4: g.on_pulse_period(v); break;
    case 5: g.on_signal_pwr(v); break;
    case 6: g.on_noise_pwr(v); break;
    default: g.reset(); break;
    }
}
// n samples at rate fs: phase[j] (top 64 bits of the turn fraction) and gate[j] of every sample, as the kernel
// evaluates them; returns the launches the call would take
int csdr__host_tg_run(void *h, int n, double fs, unsigned long long *phase, int *gate)
{
    tg::Gen &g = *(tg::Gen *)h;
    if (g.fs != fs) { g.fs = fs; g.pulse_valid = false; g.reset(); }
    tg::ChanParam p;
    g.pulse((uint32_t)n, p);
    uint32_t done = 0;
    int launches = 0;
    while (done < (uint32_t)n) {
        p.nseg = 0;
        const uint32_t lo = done;
        done += g.advance(done, (uint32_t)n - done, p);
        launches++;
        for (uint32_t j = lo; j < done; j++) {
            uint32_t s = 0;
            for (uint32_t k = 1; k < p.nseg; k++) s += p.seg_start[k] <= j;
            const uint64_t t = j - p.seg_start[s];
            const tg::u128 P = (((tg::u128)p.seg_p[s][1] << 64) | p.seg_p[s][0])
                + (((tg::u128)p.seg_d[s][1] << 64) | p.seg_d[s][0]) * (tg::u128)t
                + (((tg::u128)p.seg_d2[s][1] << 64) | p.seg_d2[s][0]) * (tg::u128)(t * (t - 1) / 2);
            phase[j] = (uint64_t)(P >> 64);
            const uint64_t m = (uint64_t)j + 1;
            const uint64_t pos = m < p.wrap1 ? p.pos0 + m : (m - p.wrap1) % p.period;
            gate[j] = !p.gate_on || pos < p.width;
        }
    }
    return launches;
}

}  // extern "C"
