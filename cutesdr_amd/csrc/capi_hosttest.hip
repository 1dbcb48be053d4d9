// capi_hosttest.hip -- test-only exports of the HOST-side setup math (no GPU needed), so that the
// CPU test suite can check filter design, stage selection and the spectrum-order bookkeeping
// against the test-side checker.  Not part of the public ABI (csdr__ prefix, absent from cutesdr_mi.h).
#include "capi_common.hpp"
#include "host_math.hpp"
#include "dc_host.hpp"
#include "pc_host.hpp"
#include "display_plan.hpp"
#include "testgen_host.hpp"
#include "scope_host.hpp"
#include "plotter_host.hpp"
#include "seq_host.hpp"
#include "spurcal_host.hpp"
#include "nb_host.hpp"
#include "fastfir_kernels.h"
#include "fft_core.hpp"
#include <cstring>
#include <vector>

using namespace csdr;

// host builds of fft_core.hpp's real-gain butterflies (the plain C++ forms of the same templates the kernel uses).
// x4 / g4: four complex points in network order and their four real gains; out4 = dit_head4_gain of them
template <int SIGN> static void host_head4_gain(const float *x4, const float *g4, float *out4)
{
    v2f x[4];
    for (int q = 0; q < 4; q++) x[q] = v2f{x4[2 * q], x4[2 * q + 1]};
    dit_head4_gain<0, 4, SIGN>(x, v2f{g4[0], g4[1]}, v2f{g4[2], g4[3]});
    for (int q = 0; q < 4; q++) { out4[2 * q] = x[q].x; out4[2 * q + 1] = x[q].y; }
}
// in: R complex points in NATURAL order; out: rows R/4 ... 3R/4 - 1 of their unnormalised DFT of sign `sign`, computed as
// the overlap-save kernel's pass I3 does: head groups, (R = 32: the middle stage,) dit_tail_middle
template <int R, int SIGN> static void host_dft_middle(const float *in, float *out)
{
    v2f x[R];
    for (int n = 0; n < R; n++) x[bitrev<R>(n)] = v2f{in[2 * n], in[2 * n + 1]};
    static_for<0, R / 4>([&](auto G) { dit_head4<G.value, R, SIGN>(x); });
    if constexpr (R == 32) dit_single<8, 32, SIGN>(x);
    static_for<0, R / 4>([&](auto I) { dit_tail_middle<I.value, R, SIGN>(x); });
    for (int r = 0; r < R / 2; r++) { out[2 * r] = x[R / 4 + r].x; out[2 * r + 1] = x[R / 4 + r].y; }
}
// host builds of the radix-4 tail groups (dit_tail_r4 / dit_tail_middle_r4).  One group: in4 = the group's four points
// A, B, C, D (positions I, I + R/4, I + R/2, I + 3R/4 of the network in front of its last two stages), out4 = the same
// positions afterwards (middle: only positions 1 and 2 are finished, 0 and 3 come back as they went in)
template <int R, int SIGN> static int host_tail_r4(int i, int middle, const float *in4, float *out4)
{
    int done = -1;
    static_for<0, R / 4>([&](auto I) {
        if (I.value != i) return;
        constexpr int Q = R / 4;
        v2f x[R];
        for (int p = 0; p < R; p++) x[p] = v2f{0.0f, 0.0f};
        for (int q = 0; q < 4; q++) x[I.value + q * Q] = v2f{in4[2 * q], in4[2 * q + 1]};
        if (middle) dit_tail_middle_r4<I.value, R, SIGN>(x); else dit_tail_r4<I.value, R, SIGN>(x);
        for (int q = 0; q < 4; q++) { out4[2 * q] = x[I.value + q * Q].x; out4[2 * q + 1] = x[I.value + q * Q].y; }
        done = 0;
    });
    return done;
}
// in: R complex points in NATURAL order; out: their unnormalised DFT of sign `sign` as the 16384-point real-gain kernel's
// register networks compute it: head groups, (R = 32: the middle stage,) radix-4 tail groups -- all R rows, or (middle)
// rows R/4 ... 3R/4 - 1 from the pruned groups
template <int R, int SIGN> static void host_dft_r4(int middle, const float *in, float *out)
{
    v2f x[R];
    for (int n = 0; n < R; n++) x[bitrev<R>(n)] = v2f{in[2 * n], in[2 * n + 1]};
    static_for<0, R / 4>([&](auto G) { dit_head4<G.value, R, SIGN>(x); });
    if constexpr (R == 32) dit_single<8, 32, SIGN>(x);
    if (middle) {
        static_for<0, R / 4>([&](auto I) { dit_tail_middle_r4<I.value, R, SIGN>(x); });
        for (int r = 0; r < R / 2; r++) { out[2 * r] = x[R / 4 + r].x; out[2 * r + 1] = x[R / 4 + r].y; }
    } else {
        static_for<0, R / 4>([&](auto I) { dit_tail_r4<I.value, R, SIGN>(x); });
        for (int r = 0; r < R; r++) { out[2 * r] = x[r].x; out[2 * r + 1] = x[r].y; }
    }
}

extern "C" {

int csdr__host_dit_tail_r4(int r, int sign, int i, int middle, const float *in4, float *out4)
{
    if (r == 16) return sign > 0 ? host_tail_r4<16, +1>(i, middle, in4, out4) : host_tail_r4<16, -1>(i, middle, in4, out4);
    if (r == 32) return sign > 0 ? host_tail_r4<32, +1>(i, middle, in4, out4) : host_tail_r4<32, -1>(i, middle, in4, out4);
    return -1;
}
int csdr__host_dft_r4(int r, int sign, int middle, const float *in, float *out)
{
    if (r == 16 && sign > 0) host_dft_r4<16, +1>(middle, in, out);
    else if (r == 16) host_dft_r4<16, -1>(middle, in, out);
    else if (r == 32 && sign > 0) host_dft_r4<32, +1>(middle, in, out);
    else if (r == 32) host_dft_r4<32, -1>(middle, in, out);
    else return -1;
    return 0;
}
// the factors of a unit twiddle the radix-4 groups are built from: e^{sign j 2 pi k/32} = j^rot m (1 + j tau)
int csdr__host_tw_factors(int k, int sign, double *m, double *tau)
{
    const TwFactors f = tw_factors(k, sign);
    *m = f.m; *tau = f.tau;
    return f.rot;
}
int csdr__host_fastfir2_radix4(void) { return fastfir2_radix4(); }
int csdr__host_fastfir2_pwres(void) { return fastfir2_pwres(); }
int csdr__host_fastfir2_hbm_knobs(void) { return fastfir2_hbm_knobs(); }
int csdr__host_fastfir2_gain_lds_bytes(void) { return fastfir2_gain_lds_bytes(); }

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
// the real gains of a design in natural order, P[k] = fastfir_gain(H[k], k), and the design itself
int csdr__host_fastfir_gains(int n, double flo, double fhi, double off, double fs, double *h_out, double *p_out)
{
    std::vector<cd> H;
    if (!fastfir_design(n, flo, fhi, off, fs, H)) return -1;
    memcpy(h_out, H.data(), sizeof(cd) * n);
    for (int k = 0; k < n; k++) p_out[k] = fastfir_gain(H[k], k);
    return 0;
}
int csdr__host_fastfir2_bin_of(int log2n, int t, int j, int e) { return fastfir2_bin_of(log2n, t, j, e); }
int csdr__host_fastfir2_gain_bin_of(int log2n, int t, int i, int c) { return fastfir2_gain_bin_of(log2n, t, i, c); }
// the same two orders composed with the rotation of the shared pass twiddles (fastfir2_twshare_shift): the slot -> bin maps the uploads
// are built from, the rotation alone, and the build flag
int csdr__host_fastfir2_slot_bin(int log2n, int t, int j, int e) { return fastfir2_slot_bin(log2n, t, j, e); }
int csdr__host_fastfir2_gain_slot_bin(int log2n, int t, int i, int c) { return fastfir2_gain_slot_bin(log2n, t, i, c); }
void csdr__host_fastfir2_twshare_shift(int log2n, int t, int *inner, int *outer) { fastfir2_twshare_shift(log2n, t, inner, outer); }
int csdr__host_fastfir2_twshare(void) { return fastfir2_twshare(); }

void csdr__host_dit_head4_gain(int sign, const float *x4, const float *g4, float *out4)
{
    if (sign > 0) host_head4_gain<+1>(x4, g4, out4); else host_head4_gain<-1>(x4, g4, out4);
}
int csdr__host_dft_middle(int r, int sign, const float *in, float *out)
{
    if (r == 16 && sign > 0) host_dft_middle<16, +1>(in, out);
    else if (r == 16) host_dft_middle<16, -1>(in, out);
    else if (r == 32 && sign > 0) host_dft_middle<32, +1>(in, out);
    else if (r == 32) host_dft_middle<32, -1>(in, out);
    else return -1;
    return 0;
}

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
// the row form's planner (display_rows_plan): states [nrows][4] = {skip, counter, gated, ready} in and out, ave [nrows];
// counts [nrows]; gath / load [nrows][6] = {row, nframes, ave, start, step, 0} with room for nrows entries;
// split6 = {ngath, nload, max_gath, max_load, max_count, next_pos}
void csdr__host_display_rows_plan(int *states4, const int *ave, int nrows, int pos, long long n, int N, int loaders,
                                  long long first_loaded, int sorted, int *counts, long long *gath6, long long *load6,
                                  int *split6)
{
    std::vector<DisplayState> rs((size_t)nrows), next((size_t)nrows);
    std::vector<SpecRow> g((size_t)nrows), l((size_t)nrows);
    for (int r = 0; r < nrows; r++) {
        rs[r].skip = states4[4 * r]; rs[r].counter = states4[4 * r + 1]; rs[r].gated = states4[4 * r + 2]; rs[r].ready = states4[4 * r + 3];
    }
    const DisplayRowsSplit d = display_rows_plan(rs.data(), ave, nrows, pos, n, N, loaders != 0, first_loaded, sorted != 0,
                                                 next.data(), counts, g.data(), l.data());
    for (int r = 0; r < nrows; r++) {
        states4[4 * r] = next[r].skip; states4[4 * r + 1] = next[r].counter; states4[4 * r + 2] = next[r].gated; states4[4 * r + 3] = next[r].ready;
    }
    auto put = [](long long *o, const SpecRow &e) { o[0] = e.row; o[1] = e.nframes; o[2] = e.ave_size; o[3] = e.start; o[4] = e.step; o[5] = 0; };
    for (int i = 0; i < d.ngath; i++) put(gath6 + 6 * i, g[i]);
    for (int i = 0; i < d.nload; i++) put(load6 + 6 * i, l[i]);
    split6[0] = d.ngath; split6[1] = d.nload; split6[2] = d.max_gath; split6[3] = d.max_load; split6[4] = d.max_count; split6[5] = d.next_pos;
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

// the batch scope's host-side pieces (scope_host.hpp), the same functions the kernel evaluates.
// The emissions of n samples from the state (inpos, pos) with pixel time pix at rate sr on a w-pixel screen:
// samples[e] = index within the call of the sample that emits e (the first max_out of them), end3 = {emissions,
// m_TimeScrnPos, m_TimeInPos} after the call; returns the emissions
long long csdr__host_scope_emissions(long long inpos, int pos, double pix, double sr, int w, long long n, long long max_out,
                                     long long *samples, long long *end3)
{
    const sc::Plan p = sc::make_plan(inpos, pos, pix, sr, w, n);
    for (long long e = 0; e < p.emits && e < max_out; e++) samples[e] = p.sample(e);
    end3[0] = p.emits; end3[1] = p.pos_end; end3[2] = p.inpos_end;
    return p.emits;
}
// m_TimeScrnPixel and m_DisplaySkipValue of a span (ms), display rate and sample rate on a w-pixel screen
void csdr__host_scope_settings(int span_ms, int display_rate, double sr, int w, double *pix, int *skip)
{
    *pix = sc::pixel_time(span_ms, w); *skip = sc::skip_value(span_ms, display_rate, sr);
}
// TRIG_OFF over m sweep starts: out3 = {displays, 1-based number of the last displaying start, counter afterwards}
void csdr__host_scope_free_run(long long cnt, int skip, long long m, long long *out3)
{
    const sc::FreeRun r = sc::free_run(cnt, skip, m);
    out3[0] = r.displays; out3[1] = r.last; out3[2] = r.cnt;
}
// One receiver of the batch scope on the CPU: the host's settings (sc::Chan, as capi_scope.hip keeps them) and the
// put with the functions the kernel calls (make_plan, searches, crossing, decide, screen_source) in the kernel's order
// of steps; the crossing search is a plain loop here.
struct HostScope {
    sc::Chan ch;
    sc::ChanState st;
    int w = 100, h = 100;
    int ring[2 * sc::kMaxW], screen[2 * sc::kMaxW];
};
void *csdr__host_scope_create(void)
{
    HostScope *s = new HostScope();
    memset(&s->st, 0, sizeof(s->st)); s->st.skipcounter = -2;
    memset(s->ring, 0, sizeof(s->ring)); memset(s->screen, 0, sizeof(s->screen));
    s->ch.derive(s->w);
    return s;
}
void csdr__host_scope_destroy(void *h) { delete (HostScope *)h; }
// what: 0 screen (v = w, v2 = h), 1 span, 2 display rate, 3 trigger mode, 4 level, 5 vertical range, 6 reset, 7 time_plot_done,
// 8 OnTimeDisplay(v), 9 OnEnablePeak(v)
void csdr__host_scope_slot(void *h, int what, int v, int v2)
{
    HostScope &s = *(HostScope *)h;
    switch (what) {
    case 0: s.w = v; s.h = v2; s.ch.reset(v); break;
    case 1: s.ch.on_horz_span(v, s.w); break;
    case 2: s.ch.on_display_rate(v); break;
    case 3: s.ch.on_trigger_mode(v, s.w); break;
    case 4: s.ch.level = v; break;
    case 5: s.ch.vert = v; break;
    case 6: s.ch.reset(s.w); break;
    case 8: s.ch.on_time_display(v, s.w); break;        // OnTimeDisplay(v != 0)
    case 9: s.ch.on_enable_peak(v); break;
    default: s.ch.time_plot_done(); break;
    }
}
// DisplayData of n samples (im NULL: the real form); returns the emits so far
long long csdr__host_scope_put(void *h, const float *re, const float *im, int n, double fs)
{
    HostScope &s = *(HostScope *)h;
    sc::ChanParam par;
    s.ch.prepare(n, fs, s.w, par, s.h, im != nullptr);
    sc::ChanState &st = s.st;
    int *ring = s.ring, *screen = s.screen;
    const int w = s.w;
    if (par.flags & (sc::F_RESET | sc::F_PEAK)) memset(ring, 0, sizeof(s.ring));     // Reset :555-560, OnEnablePeak :336-341
    sc::apply_flags(st, par.flags);
    if (par.view == sc::VIEW_FFT) {                      // the frames are the device's; the counters as the kernel sets them
        if (par.n > 0) { st.skipcounter = par.cnt_end; st.emits += (unsigned)par.count; }
        return st.emits;
    }
    if (par.n > 0) {
        const sc::Plan pl = sc::make_plan(st.inpos, st.pos, par.pix, par.sr, w, par.n);
        const long long E = pl.emits;
        const int pos0 = st.pos;
        auto get = [&](long long e, int &a, int &b) { const long long k = pl.sample(e); a = sc::sat_int(re[k]); b = im ? sc::sat_int(im[k]) : 0; };
        long long trig = -1;
        if (sc::searches(st, par))
            for (long long e = 0; e < E && trig < 0; e++) {
                int cur, prv, t;
                get(e, cur, t);
                if (e == 0) prv = st.prev; else get(e - 1, prv, t);
                if (sc::crossing(par.mode, par.level, cur, prv)) trig = e;
            }
        const sc::Display d = sc::decide(st, par, w, E, trig);
        if (d.at >= 0)
            for (int i = 0; i < w; i++) {
                int a, b, slot = 0;
                const long long e = sc::screen_source(d, i, w, pos0, &slot);
                if (e >= 0) get(e, a, b); else { a = ring[slot]; b = ring[sc::kMaxW + slot]; }
                screen[i] = a; screen[sc::kMaxW + i] = b;
            }
        for (long long e = E > w ? E - w : 0; e < E; e++) {
            int a, b;
            get(e, a, b);
            const int slot = (int)((pos0 + e) % w);
            ring[slot] = a; ring[sc::kMaxW + slot] = b;
        }
        int t;
        if (E > 0) get(E - 1, st.prev, t);
        st.inpos = pl.inpos_end; st.pos = pl.pos_end;
    }
    return st.emits;
}
// state7 as the first seven of csdr_scope_batch_get_state; screen_re / screen_im [w]
void csdr__host_scope_get(void *h, long long *state7, int *screen_re, int *screen_im)
{
    HostScope &s = *(HostScope *)h;
    const sc::ChanState &st = s.st;
    state7[0] = st.inpos; state7[1] = st.pos; state7[2] = st.prev; state7[3] = st.trigstate; state7[4] = st.trigcounter;
    state7[5] = st.trigbufpos; state7[6] = st.skipcounter;
    memcpy(screen_re, s.screen, sizeof(int) * s.w); memcpy(screen_im, s.screen + sc::kMaxW, sizeof(int) * s.w);
}
int csdr__host_scope_sat_int(double x) { return sc::sat_int(x); }

// ---- the FFT view's host-side pieces (scope_host.hpp)
// the used frames of n samples entered at m_FftBufPos = pos with the skip counter at cnt: out6 = {frames that complete,
// first used one, step, count, m_FftBufPos afterwards, skip counter afterwards}
void csdr__host_scope_fft_plan(int pos, long long cnt, int skip, long long n, long long *out6)
{
    const sc::FftPlan p = sc::fft_plan(pos, cnt, skip, n);
    out6[0] = p.frames; out6[1] = p.first; out6[2] = p.step; out6[3] = p.count; out6[4] = p.pos_end; out6[5] = p.cnt_end;
}
// m_DisplaySkipValue and m_Span of the FFT view at a display rate and sample rate
void csdr__host_scope_fft_settings(int display_rate, double sr, int *skip, int *span)
{
    *skip = sc::fft_skip_value(display_rate, sr); *span = sc::fft_span(sr);
}
// what one receiver's settings hold: out8 = {view, skip value, m_Span, m_FftBufPos, skip counter, carry buffer, pending
// flags, m_PeakOn}
void csdr__host_scope_fft_chan(void *h, long long *out8)
{
    const sc::Chan &k = ((HostScope *)h)->ch;
    out8[0] = k.view; out8[1] = k.skip; out8[2] = k.fspan; out8[3] = k.fpos; out8[4] = k.fcnt; out8[5] = k.fcur;
    out8[6] = k.flags; out8[7] = k.peak_on;
}
// completing frame j of a call entered with `fill` carried samples, as scope_fft_kernel loads it: carry [fill] and row
// [n] complex fp32 (interleaved; cpx == 0: row is real fp32 and goes in as (x, 0)) -> out [2048] complex fp32
void csdr__host_scope_fft_frame(const float *carry, int fill, const float *row, int cpx, long long j, float *out)
{
    for (int i = 0; i < sc::kFftN; i++) {
        const long long s = sc::fft_source(j, i, fill);
        if (s < 0) { out[2 * i] = carry[2 * (s + fill)]; out[2 * i + 1] = carry[2 * (s + fill) + 1]; }
        else if (cpx) { out[2 * i] = row[2 * s]; out[2 * i + 1] = row[2 * s + 1]; }
        else { out[2 * i] = row[s]; out[2 * i + 1] = 0.f; }
    }
}
// DrawFftPlot's GetScreenIntegerFFTData of bels[2048] (display order) for a receiver whose last Reset saw the rate fs
// and left m_Span = span: out [w] pixels, map4 = {m_BinMin, m_BinMax, the "more bins than pixels" branch, h}
void csdr__host_scope_fft_map(int span, int cpx, double fs, int w, int h, const double *bels, int *out, int *map4)
{
    const sc::FftMap m = sc::make_fft_map(span, cpx, fs, w, h);
    for (int x = 0; x < w; x++) out[x] = sc::fft_pixel(m, w, x, [&](int i) { return bels[i]; });
    map4[0] = m.bin_min; map4[1] = m.bin_max; map4[2] = m.bins; map4[3] = m.h;
}

// ---- the batch plotter's host-side pieces (plotter_host.hpp), the same functions the draw kernel evaluates
// one GetScreenIntegerFFTData of draw() as the kernel computes it: per pixel the largest bel of its run (the smallest
// when max_db < min_db), then the level.
// ave [n] bels in display order -> out [w]; map4 = {m_BinMin, m_BinMax, the "more bins than pixels" branch, lanes per pixel}
void csdr__host_plotter_map(int n, int invert, double fs, int span, int w, int h, int max_db, int min_db, const float *ave,
                            int *out, int *map4)
{
    const pl::Map m = pl::make_map(n, fs, span, w);
    const double gain = pl::db_gain(max_db, min_db), off = pl::db_off(max_db);
    for (int x = 0; x < w; x++) {
        int lo, hi;
        pl::pixel_bins(m, n, invert, w, x, &lo, &hi);
        const int smallest = pl::run_keeps_smallest(max_db, min_db);
        float top = pl::run_start(smallest);
        for (int i = lo; i <= hi; i++) top = pl::run_keep(top, ave[i], smallest);
        out[x] = pl::level(h, gain, off, top);
    }
    if (map4) { map4[0] = m.bin_min; map4[1] = m.bin_max; map4[2] = m.bins; map4[3] = pl::group_lanes(m, w); }
}
// a sequence of slot calls on a new view: calls [ncalls][3] = {what, a, b}, what: 0 resizeEvent(a, b), 1
// SetPercent2DScreen(a), 2 SetSpanFreq(a), 3 SetMaxdB(a), 4 SetdBStepSize(a), 5 UpdateOverlay, 6 one draw's scroll ->
// out8 = {w, h2d, wf_h, m_MindB, m_MaxdB, m_Span, ring head, lines drawn}
void csdr__host_plotter_view(const int *calls, int ncalls, int *out8)
{
    pl::View k;
    for (int c = 0; c < ncalls; c++) {
        const int a = calls[3 * c + 1], b = calls[3 * c + 2];
        switch (calls[3 * c]) {
        case 0: k.resize(a, b); break;
        case 1: k.set_percent(a); break;
        case 2: k.span = a; break;
        case 3: k.max_db = a; break;
        case 4: k.step = a; break;
        case 5: k.update_overlay(); break;
        default: k.scroll(); break;
        }
    }
    out8[0] = k.w; out8[1] = k.h2d; out8[2] = k.wf_h; out8[3] = k.min_db; out8[4] = k.max_db; out8[5] = k.span;
    out8[6] = k.head; out8[7] = k.filled;
}
// the pen of one draw: state2 = {m_ADOverLoad, m_ADOverloadOneShotCounter}, updated; returns 1 for red
int csdr__host_plotter_pen(int *state2, int fft_overload) { return pl::pen_step(&state2[0], &state2[1], fft_overload); }

// ---- the datagram sequence check's sequential form (seq_host.hpp: seq_walk over seq_step, the function K12 evaluates):
// npackets datagrams of pkt_len bytes in host memory, one receiver; *last, *missed, *events carried in and out,
// *first_gap this walk's
void csdr__host_seq_walk(const void *packets, int npackets, int pkt_len, int *last, long long *missed, long long *events, int *first_gap)
{
    seq::State s{*missed, *events, *last, -1};
    seq::seq_walk((const unsigned char *)packets, npackets, pkt_len, &s);
    *last = s.last; *missed = s.missed; *events = s.events; *first_gap = s.first_gap;
}

// ---- the NCO-spur bookkeeping (spurcal_host.hpp: the functions K13 evaluates)
// a put of n samples in calls of call_len on a receiver with (count, active): out4 = {calls that run the recurrence,
// samples they cover, count after, active after}
void csdr__host_spurcal_put(int count, int active, int n, int call_len, int *out4)
{
    const spur::Put p = spur::spurcal_put(count, active, n, call_len);
    out4[0] = p.calls; out4[1] = p.samples; out4[2] = p.count; out4[3] = p.active;
}
// ManageNCOSpurOffsets on one receiver: cmd 0 SET(vi, vq), 1 STARTCAL, 2 READ; off2, *count, *active updated
void csdr__host_spurcal_command(int cmd, double vi, double vq, double *off2, int *count, int *active)
{
    spur::Rec r{*count, *active};
    spur::spurcal_command(cmd, vi, vq, off2, &r);
    *count = r.count; *active = r.active;
}

// ---- the noise blanker's host logic (nb_host.hpp)
// samples per tile the segments of a call are cut by (mask form or sample form), and the ring's window limits
void csdr__host_nb_geometry(int mask, int *seg_tile, int *ring_min, int *ring_max)
{
    *seg_tile = nb_seg_tile(mask != 0); *ring_min = nb_ring_min(mask != 0); *ring_max = nb_ring_max(mask != 0);
}
void csdr__host_nb_segments(long long n, int channels, int mask, int ring, int *nseg, int *seg_len)
{
    const NbSegments s = nb_segments((long)n, channels, mask != 0, ring != 0);
    *nseg = s.nseg; *seg_len = s.seg_len;
}
// the kernel form (NbForm) of a call: mask or samples out, pkt_len 0 for float rows; per channel on, mag_n, integral
int csdr__host_nb_form(int mask, int pkt_len, int channels, const int *on, const int *mag_n, const int *integral,
                       int ring_switch, int int_switch)
{
    std::vector<NbHost> h(channels);
    for (int c = 0; c < channels; c++) { h[c].on = on[c] != 0; h[c].mag_n = mag_n[c]; h[c].integral = integral[c] != 0; }
    return (int)nb_choose_form(mask != 0, pkt_len, h.data(), channels, ring_switch != 0, int_switch != 0);
}

}  // extern "C"
