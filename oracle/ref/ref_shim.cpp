// ref_shim.cpp -- TEST INFRASTRUCTURE.  extern "C" entry points onto the reference's own dsp/ classes, one ref_* per
// orc_* of oracle/cutesdr_oracle.h with the same arguments, so that oracle/ref.py can stand where oracle/oracle.py stands.
// Every function only constructs, calls or reads a reference object; none restates what the reference computes.
//
// This translation unit alone is compiled with -fno-access-control: the tests read CFft::m_pFFTAveBuf,
// CFastFIR::m_pFilterCoef, CFir's taps, CIir's coefficients, CFmDemod::m_SquelchState, CDownConvert's stage list and NCO
// frequency and CDemodulator::m_InBufLimit / m_InBufPos.
//
// Zeroed construction: several reference constructors leave members unset (CDemodulator: m_pFmDemod, m_InputRate,
// m_CW_Offset, m_AGC*; CDownConvert: m_OutputRate, m_OscCos, m_OscSin; CFastFIR: all of m_pFFTOverlapBuf but its first
// entry; CFmDemod: m_SquelchThreshold; CFir / CIir: delay lines and coefficients; CAgc, CSMeter, CNoiseProc: everything
// SetParameters / SetupBlanker compares with first; CFractResampler: m_pSinc, m_pInputBuf, m_FloatTime before Init).
// Objects are therefore placement-constructed into calloc'ed storage, and operator new of this library (bound with
// -Bsymbolic, not exported) hands out zeroed storage too, which covers the objects and buffers the reference allocates
// itself.  Every such member then reads as zero, which is the oracle's initial state as well.
#include <new>
#include <stdlib.h>
#include <string.h>
#include <typeinfo>
#include "dsp/demodulator.h"
#include "dsp/fractresampler.h"
#include "dsp/noiseproc.h"
#include "dsp/iir.h"
#include "dsp/filtercoef.h"
#include "gui/testbench.h"

void *operator new(size_t n) { void *p = calloc(1, n ? n : 1); if (!p) throw std::bad_alloc(); return p; }
void *operator new[](size_t n) { void *p = calloc(1, n ? n : 1); if (!p) throw std::bad_alloc(); return p; }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

template <class T> static T *make() { return new (calloc(1, sizeof(T))) T(); }
template <class T> static T *make(double a) { return new (calloc(1, sizeof(T))) T(a); }
template <class T> static void drop(T *p) { if (p) { p->~T(); free(p); } }

typedef TYPECPX cpx;

extern "C" {

/* ---- limits of the reference's fixed buffers, for the binding's refusals ---- */
int ref_limit(int which)
{
    switch (which) {
    case 0: return 32768;            /* dsp/downconvert.cpp MAX_HALF_BAND_BUFSIZE (file-local there) */
    case 1: return MAX_INBUFSIZE;
    case 2: return MAX_MAGBUFSIZE;
    case 3: return MAX_SQBUF_SIZE;
    case 4: return 4096;             /* dsp/noiseproc.cpp: m_TestBenchDataBuf, one entry per sample of a call */
    case 5: return 32768;            /* dsp/noiseproc.cpp MAX_AVE */
    case 6: return MAX_FFT_SIZE;
    case 7: return MIN_FFT_SIZE;
    case 8: return MAX_NUMCOEF;
    case 9: return 2048;             /* dsp/fastfir.cpp CONV_FFT_SIZE (file-local there) */
    }
    return -1;
}

/* the two numbers that end SetDataRate's loop (downconvert.cpp:127), for the binding's count of the stages a call would build */
double ref_dc_loop_const(int which) { return which == 0 ? HB51TAP_MAX : 7900.0 * 2.0 /* MIN_OUTPUT_RATE, file-local there */; }

/* ---- the recorded PROFILE_* calls (one global test bench, as in the application) ---- */
int ref_tap_calls(void) { return (int)g_pTestBench->calls.size(); }
void ref_tap_call(int i, int *profile, int *n, int *is_cpx, double *rate, double *first)
{
    const CTestBench::Call &c = g_pTestBench->calls[i];
    *profile = c.profile; *n = c.n; *is_cpx = c.cpx; *rate = c.rate; *first = c.first;
}
void ref_tap_calls_clear(void) { g_pTestBench->calls.clear(); }

/* ---- CFft ---- */
CFft *ref_cfft_new(void) { return make<CFft>(); }
void ref_cfft_free(CFft *f) { drop(f); }
void ref_cfft_set_params(CFft *f, int size, int invert, double db_comp, double fs) { f->SetFFTParams(size, invert != 0, db_comp, fs); }
void ref_cfft_set_ave(CFft *f, int ave) { f->SetFFTAve(ave); }
void ref_cfft_reset(CFft *f) { f->ResetFFT(); }
int ref_cfft_put_display(CFft *f, int n, cpx *in) { return f->PutInDisplayFFT(n, in); }
int ref_cfft_get_screen(CFft *f, int max_h, int max_w, double max_db, double min_db, int start_hz, int stop_hz, int *out)
{ return f->GetScreenIntegerFFTData(max_h, max_w, max_db, min_db, start_hz, stop_hz, out) ? 1 : 0; }
void ref_cfft_fwd(CFft *f, cpx *a) { f->FwdFFT(a); }
void ref_cfft_rev(CFft *f, cpx *a) { f->RevFFT(a); }
int ref_cfft_size(const CFft *f) { return f->m_FFTSize; }
const double *ref_cfft_avebuf(const CFft *f) { return f->m_pFFTAveBuf; }

/* ---- CFastFIR (2048 points only: CONV_FFT_SIZE is fixed in the reference) ---- */
CFastFIR *ref_fastfir_new(int fft_size) { return fft_size == 2048 ? make<CFastFIR>() : 0; }
void ref_fastfir_free(CFastFIR *f) { drop(f); }
int ref_fastfir_setup(CFastFIR *f, double flo, double fhi, double offset, double fs) { f->SetupParameters(flo, fhi, offset, fs); return 0; }
int ref_fastfir_process(CFastFIR *f, int n, cpx *in, cpx *out) { return f->ProcessData(n, in, out); }
const cpx *ref_fastfir_coef(const CFastFIR *f) { return f->m_pFilterCoef; }

/* ---- CDownConvert ---- */
CDownConvert *ref_downconv_new(void) { return make<CDownConvert>(); }
void ref_downconv_free(CDownConvert *d) { drop(d); }
void ref_downconv_set_cw_offset(CDownConvert *d, double off) { d->SetCwOffset(off); }
void ref_downconv_set_frequency(CDownConvert *d, double f) { d->SetFrequency(f); }
double ref_downconv_set_data_rate(CDownConvert *d, double in_rate, double max_bw) { return d->SetDataRate(in_rate, max_bw); }
int ref_downconv_process(CDownConvert *d, int n, cpx *in, cpx *out) { return d->ProcessData(n, in, out); }
int ref_downconv_stages(const CDownConvert *d, int *codes)        /* 3 = CIC3, else the half band's length */
{
    int n = 0;
    for (; n < MAX_DECSTAGES && d->m_pDecimatorPtrs[n]; n++) {
        CDownConvert::CDec2 *s = d->m_pDecimatorPtrs[n];
        if (typeid(*s) == typeid(CDownConvert::CCicN3DecimateBy2)) codes[n] = 3;
        else if (typeid(*s) == typeid(CDownConvert::CHalfBand11TapDecimateBy2)) codes[n] = 11;
        else codes[n] = static_cast<CDownConvert::CHalfBandDecimateBy2 *>(s)->m_FirLength;
    }
    return n;
}
double ref_downconv_nco_freq(const CDownConvert *d) { return d->m_NcoFreq; }

/* ---- CFir ---- */
CFir *ref_fir_new(void) { return make<CFir>(); }
void ref_fir_free(CFir *f) { drop(f); }
void ref_fir_init_const(CFir *f, int ntaps, const double *coef) { f->InitConstFir(ntaps, coef); }
int ref_fir_init_lp(CFir *f, double scale, double astop, double fpass, double fstop, double fs) { return f->InitLPFilter(scale, astop, fpass, fstop, fs); }
int ref_fir_init_hp(CFir *f, double scale, double astop, double fpass, double fstop, double fs) { return f->InitHPFilter(scale, astop, fpass, fstop, fs); }
void ref_fir_gen_hilbert(CFir *f, double off) { f->GenerateHBFilter(off); }
void ref_fir_process_real(CFir *f, int n, double *in, double *out) { f->ProcessFilter(n, in, out); }
void ref_fir_process_cpx(CFir *f, int n, cpx *in, cpx *out) { f->ProcessFilter(n, in, out); }
int ref_fir_taps(const CFir *f, double *coef, double *icoef, double *qcoef)
{
    memcpy(coef, f->m_Coef, sizeof(double) * f->m_NumTaps);
    memcpy(icoef, f->m_ICoef, sizeof(double) * f->m_NumTaps);
    memcpy(qcoef, f->m_QCoef, sizeof(double) * f->m_NumTaps);
    return f->m_NumTaps;
}

/* ---- CIir ---- */
CIir *ref_iir_new(void) { return make<CIir>(); }
void ref_iir_free(CIir *f) { drop(f); }
void ref_iir_init(CIir *f, int kind, double f0, double q, double fs)
{
    switch (kind) {
    case 0: f->InitLP(f0, q, fs); break;
    case 1: f->InitHP(f0, q, fs); break;
    case 2: f->InitBP(f0, q, fs); break;
    default: f->InitBR(f0, q, fs); break;
    }
}
void ref_iir_process_real(CIir *f, int n, double *in, double *out) { f->ProcessFilter(n, in, out); }
void ref_iir_process_cpx(CIir *f, int n, cpx *in, cpx *out) { f->ProcessFilter(n, in, out); }
void ref_iir_coefs(const CIir *f, double *c) { c[0] = f->m_B0; c[1] = f->m_B1; c[2] = f->m_B2; c[3] = f->m_A1; c[4] = f->m_A2; }

/* ---- CAgc, CSMeter ---- */
CAgc *ref_agc_new(void) { return make<CAgc>(); }
void ref_agc_free(CAgc *a) { drop(a); }
void ref_agc_set(CAgc *a, int on, int hang, int thresh, int manual_gain, int slope, int decay, double fs)
{ a->SetParameters(on != 0, hang != 0, thresh, manual_gain, slope, decay, fs); }
void ref_agc_process_cpx(CAgc *a, int n, cpx *in, cpx *out) { a->ProcessData(n, in, out); }
void ref_agc_process_real(CAgc *a, int n, double *in, double *out) { a->ProcessData(n, in, out); }

CSMeter *ref_smeter_new(void) { return make<CSMeter>(); }
void ref_smeter_free(CSMeter *s) { drop(s); }
void ref_smeter_process(CSMeter *s, int n, cpx *in, double fs) { s->ProcessData(n, in, fs); }
double ref_smeter_peak(CSMeter *s) { return s->GetPeak(); }
double ref_smeter_ave(CSMeter *s) { return s->GetAve(); }

/* ---- demodulators ---- */
CAmDemod *ref_amdemod_new(double fs) { return make<CAmDemod>(fs); }
void ref_amdemod_free(CAmDemod *d) { drop(d); }
void ref_amdemod_set_bandwidth(CAmDemod *d, double bw) { d->SetBandwidth(bw); }
int ref_amdemod_process_mono(CAmDemod *d, int n, cpx *in, double *out) { return d->ProcessData(n, in, out); }
int ref_amdemod_process_stereo(CAmDemod *d, int n, cpx *in, cpx *out) { return d->ProcessData(n, in, out); }

CSamDemod *ref_samdemod_new(double fs) { return make<CSamDemod>(fs); }
void ref_samdemod_free(CSamDemod *d) { drop(d); }
int ref_samdemod_process_mono(CSamDemod *d, int n, cpx *in, double *out) { return d->ProcessData(n, in, out); }
int ref_samdemod_process_stereo(CSamDemod *d, int n, cpx *in, cpx *out) { return d->ProcessData(n, in, out); }

CFmDemod *ref_fmdemod_new(double fs) { return make<CFmDemod>(fs); }
void ref_fmdemod_free(CFmDemod *d) { drop(d); }
void ref_fmdemod_set_squelch(CFmDemod *d, int v) { d->SetSquelch(v); }
int ref_fmdemod_process_mono(CFmDemod *d, int n, double fm_bw, cpx *in, double *out) { return d->ProcessData(n, fm_bw, in, out); }
int ref_fmdemod_process_stereo(CFmDemod *d, int n, double fm_bw, cpx *in, cpx *out) { return d->ProcessData(n, fm_bw, in, out); }
int ref_fmdemod_squelched(const CFmDemod *d) { return d->m_SquelchState ? 1 : 0; }

int ref_ssbdemod_process_mono(int n, cpx *in, double *out) { CSsbDemod d; return d.ProcessData(n, in, out); }
int ref_ssbdemod_process_stereo(int n, cpx *in, cpx *out) { CSsbDemod d; return d.ProcessData(n, in, out); }

/* ---- CFractResampler ---- */
CFractResampler *ref_resampler_new(void) { return make<CFractResampler>(); }
void ref_resampler_free(CFractResampler *r) { drop(r); }
void ref_resampler_init(CFractResampler *r, int max_input) { r->Init(max_input); }
int ref_resampler_real(CFractResampler *r, int n, double rate, double *in, double *out) { return r->Resample(n, rate, in, out); }
int ref_resampler_cpx(CFractResampler *r, int n, double rate, cpx *in, cpx *out) { return r->Resample(n, rate, in, out); }
int ref_resampler_real_i16(CFractResampler *r, int n, double rate, double *in, short *out, double gain)
{ return r->Resample(n, rate, in, (TYPEMONO16 *)out, gain); }
int ref_resampler_cpx_i16(CFractResampler *r, int n, double rate, cpx *in, short *out, double gain)
{ return r->Resample(n, rate, in, (TYPESTEREO16 *)out, gain); }

/* ---- CNoiseProc ---- */
CNoiseProc *ref_noiseproc_new(void) { return make<CNoiseProc>(); }
void ref_noiseproc_free(CNoiseProc *p) { drop(p); }
int ref_noiseproc_setup(CNoiseProc *p, int on, double thresh, double width, double fs) { p->SetupBlanker(on != 0, thresh, width, fs); return 0; }
void ref_noiseproc_process(CNoiseProc *p, int n, cpx *in, cpx *out) { p->ProcessBlanker(n, in, out); }

/* ---- CDemodulator ---- */
typedef struct {
    int HiCut, HiCutmin, HiCutmax, LowCut, LowCutmin, LowCutmax;
    int FilterClickResolution, Offset, SquelchValue;
    int AgcSlope, AgcThresh, AgcManualGain, AgcDecay;
    int AgcOn, AgcHangOn, Symetric;
} ref_demod_info;                       /* the POD mirror of tDemodInfo that oracle/cutesdr_oracle.h uses */

CDemodulator *ref_demod_new(int fastfir_n) { return fastfir_n == 2048 ? make<CDemodulator>() : 0; }
void ref_demod_free(CDemodulator *d) { drop(d); }
void ref_demod_set_input_rate(CDemodulator *d, double rate) { d->SetInputSampleRate(rate); }
void ref_demod_set_demod(CDemodulator *d, int mode, const ref_demod_info *i)
{
    tDemodInfo t;
    t.HiCut = i->HiCut; t.HiCutmin = i->HiCutmin; t.HiCutmax = i->HiCutmax;
    t.LowCut = i->LowCut; t.LowCutmin = i->LowCutmin; t.LowCutmax = i->LowCutmax;
    t.FilterClickResolution = i->FilterClickResolution; t.Offset = i->Offset; t.SquelchValue = i->SquelchValue;
    t.AgcSlope = i->AgcSlope; t.AgcThresh = i->AgcThresh; t.AgcManualGain = i->AgcManualGain; t.AgcDecay = i->AgcDecay;
    t.AgcOn = i->AgcOn != 0; t.AgcHangOn = i->AgcHangOn != 0; t.Symetric = i->Symetric != 0;
    d->SetDemod(mode, t);
}
void ref_demod_set_freq(CDemodulator *d, double f) { d->SetDemodFreq(f); }
double ref_demod_output_rate(CDemodulator *d) { return d->GetOutputRate(); }
double ref_demod_smeter_peak(CDemodulator *d) { return d->GetSMeterPeak(); }
double ref_demod_smeter_ave(CDemodulator *d) { return d->GetSMeterAve(); }
int ref_demod_buf_limit(const CDemodulator *d) { return d->m_InBufLimit; }
int ref_demod_buf_pos(const CDemodulator *d) { return d->m_InBufPos; }
double ref_demod_input_rate(const CDemodulator *d) { return d->m_InputRate; }
double ref_demod_max_bw(const CDemodulator *d) { return d->m_DesiredMaxOutputBandwidth; }
int ref_demod_stages(const CDemodulator *d, int *codes) { return ref_downconv_stages(&d->m_DownConvert, codes); }
double ref_demod_nco_freq(const CDemodulator *d) { return d->m_DownConvert.m_NcoFreq; }
int ref_demod_process_mono(CDemodulator *d, int n, cpx *in, double *out) { return d->ProcessData(n, in, out); }
int ref_demod_process_stereo(CDemodulator *d, int n, cpx *in, cpx *out) { return d->ProcessData(n, in, out); }
/* the append form of the batch harness: the input is handed over in pieces that each end where the reference's input
 * window fills, so that every ProcessData call runs at most one pass and its audio can be put behind the last one's */
int ref_demod_process_mono_append(CDemodulator *d, int n, cpx *in, double *out)
{
    int done = 0, total = 0;
    while (done < n) {
        int room = d->m_InBufLimit - d->m_InBufPos;
        int take = room < 1 ? 1 : room;
        if (take > n - done) take = n - done;
        total += d->ProcessData(take, in + done, out + total);
        done += take;
    }
    return total;
}

}
