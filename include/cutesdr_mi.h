/*
 * cutesdr_mi.h -- C ABI of libcutesdr_mi.so, the MI355X (gfx950) implementation of the
 * CuteSDR dsp/ receive chain.
 *
 * The reference has no plugin/FFI layer: its host code instantiates the dsp/
 * classes by value and calls their public methods.  The drop-in boundary is therefore this C
 * ABI plus the same-named C++ classes in cutesdr_amd/dropin/dsp/ that forward to it.  Each
 * entry point cites the reference method it stands in for (file:line in the reference tree).
 *
 * Conventions
 *  - opaque handles, plain pointers and sizes, no C++ or torch types;
 *  - "host" entry points take interleaved double I/Q (TYPECPX = {double re, im},
 *    dsp/datatypes.h:24-41) exactly like the reference methods, may run in place, return the
 *    number of samples produced (>= 0) or a negative CSDR_E* code (a new failure class the
 *    reference does not have: HIP errors, bad handles);
 *  - "batch" entry points are the multi-channel extension: device-resident interleaved fp32
 *    I/Q, channel-major [channels][stride], no host copies, launched on the caller's stream;
 *  - the library never falls back to a CPU path: without a usable GPU every create() fails;
 *  - batch process calls only enqueue work on `stream` (NULL = the default stream) and return; the
 *    caller synchronises.  Setters, getters and the host entry points synchronise the device;
 *  - threading: a handle is not locked internally -- ONE thread at a time per handle, setters and getters
 *    included.  A setter uploads parameters or state with device copies and a getter may read and reset
 *    device state (csdr_*_get_smeter_peak); issued while a process call of the same handle is running on
 *    another thread they would race with it.  The drop-in C++ classes (cutesdr_amd/dropin/dsp/) provide the
 *    guarantee the reference's QMutex members give its host: every method that reaches this ABI holds the
 *    object's lock, so GUI-thread setters and the IQ thread's ProcessData serialise per object.  Different
 *    handles are independent and may be used from different threads at the same time.
 */
#ifndef CUTESDR_MI_H
#define CUTESDR_MI_H

#ifdef __cplusplus
extern "C" {
#endif

#define CSDR_OK 0
#define CSDR_EINVAL (-1)      /* bad argument / handle */
#define CSDR_EHIP (-2)        /* HIP runtime error, see csdr_last_error() */
#define CSDR_ENOMEM (-3)
#define CSDR_ESTATE (-4)      /* call order / configuration error */

int csdr_version(void);
const char *csdr_last_error(void);          /* thread-local, never NULL */
int csdr_device_count(void);                /* 0 when no GPU is visible */

/* device memory helpers for callers without their own allocator (tests, C hosts) */
void *csdr_dev_alloc(int device, unsigned long long bytes);
int csdr_dev_free(int device, void *p);
int csdr_dev_upload(int device, void *dst, const void *src, unsigned long long bytes);
int csdr_dev_download(int device, void *dst, const void *src, unsigned long long bytes);
int csdr_dev_sync(int device);

/* ----------------------------------------------------------------------------------------
 * CFastFIR -- overlap-save FFT band-pass (dsp/fastfir.h:17-44, dsp/fastfir.cpp).
 * fft_size in {2048, 4096, 8192, 16384}; taps = fft_size/2+1, hop = fft_size/2
 * (2048 is the reference's compiled-in size, fastfir.cpp:55-56).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_fastfir csdr_fastfir;

/* CFastFIR::CFastFIR (fastfir.cpp:67-130) */
csdr_fastfir *csdr_fastfir_create(int device, int fft_size);
void csdr_fastfir_destroy(csdr_fastfir *f);
/* CFastFIR::SetupParameters (fastfir.cpp:178-259).  Returns 1 = new filter designed,
 * 0 = unchanged, CSDR_EINVAL = rejected by the reference's sanity check (old taps kept). */
int csdr_fastfir_setup(csdr_fastfir *f, double flo, double fhi, double offset, double fs);
/* CFastFIR::ProcessData (fastfir.cpp:268-306).  in/out: n interleaved double pairs; out needs
 * room for n + fft_size/2 samples; in == out allowed.  Returns samples written. */
int csdr_fastfir_process(csdr_fastfir *f, int n, const double *in_iq, double *out_iq);

/* batched, device-resident form of the same filter */
typedef struct csdr_fastfir_batch csdr_fastfir_batch;
csdr_fastfir_batch *csdr_fastfir_batch_create(int device, int channels, int fft_size);
void csdr_fastfir_batch_destroy(csdr_fastfir_batch *b);
/* channel = -1: one filter shared by every channel; otherwise that channel's own filter */
int csdr_fastfir_batch_setup(csdr_fastfir_batch *b, int channel, double flo, double fhi,
                             double offset, double fs);
/* The same for n filters in one call, designed ON THE DEVICE (fp64, one workgroup per filter): per entry the host does
 * the reference's sanity check and queues a job of two doubles; the next csdr_fastfir_batch_process launches all queued
 * jobs on its stream right behind its patch kernel -- behind everything in flight on that stream, in front of the filter
 * launch, nobody else waited for.  Entries apply in array order: a later entry for a channel replaces an earlier one, a
 * later csdr_fastfir_batch_setup of that channel cancels its queued job, a job queued after a csdr_fastfir_batch_setup of
 * the channel wins.  channel[i] = -1: the shared filter (early-out as above) or, on a per-channel object, every channel;
 * the first entry that names a channel turns a shared-filter object per-channel (that one step waits for the device).
 * status[i]: 1 designed, 0 unchanged, CSDR_EINVAL rejected by the sanity check (old taps kept, the other entries still
 * apply).  Returns CSDR_OK or the first hard error; bad arguments (null arrays, n < 0, a channel out of range) return
 * CSDR_EINVAL and change nothing.  csdr_fastfir_batch_get_response of such a channel waits for the object's stream. */
int csdr_fastfir_batch_setup_many(csdr_fastfir_batch *b, int n, const int *channel, const double *flo, const double *fhi,
                                  const double *offset, const double *fs, int *status);
/* clears the overlap history (as a freshly constructed CFastFIR) */
int csdr_fastfir_batch_reset(csdr_fastfir_batch *b);
/* d_in/d_out: device pointers, interleaved fp32 I/Q, [channels][stride] (strides in complex
 * samples).  n_per_channel must be a positive multiple of fft_size/2; produces exactly
 * n_per_channel samples per channel (first call: the stream delayed behind fft_size/2 zeros,
 * as the reference's zero-initialised overlap does).  stream: hipStream_t or NULL.
 * blocks_per_wg <= 0 picks a default.  Asynchronous; returns CSDR_OK or an error. */
int csdr_fastfir_batch_process(csdr_fastfir_batch *b, const float *d_in, long long in_stride,
                               int n_per_channel, float *d_out, long long out_stride,
                               void *stream, int blocks_per_wg);
/* copy of the designed frequency response H[k] (natural order, fp64 pairs) for tests */
int csdr_fastfir_batch_get_response(csdr_fastfir_batch *b, int channel, double *h_out);

/* ----------------------------------------------------------------------------------------
 * CDownConvert -- NCO mixer + decimate-by-2^n cascade (dsp/downconvert.h:24-120).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_downconvert csdr_downconvert;

/* CDownConvert::CDownConvert (downconvert.cpp:60-73): 100 kHz in, no stages, phasor 1+0j */
csdr_downconvert *csdr_downconvert_create(int device);
void csdr_downconvert_destroy(csdr_downconvert *d);
/* CDownConvert::SetCwOffset (downconvert.h:30) */
int csdr_downconvert_set_cw_offset(csdr_downconvert *d, double offset);
/* CDownConvert::SetFrequency (downconvert.cpp:98-107); stores freq + CW offset */
int csdr_downconvert_set_frequency(csdr_downconvert *d, double freq);
/* CDownConvert::SetDataRate (downconvert.cpp:114-173): rebuilds the stage list when
 * (in_rate, max_bw) change, re-applies the stored frequency, returns the output rate */
double csdr_downconvert_set_data_rate(csdr_downconvert *d, double in_rate, double max_bw);
/* CDownConvert::ProcessData (downconvert.cpp:186-263): n interleaved double pairs in,
 * n / 2^stages out (n must be a multiple of 2^stages and even, as in the reference);
 * in == out allowed.  The reference also scribbles intermediate data over pInData; this
 * implementation leaves the input untouched. */
int csdr_downconvert_process(csdr_downconvert *d, int n, const double *in_iq, double *out_iq);
/* introspection for tests: stage codes (3 = CIC3, else half-band length), stored NCO freq */
int csdr_downconvert_get_stages(csdr_downconvert *d, int *codes, int cap);
double csdr_downconvert_get_nco_freq(csdr_downconvert *d);

/* batched device-resident form; channel = -1 addresses every channel */
typedef struct csdr_downconvert_batch csdr_downconvert_batch;
csdr_downconvert_batch *csdr_downconvert_batch_create(int device, int channels);
void csdr_downconvert_batch_destroy(csdr_downconvert_batch *b);
int csdr_downconvert_batch_set_cw_offset(csdr_downconvert_batch *b, int channel, double offset);
int csdr_downconvert_batch_set_frequency(csdr_downconvert_batch *b, int channel, double freq);
double csdr_downconvert_batch_set_data_rate(csdr_downconvert_batch *b, int channel, double in_rate,
                                            double max_bw);
int csdr_downconvert_batch_get_stages(csdr_downconvert_batch *b, int channel, int *codes, int cap);
double csdr_downconvert_batch_get_nco_freq(csdr_downconvert_batch *b, int channel);
/* samples channel `channel` produces for n_in input samples (n_in >> stages) */
int csdr_downconvert_batch_out_count(csdr_downconvert_batch *b, int channel, int n_in);
/* d_in [channels][in_stride] -> d_out [channels][out_stride], interleaved fp32 I/Q on the
 * device; n_per_channel even and a multiple of every channel's 2^stages.  Asynchronous. */
int csdr_downconvert_batch_process(csdr_downconvert_batch *b, const float *d_in, long long in_stride,
                                   int n_per_channel, float *d_out, long long out_stride,
                                   void *stream);

/* ----------------------------------------------------------------------------------------
 * CAgc (dsp/agc.h:19-62), CSMeter (dsp/smeter.h:13-28), CFir (dsp/fir.h:20-43),
 * CIir (dsp/iir.h:17-39) -- the leaf objects the reference also exposes on their own.
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_agc csdr_agc;
csdr_agc *csdr_agc_create(int device);
void csdr_agc_destroy(csdr_agc *a);
/* CAgc::SetParameters (agc.cpp:104-167) */
int csdr_agc_set_parameters(csdr_agc *a, int on, int use_hang, int threshold, int manual_gain,
                            int slope, int decay, double sample_rate);
/* CAgc::ProcessData complex (agc.cpp:174-296) / real (agc.cpp:301-401); in == out allowed */
int csdr_agc_process_cpx(csdr_agc *a, int n, const double *in_iq, double *out_iq);
int csdr_agc_process_real(csdr_agc *a, int n, const double *in, double *out);

typedef struct csdr_smeter csdr_smeter;
csdr_smeter *csdr_smeter_create(int device);
void csdr_smeter_destroy(csdr_smeter *s);
/* CSMeter::ProcessData (smeter.cpp:62-93), GetPeak (:98-103, resets the peak), GetAve (:108-112) */
int csdr_smeter_process(csdr_smeter *s, int n, const double *in_iq, double sample_rate);
double csdr_smeter_get_peak(csdr_smeter *s);
double csdr_smeter_get_ave(csdr_smeter *s);

typedef struct csdr_fir csdr_fir;
csdr_fir *csdr_fir_create(int device);
void csdr_fir_destroy(csdr_fir *f);
/* CFir::InitConstFir (fir.cpp:133-153), InitLPFilter (:173-261), InitHPFilter (:278-367) return
 * the tap count; GenerateHBFilter (:374-407) keeps the delay line */
int csdr_fir_init_const(csdr_fir *f, int ntaps, const double *coef);
int csdr_fir_init_lp(csdr_fir *f, double scale, double astop, double fpass, double fstop, double fs);
int csdr_fir_init_hp(csdr_fir *f, double scale, double astop, double fpass, double fstop, double fs);
int csdr_fir_generate_hb(csdr_fir *f, double freq_offset);
int csdr_fir_get_taps(csdr_fir *f, double *coef, double *icoef, double *qcoef);   /* up to 75 each */
/* CFir::ProcessFilter real (fir.cpp:72-92) / complex (:101-127) */
int csdr_fir_process_real(csdr_fir *f, int n, const double *in, double *out);
int csdr_fir_process_cpx(csdr_fir *f, int n, const double *in_iq, double *out_iq);

typedef struct csdr_iir csdr_iir;
csdr_iir *csdr_iir_create(int device);
void csdr_iir_destroy(csdr_iir *f);
/* CIir::InitLP/HP/BP/BR (iir.cpp:86-165): kind 0 LP, 1 HP, 2 BP, 3 BR */
int csdr_iir_init(csdr_iir *f, int kind, double f0, double q, double sample_rate);
int csdr_iir_get_coefs(csdr_iir *f, double *b0b1b2a1a2);
/* CIir::ProcessFilter (iir.cpp:171-201) */
int csdr_iir_process_real(csdr_iir *f, int n, const double *in, double *out);
int csdr_iir_process_cpx(csdr_iir *f, int n, const double *in_iq, double *out_iq);

/* ----------------------------------------------------------------------------------------
 * Demodulators: CAmDemod (dsp/amdemod.h), CSamDemod (dsp/samdemod.h), CFmDemod
 * (dsp/fmdemod.h), CSsbDemod (dsp/ssbdemod.h).  mono: n complex in -> n real out;
 * stereo: n complex in -> n complex out.
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_amdemod csdr_amdemod;
csdr_amdemod *csdr_amdemod_create(int device, double sample_rate);            /* amdemod.cpp:50-54 */
void csdr_amdemod_destroy(csdr_amdemod *d);
int csdr_amdemod_set_bandwidth(csdr_amdemod *d, double bandwidth);            /* :56-60 */
int csdr_amdemod_process_mono(csdr_amdemod *d, int n, const double *in_iq, double *out);     /* :66-82 */
int csdr_amdemod_process_stereo(csdr_amdemod *d, int n, const double *in_iq, double *out_iq); /* :87-104 */

typedef struct csdr_samdemod csdr_samdemod;
csdr_samdemod *csdr_samdemod_create(int device, double sample_rate);          /* samdemod.cpp:54-73 */
void csdr_samdemod_destroy(csdr_samdemod *d);
int csdr_samdemod_process_mono(csdr_samdemod *d, int n, const double *in_iq, double *out);     /* :78-110 */
int csdr_samdemod_process_stereo(csdr_samdemod *d, int n, const double *in_iq, double *out_iq); /* :115-158 */

typedef struct csdr_fmdemod csdr_fmdemod;
csdr_fmdemod *csdr_fmdemod_create(int device, double sample_rate);            /* fmdemod.cpp:62-89 */
void csdr_fmdemod_destroy(csdr_fmdemod *d);
int csdr_fmdemod_set_squelch(csdr_fmdemod *d, int value);                     /* :95-98 */
int csdr_fmdemod_process_mono(csdr_fmdemod *d, int n, double fm_bw, const double *in_iq, double *out);     /* :157-192 */
int csdr_fmdemod_process_stereo(csdr_fmdemod *d, int n, double fm_bw, const double *in_iq, double *out_iq); /* :197-236 */
int csdr_fmdemod_get_squelched(csdr_fmdemod *d);                              /* m_SquelchState, for tests */

int csdr_ssbdemod_process_mono(int n, const double *in_iq, double *out);      /* ssbdemod.cpp:48-53 */
int csdr_ssbdemod_process_stereo(int n, const double *in_iq, double *out_iq); /* :55-60 */

/* ----------------------------------------------------------------------------------------
 * CDemodulator -- the whole receive chain (dsp/demodulator.h:56-100).
 * -------------------------------------------------------------------------------------- */
/* POD mirror of tDemodInfo (dsp/demodulator.h:35-54) without the QString label */
typedef struct csdr_demod_info {
    int HiCut, HiCutmin, HiCutmax, LowCut, LowCutmin, LowCutmax;
    int FilterClickResolution, Offset, SquelchValue;
    int AgcSlope, AgcThresh, AgcManualGain, AgcDecay;
    int AgcOn, AgcHangOn, Symetric;
} csdr_demod_info;

#define CSDR_DEMOD_AM 0      /* DEMOD_* (dsp/demodulator.h:20-26) */
#define CSDR_DEMOD_SAM 1
#define CSDR_DEMOD_FM 2
#define CSDR_DEMOD_USB 3
#define CSDR_DEMOD_LSB 4
#define CSDR_DEMOD_CWU 5
#define CSDR_DEMOD_CWL 6

typedef struct csdr_demod csdr_demod;
/* CDemodulator::CDemodulator (demodulator.cpp:47-60); fastfir_n 2048 is the reference's filter */
csdr_demod *csdr_demod_create(int device, int fastfir_n);
void csdr_demod_destroy(csdr_demod *d);
int csdr_demod_set_input_rate(csdr_demod *d, double rate);                    /* :92-99 */
int csdr_demod_set_demod(csdr_demod *d, int mode, const csdr_demod_info *info); /* :107-157 */
int csdr_demod_set_freq(csdr_demod *d, double freq);                          /* demodulator.h:68-69 */
double csdr_demod_get_output_rate(csdr_demod *d);
double csdr_demod_get_smeter_peak(csdr_demod *d);
double csdr_demod_get_smeter_ave(csdr_demod *d);
int csdr_demod_get_buf_limit(csdr_demod *d);                                  /* m_InBufLimit */
/* CDemodulator::ProcessData mono (:163-215) / stereo (:221-273): buffers n samples, runs the
 * chain every m_InBufLimit samples, every pass writes at out[0], returns the summed count */
int csdr_demod_process_mono(csdr_demod *d, int n, const double *in_iq, double *out);
int csdr_demod_process_stereo(csdr_demod *d, int n, const double *in_iq, double *out_iq);
/* same chain, passes append instead of overwriting (batch harness form) */
int csdr_demod_process_mono_append(csdr_demod *d, int n, const double *in_iq, double *out);
/* Deferred output (opt-in; no counterpart in the reference, whose ProcessData computes on the caller's thread).  With it
 * on, a pass that is due to return samples (dsp/demodulator.cpp:169-214, every m_InBufLimit samples) returns the samples
 * of the PREVIOUS such pass -- finished while the caller was handing over this window -- and leaves its own on the way:
 * the call never waits for the device, the chain's pass and the caller's next m_InBufLimit samples overlap.  The same
 * samples in the same order, one window later (10 ms at 2 MSPS); the first pass returns 0.  csdr_demod_flush hands over
 * the last pass (returns its count: mono reals, stereo complex pairs; cap in doubles) -- before a switch back, a mode
 * change between mono and stereo calls, or the end of the stream.  Not together with the stage taps. */
int csdr_demod_set_deferred(csdr_demod *d, int on);
int csdr_demod_flush(csdr_demod *d, double *out, int cap);
/* Stage taps of the chain: what the reference hands to g_pTestBench->DisplayData(n, buf, m_OutputRate, PROFILE_k) in
 * every pass (dsp/demodulator.cpp:175,180,187,208; gui/testbench.h:29-38) -- PROFILE_1 the down-converter's output,
 * PROFILE_2 the band-pass filter's, PROFILE_3 the AGC's (n complex samples each, n = 0 while the filter is filling),
 * PROFILE_4 the audio (mono: n reals, stereo: n complex).  mask bit k-1 switches PROFILE_k on; 0 = off (the default:
 * nothing of this costs anything then).  With taps on every pass waits for its results, the AGC's output goes through
 * device memory (S-meter + AGC and the demodulator as two launches; same words out), and per pass and profile either
 * `fn` is called -- from inside the ProcessData call, with `user` -- or, fn == NULL, the samples are appended to a
 * per-profile host buffer that csdr_demod_get_tap returns and empties (returns the number of doubles written; complex
 * samples are two). */
typedef void (*csdr_tap_fn)(void *user, int profile, int n, const double *data, int is_complex, double rate);
int csdr_demod_set_taps(csdr_demod *d, int mask, csdr_tap_fn fn, void *user);
int csdr_demod_get_tap(csdr_demod *d, int profile, double *out, int cap);

/* batched device-resident chain: configure every channel, commit once, then process */
typedef struct csdr_demod_batch csdr_demod_batch;
csdr_demod_batch *csdr_demod_batch_create(int device, int channels, int fastfir_n);
void csdr_demod_batch_destroy(csdr_demod_batch *b);
/* CDemodulator::SetInputSampleRate (dsp/demodulator.cpp:92-99) of every receiver.  Before commit(): recorded.  After
 * commit(): applied at once, at any time, as the host does on every bandwidth switch of the radio
 * (interface/sdrinterface.cpp:753-754): every down-converter is rebuilt for the new rate (new stage list from zeroed
 * histories; oscillator phase and amplitude kept; the CW offset added once more, downconvert.cpp:169), the output rate
 * and the S-meter's time constants follow, and -- like the reference -- filter taps and overlap, AGC constants and rings
 * and the demodulator objects stay as they are until the receiver's next SetDemod, which for an unchanged mode keeps the
 * demodulator built for the old output rate.  Receivers keep their rows while a plan group still shares one decimation;
 * one whose new chain decimates differently from its group's moves as after a mode change.  Synchronises the device. */
int csdr_demod_batch_set_input_rate(csdr_demod_batch *b, double rate);
/* CDemodulator::SetDemod (dsp/demodulator.cpp:107-157) of one receiver.  Before commit(): recorded.  After commit():
 * applied at once, like the reference between two ProcessData calls -- also a mode whose maximum bandwidth (hence
 * decimator chain and output rate) differs from the present one: the receiver then continues in a plan group of its
 * own with everything the reference keeps across SetDemod (oscillator, filter overlap and partly filled filter input,
 * AGC, S-meter; new demodulator, decimator from zero histories); nothing else of the batch is disturbed.  The call
 * synchronises the device. */
int csdr_demod_batch_set_demod(csdr_demod_batch *b, int channel, int mode, const csdr_demod_info *info);
/* csdr_demod_batch_set_demod for each of n entries, in array order (a channel named twice ends with its last entry).
 * An entry that keeps its receiver's mode on a committed batch does not design its filter on the caller's thread: CW
 * offset, AGC constants, S-meter rate, squelch / FM high-pass and AM low-pass are queued as patches as in the one-receiver
 * call, the frequency response goes to the filter object's device-side design queue -- one
 * csdr_fastfir_batch_setup_many per plan group -- and nothing waits.  An entry that changes the mode, and every entry
 * before commit(), runs the one-receiver call unchanged.  status (may be NULL): per entry what the one-receiver call
 * would have returned.  Returns CSDR_OK or the first error; bad arguments (null arrays, n < 0, a channel or mode out of
 * range) return CSDR_EINVAL and change nothing. */
int csdr_demod_batch_set_demod_many(csdr_demod_batch *b, int n, const int *channel, const int *mode,
                                    const csdr_demod_info *info, int *status);
int csdr_demod_batch_commit(csdr_demod_batch *b);
/* Receivers cut from shared streams (one radio, many receivers: SURVEY 8e "if channels are cut from one stream"):
 * receiver c reads row input_row[c] of d_in (or datagram stream input_row[c]) instead of row c; several receivers
 * may name the same row, each keeps its own CDownConvert / CFastFIR / AGC / demodulator state as in the reference,
 * where every CDemodulator is handed the same buffer (interface/sdrinterface.cpp:903).  input_row: `channels` ints on
 * the host, each in [0, channels); NULL restores row c for receiver c.  Before or after commit(); the call
 * synchronises the device. */
int csdr_demod_batch_set_input_rows(csdr_demod_batch *b, const int *input_row);
int csdr_demod_batch_set_freq(csdr_demod_batch *b, int channel, double freq);
double csdr_demod_batch_get_output_rate(csdr_demod_batch *b, int channel);
double csdr_demod_batch_get_smeter_ave(csdr_demod_batch *b, int channel);
/* CSMeter::GetAve / GetPeak (smeter.cpp:98-112) of every channel at once into device arrays [channels]
 * (either may be NULL); reading the peaks resets them, as GetPeak does.  Asynchronous on `stream`: ordered
 * behind the process calls issued on it.  What a multi-GPU host gathers from its ranks. */
int csdr_demod_batch_get_smeter_all(csdr_demod_batch *b, float *d_ave, float *d_peak, void *stream);
/* d_in [channels][in_stride] complex fp32 -> d_out [channels][out_stride] fp32 mono audio.
 * Numerical contract of the recurrent stages: the scans that replace the reference's per-sample loops (averagers,
 * AGC, locked PLL tiles) differ from the sequential fp64 loop by rounding only, and an FM tile whose loop is NOT
 * locked is walked by all threads at once, each from a warmed-up state that is CHECKED to meet its predecessor's to
 * 1e-9 turns -- a bound, not bit equality: the audio of such tiles (noise, acquisition) can differ from a one-thread
 * walk, and between builds with another tiling, by up to ~1e-6 of full scale (tests: 1e-6; CSDR_PLL_OVERLAP=0 selects
 * the one-thread walk).  Strict and pipelined mode run the same kernels with the same tiling: identical words.
 * The audio WORDS do not depend on how a stream is cut into calls either, as long as every call is a whole number of
 * 512-sample tiles (the down-converter re-anchors its oscillator on a grid counted from the receiver's first sample,
 * the filter walks whole hops, the post-chain whole bursts): one call of 24 windows = 24 calls of one, bit for bit. */
int csdr_demod_batch_process(csdr_demod_batch *b, const float *d_in, long long in_stride,
                             int n_per_channel, float *d_out, long long out_stride, void *stream);
/* Pipelined mode for streaming hosts (off by default).  on != 0: a process call only enqueues, and a call's post-chains
 * (S-meter, AGC, demodulator) run on internal streams beside the NEXT call's down-converters.  In the caller's stream
 * order, after process call k+1 the INPUT buffer of call k has been consumed and the OUTPUT rows of call k are complete;
 * after csdr_demod_batch_flush everything issued so far is complete.  Same results as the strict mode, word for word.
 * One form, the chained one: the strict mode's schedule (one down-converter at a time, every group's filter in queue
 * order behind its down-converter) carried across calls, two streams per plan group, within HIP's default four hardware
 * queues.  on = 1, 2 and 3 are the same (2 and 3 once named two forms; the three-stage form behind 3 was retired as
 * the slower one: 1.75-1.80 against 1.65-1.68 ms per call on 256 mixed receivers; the strict mode: 1.60-1.65).  Plan
 * groups that a later SetDemod or csdr_demod_batch_set_input_rate opens run pipelined like the others.  CSDR_ESTATE
 * while stage taps are on (csdr_demod_batch_set_taps(b, 0) first). */
int csdr_demod_batch_set_pipelined(csdr_demod_batch *b, int on);
int csdr_demod_batch_flush(csdr_demod_batch *b, void *stream);
/* the stereo overload (dsp/demodulator.cpp:221-273: AM/FM duplicate the audio into both halves, SAM splits the
 * sidebands, SSB/CW copy the filtered I/Q) for every channel: d_out_iq [channels][out_stride] complex fp32,
 * out_stride in complex samples */
int csdr_demod_batch_process_stereo(csdr_demod_batch *b, const float *d_in, long long in_stride,
                                    int n_per_channel, float *d_out_iq, long long out_stride, void *stream);
int csdr_demod_batch_out_count(csdr_demod_batch *b, int channel);
/* The same stage taps for the receivers of a batch (strict mode only).  With a non-zero mask every group keeps the
 * LAST call's down-converter output, filter output and AGC output in device memory (the AGC's through a split launch,
 * as above); csdr_demod_batch_get_tap copies receiver `channel`'s samples of that call to host memory -- PROFILE_1 ..
 * 3: interleaved fp32 I/Q, PROFILE_1 counts the samples the down-converter appended in that call, 2 and 3 the samples
 * the filter released -- and returns the number of floats (synchronous; PROFILE_4 is the caller's own output row).
 * The mask holds for every receiver, also for one that a mode or input-rate change moves into a new plan group.  Both
 * orders are refused with CSDR_ESTATE: set_taps on a pipelined batch, set_pipelined on a batch with taps on. */
int csdr_demod_batch_set_taps(csdr_demod_batch *b, int mask);
int csdr_demod_batch_get_tap(csdr_demod_batch *b, int channel, int profile, float *out, int cap);
/* Diagnostics: the number of plan groups the batch runs per call (rows that share one decimation; every group is one
 * set of launches), and with rows != NULL the number of rows -- live and muted -- of all groups.  A mode change to a
 * chain of the same decimation stays in its row; one to another decimation moves the receiver into a muted row of a
 * matching group when there is one, else into a group of its own; a group whose rows are all muted is dropped. */
int csdr_demod_batch_group_count(csdr_demod_batch *b, int *rows);
/* ---- the same chain over SEVERAL devices from one host object -------------------------------------------
 * Receivers are independent: shard s owns the contiguous channel range [s C / N, (s+1) C / N) on device devices[s], with
 * all its state resident there; a process call is N asynchronous batch calls, no collective on the data path.  Global
 * channel ids everywhere; set_demod / set_freq are routed to the owning shard.  What crosses devices is what the
 * survey names: the S-meters gathered to the host, and -- for receivers cut from ONE radio's stream, as
 * CSdrInterface hands every CDemodulator the same buffer (interface/sdrinterface.cpp:903) -- the broadcast of that
 * block to every other shard's device (hipMemcpyPeerAsync over xGMI, one copy per device on the shard's stream).
 * Several shards may name the same device.  A host with one PROCESS per GPU (bench.py --gpus N, torch.distributed /
 * RCCL) uses csdr_demod_batch per rank instead. */
typedef struct csdr_demod_shard csdr_demod_shard;
csdr_demod_shard *csdr_demod_shard_create(const int *devices, int nshards, int channels, int fastfir_n);
void csdr_demod_shard_destroy(csdr_demod_shard *s);
int csdr_demod_shard_count(csdr_demod_shard *s);
int csdr_demod_shard_range(csdr_demod_shard *s, int shard, int *first, int *count, int *device);
int csdr_demod_shard_set_input_rate(csdr_demod_shard *s, double rate);   /* every shard's batch; before or after commit */
int csdr_demod_shard_set_demod(csdr_demod_shard *s, int channel, int mode, const csdr_demod_info *info);
/* csdr_demod_batch_set_demod_many with GLOBAL channel ids: entries routed to the owning shards, one call per shard */
int csdr_demod_shard_set_demod_many(csdr_demod_shard *s, int n, const int *channel, const int *mode,
                                    const csdr_demod_info *info, int *status);
int csdr_demod_shard_commit(csdr_demod_shard *s);
int csdr_demod_shard_set_freq(csdr_demod_shard *s, int channel, double freq);
double csdr_demod_shard_get_output_rate(csdr_demod_shard *s, int channel);
int csdr_demod_shard_set_pipelined(csdr_demod_shard *s, int on);
/* d_in[k] / d_out[k]: shard k's rows [count_k][stride] on ITS device; streams[k] or NULL (the object's own streams) */
int csdr_demod_shard_process(csdr_demod_shard *s, const float *const *d_in, long long in_stride, int n_per_channel,
                             float *const *d_out, long long out_stride, void *const *streams);
int csdr_demod_shard_out_count(csdr_demod_shard *s, int channel);
/* shared-stream mode: receiver c reads row input_row[c] (< nrows <= receivers per shard) of a wide-band block that
 * process_shared takes ONCE, resident on src_device behind src_stream's work, and copies to the other devices */
int csdr_demod_shard_set_input_rows(csdr_demod_shard *s, const int *input_row, int nrows);
int csdr_demod_shard_process_shared(csdr_demod_shard *s, const float *d_block, int src_device, void *src_stream,
                                    long long in_stride, int n_per_channel, float *const *d_out, long long out_stride);
/* The datagram and blanker forms of the one-device batch on every shard.  set_blanker = CNoiseProc::SetupBlanker for all
 * receivers (noiseproc.cpp:78-119; the shard object owns one csdr_noiseproc_batch per device); process_packets takes
 * d_packets[s] = shard s's receivers' datagrams on ITS device ([count_s][npackets][pkt_len] bytes, as
 * csdr_demod_batch_process_packets) and runs the blanker fused in front when one is set; process_blanked is
 * csdr_demod_shard_process with that blanker in front of fp32 rows. */
int csdr_demod_shard_set_blanker(csdr_demod_shard *s, int on, double threshold, double width_us, double sample_rate);
int csdr_demod_shard_process_packets(csdr_demod_shard *s, const void *const *d_packets, int npackets, int pkt_len,
                                     float *const *d_out, long long out_stride, void *const *streams);
int csdr_demod_shard_process_blanked(csdr_demod_shard *s, const float *const *d_in, long long in_stride, int n_per_channel,
                                     float *const *d_out, long long out_stride, void *const *streams);
/* waits for everything issued on the shards' own streams (pipelined mode: flushes first) */
int csdr_demod_shard_sync(csdr_demod_shard *s);
/* CSMeter::GetAve / GetPeak of every receiver into HOST arrays indexed by global channel (either may be NULL; reading
 * the peaks resets them): the gather of SURVEY 8e.  Synchronous. */
int csdr_demod_shard_get_smeter_all(csdr_demod_shard *s, float *h_ave, float *h_peak);

/* The same pass fed with the datagrams as they arrived (interface/netiobase.cpp:479-527):
 * d_packets [channels][npackets][pkt_len] bytes on the device, 4-byte aligned, pkt_len 1028 (16 bit) or 1444
 * (24 bit).  No unpack pass: the first kernel at input rate decodes the datagrams in its own loads -- the
 * down-converter, or the blanker when nb is given (what CSdrInterface::ProcessIQData runs in place before the
 * chain, sdrinterface.cpp:884; nb may be NULL, it must have as many channels).  npackets * samples-per-packet
 * must be a multiple of the largest decimation in use.  Forward declaration: csdr_noiseproc_batch is defined
 * further down. */
struct csdr_noiseproc_batch;
int csdr_demod_batch_process_packets(csdr_demod_batch *b, const void *d_packets, int npackets, int pkt_len,
                                     struct csdr_noiseproc_batch *nb, float *d_out, long long out_stride,
                                     void *stream);

/* csdr_demod_batch_process with CNoiseProc's blanker in front (interface/sdrinterface.cpp:884 runs it in place before
 * the chain), fused: the blanker pass leaves one bit per sample and the down-converter zeroes the delayed sample under
 * it in its own load -- no blanked copy of d_in exists.  nb: as many channels as b; every receiver reads its own row
 * (not with csdr_demod_batch_set_input_rows).  The two-pass equivalent: csdr_noiseproc_batch_process into a buffer of
 * the caller's, then csdr_demod_batch_process on that. */
int csdr_demod_batch_process_blanked(csdr_demod_batch *b, const float *d_in, long long in_stride, int n_per_channel,
                                     struct csdr_noiseproc_batch *nb, float *d_out, long long out_stride, void *stream);

/* ----------------------------------------------------------------------------------------
 * CFft -- display spectrum and plain transforms (dsp/fft.h:24-85).  FFT sizes 512..65536 as in
 * the reference (clamped to that range, fft.cpp:140-145); a size that is not a power of two
 * returns CSDR_EINVAL.
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_fft csdr_fft;
csdr_fft *csdr_fft_create(int device);                                       /* fft.cpp:41-62 */
void csdr_fft_destroy(csdr_fft *f);
int csdr_fft_set_params(csdr_fft *f, int size, int invert, double db_comp, double fs);  /* :118-243 */
int csdr_fft_set_ave(csdr_fft *f, int ave);                                  /* :103-113 */
int csdr_fft_reset(csdr_fft *f);                                             /* :248-259 */
/* CFft::PutInDisplayFFT (:267-288): n complex doubles (n = FFT size); returns m_TotalCount */
int csdr_fft_put_display(csdr_fft *f, int n, const double *in_iq);
/* CFft::GetScreenIntegerFFTData (:308-410): fills out[0..max_w), returns the overload flag */
int csdr_fft_get_screen(csdr_fft *f, int max_h, int max_w, double max_db, double min_db,
                        int start_hz, int stop_hz, int *out);
/* m_pFFTAveBuf (bels, display order, `size` floats) for tests; returns the size */
int csdr_fft_get_ave(csdr_fft *f, float *out);
/* CFft::FwdFFT / RevFFT (:416-426): in-place, unnormalised, FwdFFT has the POSITIVE exponent */
int csdr_fft_fwd(csdr_fft *f, double *inout_iq);
int csdr_fft_rev(csdr_fft *f, double *inout_iq);
/* the same with the caller's doubles transformed as they are, in fp64 (csdr_fft_batch_fwd_f64 on one row) */
int csdr_fft_fwd_f64(csdr_fft *f, double *inout_iq);
int csdr_fft_rev_f64(csdr_fft *f, double *inout_iq);

/* batched spectra: [channels][in_stride] complex fp32 on the device, nframes frames per row */
typedef struct csdr_fft_batch csdr_fft_batch;
csdr_fft_batch *csdr_fft_batch_create(int device, int channels);
void csdr_fft_batch_destroy(csdr_fft_batch *f);
int csdr_fft_batch_set_params(csdr_fft_batch *f, int size, int invert, double db_comp, double fs);
int csdr_fft_batch_set_ave(csdr_fft_batch *f, int ave);
int csdr_fft_batch_reset(csdr_fft_batch *f);
int csdr_fft_batch_size(csdr_fft_batch *f);
int csdr_fft_batch_put_display(csdr_fft_batch *f, const float *d_in, long long in_stride, int nframes,
                               void *stream);
/* CFft::FwdFFT / RevFFT (fft.cpp:416-426) of nframes frames of every row.
 * The frame size is the object's (csdr_fft_batch_set_params, 512..65536).
 * Frame k of row c is d_in[(c*in_stride + k*size) .. + size) complex fp32.
 * Its transform goes to the same place in d_out with out_stride.
 * Unnormalised; FwdFFT has the POSITIVE exponent, RevFFT the negative one, as csdr_fft_fwd / _rev.
 * d_out == d_in with out_stride == in_stride transforms in place (what the reference does).
 * Any other overlap of the two row blocks is refused.
 * Bases 8-byte aligned, strides in complex samples, each >= nframes*size.
 * Asynchronous on `stream`; nothing is allocated per call and the host waits for nothing.
 * Reads and writes nothing of the display state (average, counters, overload flags, frame carry).
 * The reference's FwdFFT also feeds the display average; this one does not.
 * nframes == 0: CSDR_OK, no launch.
 * CSDR_EINVAL before anything is written for NULL, nframes < 0, a short stride or a partial overlap. */
int csdr_fft_batch_fwd(csdr_fft_batch *f, const float *d_in, long long in_stride, float *d_out,
                       long long out_stride, int nframes, void *stream);
int csdr_fft_batch_rev(csdr_fft_batch *f, const float *d_in, long long in_stride, float *d_out,
                       long long out_stride, int nframes, void *stream);
/* frames of every row that one pass of the 32768- and 65536-point transforms takes through the object's work buffer
 * (sized in csdr_fft_batch_set_params); a longer call runs in groups of this many on the stream.  0 at the other sizes.
 * Calls on one object share that buffer: keep them on one stream, or order them. */
int csdr_fft_batch_plain_group(csdr_fft_batch *f);
/* The same transforms in fp64, the reference's own precision (TYPECPX = two doubles): complex fp64 rows in and out.
 * The contract is the one above with double pairs: strides in complex samples, bases 16-byte aligned.
 * d_out == d_in with equal strides transforms in place; any other overlap is CSDR_EINVAL before anything is written.
 * nframes == 0: CSDR_OK, no launch.  Asynchronous on `stream`; nothing of the display state is read or written.
 * The fp64 tables (every entry rounded once from long double) and, at 8192 points and above, the fp64 work buffer
 * belong to the object's present size: csdr_fft_batch_prepare_f64 builds them (it may allocate and wait),
 * csdr_fft_batch_set_params drops them, and a transform call on an unprepared object prepares it first.
 * After that a call allocates nothing and waits for nothing.  An object that never asks for fp64 holds none of it.
 * At 8192 points and above an object of more than 65535 rows is CSDR_EINVAL (before anything is allocated). */
int csdr_fft_batch_prepare_f64(csdr_fft_batch *f);
int csdr_fft_batch_fwd_f64(csdr_fft_batch *f, const double *d_in, long long in_stride, double *d_out,
                           long long out_stride, int nframes, void *stream);
int csdr_fft_batch_rev_f64(csdr_fft_batch *f, const double *d_in, long long in_stride, double *d_out,
                           long long out_stride, int nframes, void *stream);
/* frames of every row that one pass of the fp64 four-step form (8192 ... 65536 points) takes through its work buffer;
 * 0 at the other sizes.  Calls on one object share that buffer: keep them on one stream, or order them. */
int csdr_fft_batch_plain_group_f64(csdr_fft_batch *f);
int csdr_fft_batch_get_ave(csdr_fft_batch *f, int channel, float *out);
int csdr_fft_batch_get_total_count(csdr_fft_batch *f, int channel);
int csdr_fft_batch_get_screen(csdr_fft_batch *f, int channel, int max_h, int max_w, double max_db,
                              double min_db, int start_hz, int stop_hz, int *out);
/* the same mapping for every channel at once, on the device: d_out is
 * [channels][out_stride] int32 on the device, out_stride >= max_w; pixels that no bin maps to keep
 * what d_out held (the reference leaves them untouched too).  d_overload: optional [channels] int32,
 * the overload flag of each channel's last PutInDisplayFFT.  Asynchronous on `stream`. */
int csdr_fft_batch_get_screen_all(csdr_fft_batch *f, int max_h, int max_w, double max_db, double min_db,
                                  int start_hz, int stop_hz, int *d_out, long long out_stride, int *d_overload,
                                  void *stream);
/* CPlotter's waterfall palette (gui/plotter.cpp:67-83): 256 colours, 0xFFRRGGBB each (QRgb order) */
void csdr_plotter_color_table(unsigned int *out256);
/* The new top line of the waterfall of every channel (CPlotter::draw, gui/plotter.cpp:425-441):
 * GetScreenIntegerFFTData(255, max_w, ...) and, per pixel, the palette entry 255 - y.  d_rgb is
 * [channels][out_stride] 0xFFRRGGBB on the device, out_stride >= max_w; pixels that no bin maps to keep what
 * d_rgb held (the reference paints them from an uninitialised buffer).  d_overload as above.  Asynchronous. */
int csdr_fft_batch_get_waterfall_all(csdr_fft_batch *f, int max_w, double max_db, double min_db, int start_hz,
                                     int stop_hz, unsigned int *d_rgb, long long out_stride, int *d_overload,
                                     void *stream);

/* The display path of CSdrInterface::ProcessIQData (interface/sdrinterface.cpp:878-907) on the device: each call
 * appends n samples of every row to the display stream.  Each sample has the channel's DC offset subtracted
 * (:889-894) and goes into the frame being filled (m_DataBuf, kept per channel on the device across calls).  When a
 * frame of `size` samples completes, the skip counter (:898-900) and, if enabled, the screen gate (:901-906) decide
 * whether it reaches PutInDisplayFFT.  The frame position and the partial frame's length are one per object: every row
 * gets the same sample count per call.  Skip value, skip counter, gate and ready flag -- and the averaging length -- are
 * one set per object in the UNIFORM form, which the object-wide setters keep, and one set per ROW in the row form, which
 * any csdr_fft_batch_*_row setter below enters: there each row is one listener with its own display rate, smoothing and
 * ScreenUpdateDone(), a row that uses no frame in a call is not touched (average, counters and overload word as they
 * were), and the put calls return the largest per-row count; csdr_fft_batch_get_emits tells which rows emitted.  Used
 * frames go through exactly the averaging, log and overload code
 * of csdr_fft_batch_put_display, so get_ave / get_total_count / get_screen_all / get_waterfall_all work unchanged.
 * With the blanker on, the reference's display sees the blanked, delayed samples (:884 runs in place first):
 * csdr_fft_batch_put_display_stream_blanked / _packets_blanked below give that picture behind a blanked chain call,
 * from the mask the call left -- no second blanker pass.
 * The SPUR_CAL_MAXSAMPLES bookkeeping of NcoSpurCalibrate and its commands, per receiver on the device, are
 * csdr_spurcal_batch_* below: its csdr_spurcal_batch_dc() is a d_dc for these calls.  The reference calibrates behind
 * the blanker (:886); csdr_spurcal_batch_put_*_blanked see those samples from the mask of the chain call, as the blanked
 * display pair does, while the stateless csdr_ingest_spurcal* see the input they are handed.
 * Out of scope: shard forms (of the plain and of the blanked pair). */
/* SetMaxDisplayRate (sdrinterface.h:112-114): skip value = (int)(sample_rate / (size * max_display_rate)), counter 0.
 * gated != 0 turns on the m_ScreenUpateFinished handshake: after a used frame, none is used until
 * csdr_fft_batch_screen_update_done.  Until this is called the skip value is 0 (every frame) and the gate is off.
 * csdr_fft_batch_set_params sets the frame position to 0 and, once a display rate is set, re-derives the skip value
 * from its own size and fs with the last max_display_rate, as SetFftSize does (:709-718). */
int csdr_fft_batch_set_display_rate(csdr_fft_batch *f, double sample_rate, int max_display_rate, int gated);
/* ScreenUpdateDone() (sdrinterface.h:67) */
int csdr_fft_batch_screen_update_done(csdr_fft_batch *f);
/* StartSdr (:512, :591): frame position 0, gate open (in the row form: every row's) */
int csdr_fft_batch_stream_reset(csdr_fft_batch *f);
/* The row form.  row in [0, channels) is one row, row < 0 every row; any other row: CSDR_EINVAL, nothing changed.
 * After one of the three setters the object is in the row form (csdr_fft_batch_row_form: 1) -- also when every row then
 * holds the same values: nothing looks for uniformity.  There the five put calls plan each row by itself
 * (put_display: every row nframes frames with the row's averaging length).  The object-wide csdr_fft_batch_set_ave
 * and csdr_fft_batch_set_display_rate write every row and end their half (averaging / display) of the row form; with
 * both ended the object is uniform again and runs the uniform code.  set_display_rate leaves ONE ready flag: set if every
 * row's was.  csdr_fft_batch_screen_update_done sets every row ready.  csdr_fft_batch_set_params re-derives every row's
 * skip value from that row's stored display rate and zeroes the counters.
 * set_ave_row: CFft::SetFFTAve of that row (ave <= 0: 1), then ResetFFT of THAT row: average, sum and both counters of
 * the other rows stay as they are.  reset_row: ResetFFT of one row (changes no form).
 * set_display_rate_row: SetMaxDisplayRate at the object's sample rate (the last set_display_rate's, else set_params's fs)
 * and size, counter 0; gated switches that row's m_ScreenUpateFinished handshake.  max_display_rate >= 1.
 * screen_update_done_row: ScreenUpdateDone() of one listener.
 * Not per row: FFT size, sample rate, invert flag, dB compensation, frame position, stream_reset. */
int csdr_fft_batch_set_ave_row(csdr_fft_batch *f, int row, int ave);
int csdr_fft_batch_reset_row(csdr_fft_batch *f, int row);
int csdr_fft_batch_set_display_rate_row(csdr_fft_batch *f, int row, int max_display_rate, int gated);
int csdr_fft_batch_screen_update_done_row(csdr_fft_batch *f, int row);
int csdr_fft_batch_row_form(csdr_fft_batch *f);
/* out[channels]: the frames each row used in the object's last put call, each one an emit NewFftData() for that
 * listener (uniform form: every entry the call's return value).  Host state only: waits for nothing. */
int csdr_fft_batch_get_emits(csdr_fft_batch *f, int *out);
/* n samples of every row of d_in ([channels][in_stride] complex fp32, 8-byte aligned) appended to the display stream;
 * returns the number of frames that entered the average in this call (each one an emit NewFftData()), >= 0, or CSDR_E*.
 * d_dc: optional [channels][2] doubles (I, Q), subtracted as csdr_ingest_unpack does, (float)((double)v - dc); read on
 * `stream`, so a csdr_ingest_spurcal* issued before it on the same stream is seen (:886 runs before :889).  A call that
 * uses no frame launches no spectrum work and leaves average, counters and overload flags as they were; it still
 * updates the partial frame.  Asynchronous on `stream`. */
int csdr_fft_batch_put_display_stream(csdr_fft_batch *f, const float *d_in, long long in_stride, int n,
                                      const double *d_dc, void *stream);
/* the same on datagrams: d_packets [channels][npackets][pkt_len] bytes on the device, decoded in the spectrum kernels'
 * frame load (2048 ... 8192 points; a frame that begins in the carry, and the other sizes, through a gather) --
 * the rules of csdr_demod_batch_process_packets (pkt_len 1028 or 1444, 4-byte aligned, below 2 GiB per channel) */
int csdr_fft_batch_put_display_packets(csdr_fft_batch *f, const void *d_packets, int npackets, int pkt_len,
                                       const double *d_dc, void *stream);
/* The display stream of the samples the LAST blanked chain call of `b` consumed, as its blanker handed them over
 * (:884): stream sample s of row c, before the DC correction, is
 *     blanker of c on ? (mask bit s of the call set ? (0, 0) : input[s - delay_n - 1]) : input[s]
 * with input[j < 0] the samples of the calls before -- the rule the blanked down-converter applies in its own loads; a
 * blanked sample becomes -dc (:891-894) and the carried partial frame holds blanked samples, as m_DataBuf does.  Nothing
 * is blanked twice: the call reads the mask, the blanker's state and the history the chain call left on the device.
 * Return value, frame logic, averaging and readers are those of the unblanked pair; a receiver whose blanker is off gets
 * exactly its samples.  The contract:
 *  - call it after csdr_demod_batch_process_blanked (-> _put_display_stream_blanked) or csdr_demod_batch_process_packets
 *    with a blanker (-> _put_display_packets_blanked), with the same `stream`, the same input buffer and the same count
 *    (and stride / packet length), and BEFORE the next call on `b`: the mask is single-buffered and the blanker's
 *    history halves alternate;
 *  - f and b are on the same device and have the same number of channels; every receiver reads its own row (what
 *    process_blanked demands);
 *  - the blanker object of that call still exists and has not been set up in between;
 *  - strict and pipelined mode both work: the display only reads, on the caller's stream, behind the call's mask pass,
 *    and the next call's mask pass is ordered behind it on that stream.
 * CSDR_ESTATE when the last process call of `b` was not such a call (none yet, an unblanked one, or a commit or a rate
 * change since; with CSDR_BLANK_FUSED=0 the chain runs the two-pass blanker and leaves no mask: CSDR_ESTATE too);
 * CSDR_EINVAL when buffer, form, count, channels or device differ.  A refused call changes nothing.
 * The frames are read where they lie at 2048 and 4096 points (the first one or two of a call, whose delayed samples
 * may lie in front of it, and every other size through the gather). */
int csdr_fft_batch_put_display_stream_blanked(csdr_fft_batch *f, csdr_demod_batch *b, const float *d_in,
                                              long long in_stride, int n, const double *d_dc, void *stream);
int csdr_fft_batch_put_display_packets_blanked(csdr_fft_batch *f, csdr_demod_batch *b, const void *d_packets,
                                               int npackets, int pkt_len, const double *d_dc, void *stream);

/* ----------------------------------------------------------------------------------------
 * CFractResampler (dsp/fractresampler.h:17-33)
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_resampler csdr_resampler;
csdr_resampler *csdr_resampler_create(int device);
void csdr_resampler_destroy(csdr_resampler *r);
int csdr_resampler_init(csdr_resampler *r, int max_input_size);              /* fractresampler.cpp:85-135 */
/* Resample overloads: rate = input rate / output rate; return the output sample count */
int csdr_resampler_resample_real(csdr_resampler *r, int n, double rate, const double *in, double *out);       /* :258-297 */
int csdr_resampler_resample_cpx(csdr_resampler *r, int n, double rate, const double *in_iq, double *out_iq);  /* :144-184 */
int csdr_resampler_resample_real_i16(csdr_resampler *r, int n, double rate, const double *in, short *out,
                                     double gain);                           /* :306-352 */
int csdr_resampler_resample_cpx_i16(csdr_resampler *r, int n, double rate, const double *in_iq, short *out_lr,
                                    double gain);                            /* :194-249 */

/* device-resident batch form for the chain's mono audio rows: [channels][stride] fp32 in; fp32 or
 * int16 (scaled by gain, clipped, truncated: fractresampler.cpp:306-352) out.  Every channel runs
 * on the same clock: one rate and one time accumulator (m_FloatTime) for the batch.  Returns the
 * output samples per channel; asynchronous on `stream`. */
typedef struct csdr_resampler_batch csdr_resampler_batch;
csdr_resampler_batch *csdr_resampler_batch_create(int device, int channels);
void csdr_resampler_batch_destroy(csdr_resampler_batch *b);
int csdr_resampler_batch_resample(csdr_resampler_batch *b, const float *d_in, long long in_stride, int n, double rate,
                                  float *d_out_f32, short *d_out_i16, long long out_stride, double gain, void *stream);

/* ----------------------------------------------------------------------------------------
 * Sound-sink adaptation: the queue and rate-error loop of CSoundOut
 * (interface/soundout.cpp, both modes) around the device resampler -- the step right after the path in
 * a live receiver.  put = PutOutQueue (:196-305): resample to 48 kHz int16 with Rate = m_OutRatio *
 * (1 + m_RateCorrection) and the volume gain, queue (16384 entries; overflow drops a quarter); get = GetOutQueue
 * (:311-445) for the audio thread (silence until half full, underflow backs up a quarter); every second of
 * consumed samples the P-controller CalcError (:456-468) sets the correction from the average fill level.
 * One producer thread and one consumer thread as in the reference: the caller serialises put and get per handle.
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_soundsink csdr_soundsink;
csdr_soundsink *csdr_soundsink_create(int device, int stereo);               /* soundout.cpp:60-76 */
void csdr_soundsink_destroy(csdr_soundsink *s);
int csdr_soundsink_change_user_data_rate(csdr_soundsink *s, double rate);    /* :155-175 */
int csdr_soundsink_set_blocking(csdr_soundsink *s, int on);                  /* Start(..., BlockingMode) :86-90: put waits while the queue is full (:209-220), get skips the rate loop (:354-358) */
int csdr_soundsink_set_volume(csdr_soundsink *s, int vol);                   /* :180-189 */
/* in: n doubles (mono sink) or n interleaved double pairs (stereo sink), at most 8192 samples; returns the
 * resampled samples produced */
int csdr_soundsink_put(csdr_soundsink *s, int n, const double *in);
/* out: n shorts, or n L/R pairs of a stereo sink; returns n */
int csdr_soundsink_get(csdr_soundsink *s, int n, short *out);
double csdr_soundsink_get_rate_correction(csdr_soundsink *s);                /* m_RateCorrection */
double csdr_soundsink_get_ave_level(csdr_soundsink *s);                      /* m_AveOutQLevel */
int csdr_soundsink_get_level(csdr_soundsink *s);                             /* m_OutQLevel */
int csdr_soundsink_get_ppm_error(csdr_soundsink *s);                         /* m_PpmError */

/* ----------------------------------------------------------------------------------------
 * Batch sound sink: C independent CSoundOut sinks (non-blocking mode) behind the batched chain, the last step from
 * "rows of audio at group rates on the device" to "48 kHz int16 per listener".  Every receiver has its own user
 * rate (m_OutRatio), volume, resampler state (m_FloatTime and the 28-sample history), 16384-entry queue and rate
 * loop, with the single sink's rules; put resamples every receiver at its own rate in one launch.
 * Threads: one producer calls put; any number of consumers call get and the accessors, at most one per receiver at a
 * time.  Each receiver has its own mutex; put reads each receiver's rate and gain under it.  Nothing here waits on
 * the whole device: put waits on `stream` only.
 * Left out: blocking mode (Start(..., BlockingMode)) -- in a batch one full queue would stall every receiver -- and a
 * shard form (a shard host makes one sink batch per shard device).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_soundsink_batch csdr_soundsink_batch;
/* NULL without a HIP device (no CPU fallback) */
csdr_soundsink_batch *csdr_soundsink_batch_create(int device, int channels, int stereo);
void csdr_soundsink_batch_destroy(csdr_soundsink_batch *s);
/* channel < 0: every receiver.  Clears only that receiver's queue; its resampler state is kept (soundout.cpp:155-175) */
int csdr_soundsink_batch_change_user_data_rate(csdr_soundsink_batch *s, int channel, double rate);
int csdr_soundsink_batch_set_volume(csdr_soundsink_batch *s, int channel, int vol);       /* :180-189; channel < 0: every receiver */
/* PutOutQueue (:196-305, non-blocking branch) for every receiver at once.
 * d_in:   device [channels][in_stride] fp32 mono rows, or complex fp32 rows of a stereo sink (in_stride in samples of
 *         the row): the output of csdr_demod_batch_process / _process_stereo.
 * n_in:   host array of per-receiver counts, each 0..8192 (csdr_demod_batch_out_count of each channel); a row with 0
 *         produces nothing and changes nothing.
 * n_out:  optional host array, receives the resampled count of each receiver.
 * CSDR_EINVAL before any state changes if a row breaks a rule (n_in <= 8192, n_in / rate + 8 <= 16384).  Ordered
 * behind `stream`; returns when every queue holds its new samples. */
int csdr_soundsink_batch_put(csdr_soundsink_batch *s, const float *d_in, long long in_stride, const int *n_in,
                             int *n_out, void *stream);
/* GetOutQueue (:311-445) of one receiver: n samples, or n L/R pairs of a stereo sink; returns n */
int csdr_soundsink_batch_get(csdr_soundsink_batch *s, int channel, int n, short *out);
/* PROFILE_5 (interface/soundout.cpp:207, :265; gui/testbench.h:29-38): the resampled int16 samples of the LAST put on
 * their way into the queues, at the sink's 48 kHz -- what the reference hands to DisplayData(n, m_pData, 48000,
 * PROFILE_5).  *d_rows: device pointer to [channels][*stride] int16 (int16 L/R pairs of a stereo sink, *stride in
 * pairs), *d_counts: device pointer to [channels] int32, the resampled count of each receiver (0 for a row with n_in =
 * 0).  They are the staging the put itself fills (pinned host memory mapped into the device): nothing is copied, the
 * pointers are the same after every put, the rows are complete when put returns (it has waited on its stream) and
 * valid until the next put begins.  Made for csdr_scope_batch_put_mono16 / _stereo16.  CSDR_ESTATE before the first
 * put.  Out of scope: a shard form, PROFILE_6 (the reference has it commented out: samdemod.cpp:91-92). */
int csdr_soundsink_batch_get_tap(csdr_soundsink_batch *s, const short **d_rows, long long *stride,
                                 const int **d_counts);
double csdr_soundsink_batch_get_rate_correction(csdr_soundsink_batch *s, int channel);    /* m_RateCorrection */
double csdr_soundsink_batch_get_ave_level(csdr_soundsink_batch *s, int channel);          /* m_AveOutQLevel */
int csdr_soundsink_batch_get_level(csdr_soundsink_batch *s, int channel);                 /* m_OutQLevel */
int csdr_soundsink_batch_get_ppm_error(csdr_soundsink_batch *s, int channel);             /* m_PpmError */

/* ----------------------------------------------------------------------------------------
 * Input-rate stages in front of the down-converter
 *
 * CNoiseProc (dsp/noiseproc.h:23-58): impulse blanker.  setup = SetupBlanker (noiseproc.cpp:78-119,
 * including its quirk that a change of the sample rate alone is ignored); process =
 * ProcessBlanker (:121-176).  Returns CSDR_EINVAL for sample rates whose 5 ms magnitude window
 * does not fit the reference's 32768-entry buffer (the reference overruns it).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_noiseproc csdr_noiseproc;
csdr_noiseproc *csdr_noiseproc_create(int device);                           /* noiseproc.cpp:59-65 */
void csdr_noiseproc_destroy(csdr_noiseproc *p);
int csdr_noiseproc_setup(csdr_noiseproc *p, int on, double threshold, double width_us, double sample_rate);
/* n complex doubles in, n out (in == out allowed, as the host calls it: sdrinterface.cpp:884) */
int csdr_noiseproc_process(csdr_noiseproc *p, int n, const double *in_iq, double *out_iq);

/* device-resident batch form: [channels][stride] complex fp32; d_out must not alias d_in */
typedef struct csdr_noiseproc_batch csdr_noiseproc_batch;
csdr_noiseproc_batch *csdr_noiseproc_batch_create(int device, int channels);
void csdr_noiseproc_batch_destroy(csdr_noiseproc_batch *b);
/* channel < 0: every channel */
int csdr_noiseproc_batch_setup(csdr_noiseproc_batch *b, int channel, int on, double threshold, double width_us,
                               double sample_rate);
int csdr_noiseproc_batch_process(csdr_noiseproc_batch *b, const float *d_in, long long in_stride, int n_per_channel,
                                 float *d_out, long long out_stride, void *stream);
/* PROFILE_7 (noiseproc.cpp:127, :159-175): the blanker's own trace m_TestBenchDataBuf of the object's LAST call, the
 * picture a threshold and a width are set from.  That call may be csdr_noiseproc_batch_process or the blanker pass
 * that csdr_demod_batch_process_blanked / _process_packets run on `b`; the trace re-reads its samples and starts from
 * the state and history that call began with (kept untouched until the next call).  Per sample i of receiver c, into
 * d_trace = device [channels][trace_stride] complex fp32:
 *     blanker on:   re = blanked_i ? 0 : (float)(m_MagAveSum_i / m_Ratio)   (the fp64 moving sum after sample i entered
 *                   it, :143-147; one fp64 division, :169), im = (float)((double)o.re + o.im) with o = x[i - delay - 1],
 *                   the delayed sample, blanked or not (:159)
 *     blanker off:  the input sample (:127)
 * A threshold of 0 (m_Ratio = 0) gives IEEE's inf / NaN, as in the reference.
 * Contract, as for the *_blanked display calls: d_in / in_stride / n_per_channel (float rows), or d_packets / npackets
 * / pkt_len with n_per_channel = npackets x samples per datagram (d_in ignored), are those of that last call; same
 * `stream`; before the next call on `b`; no csdr_noiseproc_batch_setup in between.  The object remembers buffer,
 * stride, count and packet length of its last call: CSDR_ESTATE when they differ, when there was no call yet or a
 * set-up since; CSDR_EINVAL for a bad argument (d_trace 16-byte aligned, trace_stride even and >= n_per_channel).  A
 * refused call writes nothing.  An accepted one writes d_trace only -- no state, no history: the next call is what it
 * would have been.
 * Behind csdr_noiseproc_batch_process the trace's sums and decisions are that call's bit for bit (same kernel form,
 * same segments).  Behind a chain's mask pass on arbitrary fp32 rows a decision that ties to the last bit of an fp64
 * sum can differ from the mask (that pass cuts its segments differently); on datagram input every sum is exact and
 * nothing can differ.
 * Out of scope: shard forms, a trace that goes into the scope without rows in between, PROFILE_7 forwarding in the
 * drop-in CNoiseProc. */
int csdr_noiseproc_batch_trace_last(csdr_noiseproc_batch *b, const float *d_in, long long in_stride, const void *d_packets,
                                    int npackets, int pkt_len, int n_per_channel, float *d_trace, long long trace_stride,
                                    void *stream);

/* IQ wire format (interface/netiobase.cpp:479-527): whole UDP datagrams, 4 header bytes then
 * little-endian I,Q pairs; pkt_len 1028 = 256 samples of 16 bit, 1444 = 240 samples of 24 bit
 * (scaled onto the 16-bit range).  d_packets: [channels][npackets][pkt_len] bytes on the device;
 * d_out: [channels][out_stride] complex fp32; d_dc: optional [channels][2] doubles (I, Q offsets,
 * subtracted as CSdrInterface::ProcessIQData does for the display path, sdrinterface.cpp:889-894).
 * d_packets 4-byte aligned, d_out 16-byte aligned, out_stride even.
 * Returns the complex samples written per channel. */
int csdr_ingest_unpack(int device, const void *d_packets, int channels, int npackets, int pkt_len, float *d_out,
                       long long out_stride, const double *d_dc, void *stream);
/* host form of the same conversion: packets in host memory, complex doubles out */
int csdr_ingest_unpack_host(int device, const void *packets, int npackets, int pkt_len, double *out_iq);
/* CSdrInterface::NcoSpurCalibrate (sdrinterface.cpp:829-848): d_dc[ch][0..1] <- running I/Q means
 * (alpha 1e-5) advanced over n more samples of each row of d_iq */
int csdr_ingest_spurcal(int device, const float *d_iq, long long in_stride, int channels, int n, double *d_dc,
                        void *stream);
int csdr_ingest_spurcal_host(int device, int n, const double *in_iq, double *dc_iq);
/* the same over datagrams ([channels][npackets][pkt_len] bytes on the device, the rules of csdr_ingest_unpack), decoded
 * in the kernel's loads: d_dc equals, bit for bit, csdr_ingest_unpack (no DC) followed by csdr_ingest_spurcal */
int csdr_ingest_spurcal_packets(int device, const void *d_packets, int channels, int npackets, int pkt_len, double *d_dc,
                                void *stream);

/* ----------------------------------------------------------------------------------------
 * Batch signal generator: C independent CTestBench generators (gui/testbench.cpp:352-517: swept complex tone, pulse
 * gating, additive Gaussian noise), one per receiver, writing the batch chain's fp32 input rows on the device -- the
 * first step of CSdrInterface::ProcessIQData (sdrinterface.cpp:883), where the generator REPLACES the live IQ.
 *
 * State.  Every receiver has the reference's members: sweep start / stop (Hz), sweep rate (Hz/s), pulse width /
 * period (s), signal / noise power (dB; amplitude 32767 * 10^(dB/20)), on/off, generator sample rate.  Defaults as the
 * constructor's (:90-121): off, width 0.01 s, period 0.5 s, sample rate 1; the members the constructor leaves to the
 * GUI start as: start = stop = 0 Hz, rate 0 Hz/s, signal 0 dB, noise -160 dB.  Each setter has exactly the state
 * effect of its slot: set_sweep_start (:225-230) and set_sweep_stop (:232-237) put the frequency back to start and
 * the phase to 0; set_sweep_rate (:239-244) puts the phase to 0 and the per-sample increment to rate / sample rate
 * (which re-arms a finished sweep for one step); the pulse and power setters (:312-332) change their member only;
 * reset is the generator part of Reset() (:527-532, :575: frequency <- start, phase <- 0, increment <- rate / sample
 * rate, amplitudes, pulse timer <- 0).  channel < 0: every receiver.  All state is on the host: a setter waits for
 * nothing.  Setters and generate of one object exclude each other (one mutex).
 *
 * What is exact.  The frequency sequence f <- fl(f + inc) with its end of sweep (first f >= stop, :424-427) and the
 * pulse timer t <- fl(t + 1/Fs) with its restart (t > period) and gate (off while t > width, :399-406) are the
 * reference's fp64 recurrences bit for bit.  The phase is the exact sum of that frequency sequence over Fs, in turns
 * modulo 1 (128-bit fixed point; the reference's own fp64 accumulator with one fmod per call drifts by about 1.5e-15
 * rad per sample from it in 256-sample calls), and does not depend on how the stream is cut into calls: generate(n)
 * once and generate(n/k) k times write the same words -- complex and real, sweep, pulse and noise alike.
 *
 * Noise (:433-444) keeps Marsaglia's polar method and replaces libc rand() by a counter-based generator, all
 * arithmetic on unsigned 64-bit words modulo 2^64:
 *     mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
 *     key(c)    = mix(seed + 0x9E3779B97F4A7C15 * (c + 1))                    c = receiver index, seed 0 until set_seed
 *     h(c,i,a)  = mix(key(c) + 0x9E3779B97F4A7C15 * (32 * i + a))             a = attempt 0..31
 *     k1 = h >> 33,  k2 = (h >> 2) & 0x7FFFFFFF                               the two 31-bit draws
 *     u1 = 1 - 2 * k1 / 2147483647,  u2 = 1 - 2 * k2 / 2147483647,  r = u1 * u1 + u2 * u2      (fp64, no fused multiply-add)
 * The first attempt with neither r >= 1 nor r == 0 is taken: rad = sqrt(-2 ln(r) / r) in fp64, I += noise amplitude *
 * u1 * rad, Q += noise amplitude * u2 * rad (the real form adds the I term only); 32 rejections in a row (probability
 * 4e-22) add nothing.  i counts the samples the receiver has generated since the object's creation or the last
 * set_seed -- every sample of every call while it is on, with or without noise; a reset does not touch it.  Noise is
 * added only while noise power > -160 dB (:433).  signal + noise is summed in fp64 and rounded to fp32 once.
 *
 * Deliberate deviations: a sample rate different from the last call's resets the receiver BEFORE the call's first
 * sample (the reference queues a Qt signal whose arrival time is undefined, :361-365); own generator instead of rand().
 * Out of scope: a drop-in CTestBench class (it is a QDialog), the USE_FILE playback
 * kludge, a generator that emits datagrams, fusing the generator into the down-converter's loads, a shard form (a
 * shard host makes one generator per device, as for the batch sound sink).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_testgen_batch csdr_testgen_batch;
/* NULL without a HIP device (no CPU fallback) */
csdr_testgen_batch *csdr_testgen_batch_create(int device, int channels);
void csdr_testgen_batch_destroy(csdr_testgen_batch *t);
int csdr_testgen_batch_set_on(csdr_testgen_batch *t, int channel, int on);                        /* OnGenOn :307-310 */
int csdr_testgen_batch_set_sweep_start(csdr_testgen_batch *t, int channel, double hz);            /* OnSweepStart :225-230 */
int csdr_testgen_batch_set_sweep_stop(csdr_testgen_batch *t, int channel, double hz);             /* OnSweepStop :232-237 */
int csdr_testgen_batch_set_sweep_rate(csdr_testgen_batch *t, int channel, double hz_per_s);       /* OnSweepRate :239-244 */
int csdr_testgen_batch_set_pulse_width(csdr_testgen_batch *t, int channel, double seconds);       /* OnPulseWidth :312-315; <= 0: no gating */
int csdr_testgen_batch_set_pulse_period(csdr_testgen_batch *t, int channel, double seconds);      /* OnPulsePeriod :317-320 */
int csdr_testgen_batch_set_signal_power(csdr_testgen_batch *t, int channel, double db);           /* OnSignalPwr :322-326 */
int csdr_testgen_batch_set_noise_power(csdr_testgen_batch *t, int channel, double db);            /* OnNoisePwr :328-332 */
int csdr_testgen_batch_reset(csdr_testgen_batch *t, int channel);                                 /* Reset :527-532, :575 */
/* seed of the noise of every receiver; puts every receiver's sample counter i back to 0 */
int csdr_testgen_batch_set_seed(csdr_testgen_batch *t, unsigned long long seed);
/* CreateGeneratorSamples(int, TYPECPX*, double) (:352-447) of every receiver: n complex fp32 samples into the front of
 * every row of d_iq = device [channels][stride] complex fp32, asynchronous on `stream`.  A receiver whose generator is
 * off leaves its row untouched and its state as it is (:359-360).  d_iq 16-byte aligned, stride even and >= n, n <=
 * 2^30, sample_rate > 0; CSDR_EINVAL before any state changes otherwise.  One launch per call, except that a receiver
 * whose sweep passes more than 8 binades of fp64 inside the call (a sweep through 0 Hz in a very long call) adds
 * launches for the rest.  Queued calls need not be waited for: the words of a launch travel in a ring of 16 pinned
 * buffers, and a call waits (on that launch's event only) when the launch 16 before it has not finished. */
int csdr_testgen_batch_generate(csdr_testgen_batch *t, float *d_iq, long long stride, int n, double sample_rate, void *stream);
/* the TYPEREAL overload (:454-517): 3 * amplitude * cos(phase), the noise's I term; fp32 mono rows, stride a multiple of 4 */
int csdr_testgen_batch_generate_real(csdr_testgen_batch *t, float *d_out, long long stride, int n, double sample_rate,
                                     void *stream);

/* --------------------------------------------------------------------------------------
 * Batch test-bench scope: the time view of CTestBench::DisplayData with ChkForTrigger (gui/testbench.cpp:583-695,
 * :819-898), the oscilloscope that decides which stretch of a tapped stream is looked at, for every receiver of a
 * batch at once and without the rows leaving the device.  Together with the generator above and the stage taps it is
 * the third part of the reference's test bench.
 *
 * Per receiver, each input sample emits zero or more screen pixels: while (double)m_TimeInPos / samplerate >=
 * (double)m_TimeScrnPos * m_TimeScrnPixel (:618-621).  An emission calls ChkForTrigger((int)re), writes (int)re and
 * (int)im (0 in the real form) into the w-entry ring m_TimeBuf1/2 and advances the screen position; at w both
 * positions go back to 0 (:623-632).  ChkForTrigger (:819-898) runs before the pixel is written and keeps
 * m_PreviousSample on every emission: in the triggered modes it waits for the first crossing of the level, counts
 * m_PostScrnCaptureLength = (7*w)/10 further emissions and then copies the ring, oldest entry first, into the screen
 * m_TimeScrnBuf1/2 and emits NewTimeData: the trigger sample sits at screen index w - (7*w)/10.  TRIG_OFF decides at
 * screen position 0 with the skip counter (:823-834) and copies the ring from slot (7*w)/10.  All of it is
 * reproduced bit for bit; the output side is all integers.
 *
 * Settings, per receiver, defaults as the constructor's (:94, :111-117): screen 100 x 100 (one geometry for the
 * object), display rate 10, horizontal span 100 ms, vertical range 65000, trigger level 100, trigger mode 0
 * (0 TRIG_OFF, 1 TRIG_PNORM, 2 TRIG_PSINGLE, 3 TRIG_NNORM, 4 TRIG_NSINGLE), state WAIT, sample rate 1.  Each setter
 * has exactly the state effect of its slot with the time display on; channel < 0: every receiver.  The settings live
 * on the host: a setter waits for nothing, and what it changes -- a reset and the re-arm included -- is applied in
 * stream order by the next put.  m_DisplaySkipValue is a qint32 (gui/testbench.h:174): the quotient is truncated
 * when it is stored, here too.
 *
 * Deliberate deviations.  (1) A sample rate different from the last call's resets the receiver at once and drops the
 * call's samples (:587-592 return without using them; the reference's reset arrives through a queued Qt signal at an
 * undefined time).  As in the reference the first call of a receiver, whose rate differs from the constructor's 1,
 * is such a call.  (2) After a display the trigger state is WAITDISPLAY until the GUI's DrawTimePlot puts it back to
 * WAIT (:995-999); here that hand-back is the explicit call time_plot_done, so a receiver in a triggered mode displays
 * at most once between two hand-backs and nothing depends on thread timing.  TRIG_OFF does not look at the state and
 * may display several times in one call: the screen is the last one, get_emits counts all.  (3) (int) of a sample
 * saturates at the ends of int32 and gives 0 for a NaN (undefined in the reference).  (4) The vertical mapping uses a
 * 64-bit product (the reference's 2*c*v overflows 32 bits for large v), its result saturates to int32, and a
 * vertical range of 0 gives y = h/2 (the reference divides by 0).
 *
 * The FFT view: the frequency branch of DisplayData (:594-611, :654-672), DrawFftPlot (:1005-1068), OnEnablePeak
 * (:334-343) and OnTimeDisplay (:282-286), per receiver.  Deviation (5): a new object is in the TIME view (the
 * constructor's default is m_TimeDisplay = false, :110); set_time_display(s, channel, 0) moves a receiver into the FFT
 * view.  Every put takes each receiver down the branch of its own view.
 *   Frame carry.  Samples are appended to m_FftInBuf at m_FftBufPos, real rows as (x, 0), complex rows as they are
 * (:599, :659-660).  At 2048 (TEST_FFTSIZE) the position returns to 0 (:600-602); then `if (++m_DisplaySkipCounter >=
 * m_DisplaySkipValue)` sets the counter to 0 and the frame is used: PutInDisplayFFT, emit NewFftData (:603-608).  There
 * is no `> 2` clause in this view (that one is TRIG_OFF's).  The counter is the member the time view uses; Reset puts
 * it to -2, so the first complete frame after a reset is never used.
 *   Skip value.  m_DisplaySkipValue = fs / (2048 * m_DisplayRate), truncated into the qint32, computed by Reset (:570)
 * and OnDisplayRate (:257) from the rate known at that moment; set_horz_span only stores the span in this view (:272-273).
 *   Reset (:535-538, :550-557, :570-574): SetFFTParams(2048, FALSE, 0.0, fs) and ResetFFT (the bels go to 0), frame
 * position 0, peak buffer = h for every pixel, m_Span = (qint32)fs, then m_Span - (m_Span + 5) % 10 + 5, skip value as
 * above, counter -2 -- beside the time-view part above, which stays as it is, in either view.  set_time_display stores
 * the view and is a Reset (:282-286).  Deviation (1) holds here too: a call whose rate differs from the last call's
 * resets the receiver and drops that call's samples.
 *   The transform is CFft at 2048 points with SetFFTAve(0) (:128-132), an average size of 1 (dsp/fft.cpp:103-113): the
 * running sum is sum - sum + p, so every used frame stands alone and the bels after a frame depend on that frame only.
 * Window, I/Q swap, K_B, K_C and display order as csdr_fft_batch's (dsp/fft.cpp:267-288, :562-589).
 *   Draw.  Deviation (6): NewFftData is a queued signal and the GUI draws some time later; here every used frame is
 * drawn at once, at the moment it is used (the idealisation time_plot_done makes for the time view).  A draw is
 * GetScreenIntegerFFTData(h, w, m_MaxdB = 10, m_MindB = -170, start, stop) with stop = m_Span / 2 and start = -m_Span /
 * 2 if the put that completed the frame was complex (m_NewDataIsCpx), else 0, in C's integer division (:1026-1043);
 * m_MindB is -170 because DrawFreqOverlay sets m_MaxdB - 18 * m_dBStepSize (:1257) before anything can be drawn, and
 * the reference has no slot that changes either value.  Then peak[i] = min(peak[i], y[i]) for i < w (:1046-1052),
 * whether or not the peak trace is shown; the screen is the last drawn frame's y.  OutBuf[w], which the reference
 * writes in the "more bins than pixels" branch, is dropped.  With these start / stop values every pixel below w
 * receives a bin in both branches, so no pixel is ever left over.
 *   enable_peak (OnEnablePeak): the peak buffer goes back to h and m_TimeBuf1/2 are zeroed -- a receiver in the time
 * view loses its ring, as in the reference; the flag itself is kept and only reported.
 *   An FFT-view receiver needs sample_rate < 2^31 - 16 ((qint32)fs and the + 5): CSDR_EINVAL before any state changes.
 *
 * The int16 overloads (TYPESTEREO16 :761-814, TYPEMONO16 :702-754), the only ones PROFILE_5 reaches.  Stereo: the time
 * view triggers on (int)re and the ring gets re and im; the FFT view takes (re, im), mapped as complex.  Mono: the FFT
 * frame entry is (x, x), BOTH parts (:718-719), m_NewDataIsCpx is false and the screen starts at 0 Hz; in the time view
 * the ring gets pBuf[i] and 0, but ChkForTrigger and m_PreviousSample see pBuf[i<<1] (:741).  Deviation (7): index 2i
 * counts inside the call's n[c] samples, and for 2i >= n[c] the trigger sample is 0 (the reference reads past its
 * buffer there).  Deviations (1)-(6) hold.
 *
 * Out of scope: a drop-in CTestBench class (it is a QDialog), an automatic re-arm inside a call, a shard form (a shard host
 * makes one scope per device, as for the batch sound sink), painting and overlays, a setter for the dB range (the
 * reference has none).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_scope_batch csdr_scope_batch;
/* NULL without a HIP device (no CPU fallback); channels 1..4096 */
csdr_scope_batch *csdr_scope_batch_create(int device, int channels);
void csdr_scope_batch_destroy(csdr_scope_batch *s);
/* resizeEvent (:920-932): 1 <= w <= 2048 (TB_MAX_SCREENSIZE), h >= 2; a Reset() of every receiver */
int csdr_scope_batch_set_screen(csdr_scope_batch *s, int w, int h);
int csdr_scope_batch_set_horz_span(csdr_scope_batch *s, int channel, int ms);          /* OnHorzSpan :270-280: pixel time and skip value, no reset; ms >= 1 */
int csdr_scope_batch_set_display_rate(csdr_scope_batch *s, int channel, int rate);     /* OnDisplayRate :247-254; rate >= 1 */
int csdr_scope_batch_set_trigger_mode(csdr_scope_batch *s, int channel, int mode);     /* OnTriggerMode :288-292: a Reset() */
int csdr_scope_batch_set_trig_level(csdr_scope_batch *s, int channel, int level);      /* OnTrigLevel :294-299 */
int csdr_scope_batch_set_vert_range(csdr_scope_batch *s, int channel, int range);      /* OnVertRange :261-268 */
/* the time-view part of Reset() (:541-548, :555-565, :574): pixel time, positions and previous sample 0, state WAIT,
 * ring cleared, skip value, skip counter -2; the screen keeps its contents */
int csdr_scope_batch_reset(csdr_scope_batch *s, int channel);
/* DisplayData(int, TYPEREAL*, double, int) (:643-695) of every receiver: d_rows = device [channels][stride] fp32, the
 * rows csdr_demod_batch_process writes and the taps hand out; n[c] samples of row c (host array, 0 <= n[c] <= 2^24 and
 * <= stride; 0: the receiver is left exactly as it is), sample_rate[c] > 0 (host array).  Only enqueues on `stream`
 * and waits for nothing (the settings of a call travel in a ring of 16 pinned buffers; a call waits, on that launch's
 * event only, when the launch 16 before it has not finished); the rows are never written; where a sweep is longer
 * than the screen only the emitted samples are read.  One launch per call.  A sweep (span * sample rate) of more than
 * 2^30 samples is CSDR_EINVAL (m_TimeInPos is an int), before any state changes. */
int csdr_scope_batch_put_real(csdr_scope_batch *s, const float *d_rows, long long stride, const int *n,
                              const double *sample_rate, void *stream);
/* the TYPECPX overload (:583-636): rows of complex fp32, stride in complex samples; the trigger looks at re */
int csdr_scope_batch_put_cpx(csdr_scope_batch *s, const float *d_rows, long long stride, const int *n,
                             const double *sample_rate, void *stream);
/* the TYPEMONO16 overload (:702-754): rows of int16, 2-byte aligned; rules, bounds and ordering as put_real.  The rows
 * may lie in device-mapped host memory (csdr_soundsink_batch_get_tap) */
int csdr_scope_batch_put_mono16(csdr_scope_batch *s, const short *d_rows, long long stride, const int *n,
                                const double *sample_rate, void *stream);
/* the TYPESTEREO16 overload (:761-814): rows of int16 (re, im) pairs, 4-byte aligned, stride in pairs */
int csdr_scope_batch_put_stereo16(csdr_scope_batch *s, const short *d_rows, long long stride, const int *n,
                                  const double *sample_rate, void *stream);
/* DrawTimePlot's re-arm (:995-999): the state goes back to WAIT unless the mode is one of the two single ones;
 * applied in stream order by the next put */
int csdr_scope_batch_time_plot_done(csdr_scope_batch *s, int channel);
/* NewTimeData (FFT view: NewFftData) emits of every receiver since the last get_emits into h_emits[channels]; waits for the last put only
 * (its event, on a stream of the object's own) */
int csdr_scope_batch_get_emits(csdr_scope_batch *s, int *h_emits);
/* host copy of m_TimeScrnBuf1/2, w entries each; waits as get_emits does */
int csdr_scope_batch_get_screen(csdr_scope_batch *s, int channel, int *re, int *im);
/* the data-dependent state of one receiver: m_TimeInPos, m_TimeScrnPos, m_PreviousSample, m_TrigState, m_TrigCounter,
 * m_TrigBufPos, m_DisplaySkipCounter, emits since creation (modulo 2^32); waits as get_emits does */
int csdr_scope_batch_get_state(csdr_scope_batch *s, int channel, long long *state8);
/* every receiver's last screen into d_out = device [channels][2][out_stride] int32 (re, im; the first w entries of a
 * row, the rest untouched) and, when d_y is not NULL, DrawTimePlot's vertical mapping of both halves (:973-988), y =
 * h/2 - (2*(h/2)*v) / m_VertRange with C's truncating division, into d_y = device [channels][2][vert_stride] int32.
 * Asynchronous on `stream`, behind the puts before it. */
int csdr_scope_batch_get_screens_all(csdr_scope_batch *s, int *d_out, long long out_stride, int *d_y, long long vert_stride,
                                     void *stream);
/* OnTimeDisplay (:282-286): timemode != 0 the time view, 0 the FFT view; a Reset() of the receiver, applied in stream
 * order by the next put.  CSDR_EINVAL, before any state changes, when the receiver's current rate does not fit the view */
int csdr_scope_batch_set_time_display(csdr_scope_batch *s, int channel, int timemode);
/* OnEnablePeak (:334-343): peak buffer back to h, m_TimeBuf1/2 zeroed, in either view; applied by the next put */
int csdr_scope_batch_enable_peak(csdr_scope_batch *s, int channel, int on);
/* host copies of the last drawn frame's y and of m_FftPkBuf, w entries each; returns 1 if that frame was mapped as
 * complex (start = -m_Span / 2), 0 as real, < 0 on error; waits as get_emits does.  Before the first draw the screen is
 * all 0 and the peak all h */
int csdr_scope_batch_get_fft_screen(csdr_scope_batch *s, int channel, int *screen, int *peak);
/* m_pFFTAveBuf of the last used frame: 2048 bels in display order, as csdr_fft_batch_get_ave; 0 after a Reset */
int csdr_scope_batch_get_fft_ave(csdr_scope_batch *s, int channel, float *out2048);
/* m_FftBufPos, m_DisplaySkipCounter, m_DisplaySkipValue, CFft's m_TotalCount since the last Reset; waits as get_emits does */
int csdr_scope_batch_get_fft_state(csdr_scope_batch *s, int channel, long long *state4);
/* every FFT-view receiver's last drawn y and peak buffer into d_out = device [channels][2][out_stride] int32 (screen,
 * peak; the first w entries of a row, the rest untouched; out_stride >= w).  The rows of a receiver in the time view are
 * left untouched.  Asynchronous on `stream`, behind the puts before it. */
int csdr_scope_batch_get_fft_screens_all(csdr_scope_batch *s, int *d_out, long long out_stride, void *stream);

/* ----------------------------------------------------------------------------------------
 * Batch plotter: V views, each one CPlotter's display state (reference gui/plotter.cpp, gui/plotter.h), over the rows of
 * a csdr_fft_batch.  Several views may plot the same row with their own window size, span, dB range and 2D/waterfall
 * split; one launch per draw updates every running view: the waterfall's scroll and new top line, the 2D trace and the
 * overload pen.  The waterfall image stays on the device.
 *
 * Per view, as the reference:
 *   Construction (gui/plotter.cpp:100-114): span 50000, m_MaxdB 0, m_MindB -130, m_dBStepSize 10, 50 percent 2D, not
 * running, size (0, 0), m_ADOverLoad false, one-shot counter 0.  Here also: view v plots row v until set_source.
 *   resizeEvent (:374-389): 2D height = percent * H / 100, waterfall height = (100 - percent) * H / 100 in integer
 * arithmetic, both W wide; the waterfall is black after EVERY resize event, one at the same size included; then
 * DrawOverlay, whose only arithmetic effect is m_MindB = m_MaxdB - VERT_DIVS (14) * m_dBStepSize (:597, plotter.h:16),
 * and only when the overlay pixmap is not null: W > 0 and 2D height > 0.
 *   SetPercent2DScreen (plotter.h:35) stores the percentage and resizes at the widget's size (so it blackens too).
 *   SetSpanFreq, SetMaxdB, SetdBStepSize (plotter.h:41-44) only store; m_MindB follows at the next UpdateOverlay(),
 * which the reference's host calls after each of them (gui/mainwindow.cpp:914-915, 930-933).  A setter without
 * update_overlay leaves m_MindB as it was, here too.
 *   SetADOverload (plotter.h:43) sets the flag and zeroes the one-shot counter; SetRunningState stores the flag, and
 * draw() does nothing for a view that is not running, not even the scroll.
 *   draw() (:408-480): scroll the waterfall down one line (:425); GetScreenIntegerFFTData(255, w, m_MaxdB, m_MindB,
 * -m_Span / 2, m_Span / 2) gives the new top line m_ColorTbl[255 - y] (:429-441) and its return value is the FFT's
 * overload flag; the same call at the 2D height gives the trace (:451-474); the pen is red if m_ADOverLoad or that
 * flag, else green, and in the red branch only `if (counter++ > 10) { counter = 0; m_ADOverLoad = false; }` (:458-468;
 * OVERLOAD_DISPLAY_LIMIT :50) -- a SetADOverload(true) alone shows red for 12 draws.  -m_Span / 2 and m_Span / 2 are
 * integer divisions of a qint32.
 *   The mapping is csdr_fft_batch_get_screen's, bit for bit, for finite bels (dsp/fft.cpp:308-410 with that function's
 * two bound fixes): every pixel of [0, w) is defined by a draw, and a pixel that covers several bins shows the smallest
 * of their levels -- its strongest bin, or, while a stale m_MindB lies above m_MaxdB (a setter without update_overlay, or
 * a view without a 2D pixmap, whose m_MindB never follows), its weakest, as that function does.  Where C leaves a
 * double -> int conversion undefined the value saturates; that includes m_MaxdB == m_MindB, where the gain is infinite.
 *
 * Storage and ordering.  The settings live on the host; a setter touches no device memory and waits for nothing, and
 * what it changed -- a resize's blackening and SetADOverload included -- travels with the next draw in stream order
 * (a ring of 16 pinned parameter slots; a call waits, on that launch's event only, when the launch 16 before it has
 * not finished).  Trace, waterfall ring, pen, one-shot counter and m_ADOverLoad live on the device.  The waterfall is a
 * ring [wf_h][w] of 0xFFRRGGBB with a head row: a draw moves the head and writes one line, a resize resets head and
 * line count, and the readers show black below the lines drawn since -- no image is ever copied or cleared.  resize
 * and set_percent_2d allocate when a view grows (every allocation of a call before any view changes: CSDR_ENOMEM
 * changes nothing); they then wait for the object's launches in flight.  The trace is forgotten (all 0 until the next
 * draw) when the widget's size changes and on every set_percent_2d, where the reference makes a new m_2DPixmap
 * (:378-384); a resize event at the same size keeps it.
 *   view < 0 in a setter: every view.  Refused with CSDR_EINVAL, nothing changed: a view out of range, a negative row,
 * w or h outside [0, 4096] (MAX_SCREENSIZE :48), percent outside [0, 100], step < 1 (m_MaxdB == m_MindB).
 *
 * Out of scope: painting (grid, text, cursors: DrawOverlay's drawing, MakeFrequencyStrs, the mouse), CMeter, a shard
 * form (one plotter batch per device), image encoding, a per-view FFT size or average (properties of the row).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_plotter_batch csdr_plotter_batch;
/* NULL without a HIP device (no CPU fallback); views 1..4096 */
csdr_plotter_batch *csdr_plotter_batch_create(int device, int views);
void csdr_plotter_batch_destroy(csdr_plotter_batch *p);
int csdr_plotter_batch_set_source(csdr_plotter_batch *p, int view, int fft_row);      /* the row of the spectrum batch a view plots */
int csdr_plotter_batch_resize(csdr_plotter_batch *p, int view, int w, int h);         /* resizeEvent :374-389; may allocate and then waits */
int csdr_plotter_batch_set_percent_2d(csdr_plotter_batch *p, int view, int percent);  /* SetPercent2DScreen; may allocate and then waits */
int csdr_plotter_batch_set_span(csdr_plotter_batch *p, int view, int span_hz);        /* SetSpanFreq */
int csdr_plotter_batch_set_max_db(csdr_plotter_batch *p, int view, int max_db);       /* SetMaxdB */
int csdr_plotter_batch_set_db_step(csdr_plotter_batch *p, int view, int step);        /* SetdBStepSize; step >= 1 */
int csdr_plotter_batch_update_overlay(csdr_plotter_batch *p, int view);               /* DrawOverlay's m_MindB :597 */
int csdr_plotter_batch_set_ad_overload(csdr_plotter_batch *p, int view, int on);      /* SetADOverload; applied by the next draw, running or not */
int csdr_plotter_batch_set_running(csdr_plotter_batch *p, int view, int on);          /* SetRunningState */
/* CPlotter::draw of every running view, one launch on `stream`: reads f's size, sample rate, invert flag, averaged bels
 * and overload words as they are at the call, in stream order behind the puts issued on `stream`; neither uses nor
 * disturbs the translate table csdr_fft_batch_get_screen caches in f.  Returns the number of views drawn: the running
 * ones with w > 0 (a running view with w == 0 takes the pen step, draws nothing and is not counted; wf_h == 0: a trace
 * only; 2D height 0: a waterfall only, the trace all 0).  CSDR_EINVAL, nothing changed: f NULL or on another device, a running view whose row is >= f's
 * channels. */
int csdr_plotter_batch_draw(csdr_plotter_batch *p, csdr_fft_batch *f, void *stream);
/* csdr_plotter_batch_draw of the running views whose row emitted in f's last put call (csdr_fft_batch_get_emits > 0):
 * every other view is left alone -- it does not scroll, keeps its trace and takes no pen step, and a pending
 * set_ad_overload stays pending.  Returns the views drawn, as above. */
int csdr_plotter_batch_draw_emitted(csdr_plotter_batch *p, csdr_fft_batch *f, void *stream);
/* host readers: wait for the object's last call only (its event, on a stream of the object's own).
 * get_trace: the last draw's w levels into out_y and its pen into pen_red (1 red, 0 green; may be NULL); all 0 before
 * the first draw since the size changed; returns w.  get_waterfall: the image [wf_h][w], newest line first, black below the lines
 * drawn since the last resize; returns wf_h. */
int csdr_plotter_batch_get_trace(csdr_plotter_batch *p, int view, int *out_y, int *pen_red);
int csdr_plotter_batch_get_waterfall(csdr_plotter_batch *p, int view, unsigned int *out_rgb);
/* w, 2D height, waterfall height and m_MindB of a view (any pointer may be NULL); host state, waits for nothing */
int csdr_plotter_batch_get_geometry(csdr_plotter_batch *p, int view, int *w, int *h2d, int *wf_h, int *min_db);
/* device readers, asynchronous on `stream` behind the object's calls before them; a later draw waits for them.
 * get_traces_all: view v's trace into d_y[v * stride ...] (the first w entries, the rest untouched) and its pen into
 * d_pen[v] (may be NULL).  get_lines_all: each view's newest waterfall line into d_rgb[v * stride ...], black before
 * the first draw since a resize, untouched for a view without a waterfall.  stride >= the widest view.
 * get_waterfall_dev: one view's image unrolled into d_rgb [wf_h][w], row pitch w, as get_waterfall; returns wf_h. */
int csdr_plotter_batch_get_traces_all(csdr_plotter_batch *p, int *d_y, long long stride, int *d_pen, void *stream);
int csdr_plotter_batch_get_lines_all(csdr_plotter_batch *p, unsigned int *d_rgb, long long stride, void *stream);
int csdr_plotter_batch_get_waterfall_dev(csdr_plotter_batch *p, int view, unsigned int *d_rgb, void *stream);

/* --------------------------------------------------------------------------------------
 * Datagram sequence check: C independent copies of the packet bookkeeping of CUdpThread::OnreadyRead (reference
 * interface/netiobase.cpp:484-496 for 24 bit, :509-521 for 16 bit: the same text), one per receiver, advanced over the
 * datagrams of one call in one launch.  The buffer is the one csdr_demod_batch_process_packets reads -- [channels]
 * [npackets][pkt_len] bytes as they arrived -- so one upload serves both calls on one stream; bytes 2-3 of each
 * datagram, little endian, are its sequence number, and nothing else of the datagram is read.
 *
 * The rule, per receiver: `last` is m_LastSeqNum, a quint16 that starts at 0 (:433); `missed` is
 * CNetIOBase::m_MissedPackets (the GUI's status line, gui/mainwindow.cpp:760), held in 64 bits.  For each datagram in
 * order:
 *     if (seq == 0) last = 0;
 *     if (seq != last) { missed += (int)(qint16)seq - (int)(qint16)last; last = seq; }
 *     last = (last + 1) & 0xffff; if (last == 0) last = 1;
 * with the qint16 casts kept: one datagram lost across 0x7fff/0x8000 moves the count by -65535, a duplicate or a late
 * datagram moves it down.  Two more results of the same test seq != last, which the signed sum hides: `events`, the
 * number of datagrams that failed it (accumulates like missed; a swap adds +k and -k to missed and 2 or 3 here), and
 * `first_gap`, the index within the LAST put of its first such datagram, or -1 (also before the first put).
 *
 * Ordering.  put is asynchronous on `stream`; the state lives on the device.  clear and reset take effect between the
 * puts issued before and after them: a small launch on a stream of the object's own, ordered behind the last call by its
 * event, and the next put waits for that event on its stream -- no host wait, no device-wide one.  get waits for the
 * object's last call only; get_all is asynchronous on `stream` behind it, and a later put waits for it.
 *   Refused with CSDR_EINVAL before any state changes: pkt_len other than 1028 or 1444, d_packets NULL or not 4-byte
 * aligned, npackets < 0, a receiver's npackets * pkt_len at or above 2 GiB (offsets are 32 bit), a channel out of range.
 * npackets == 0 returns 0 and changes nothing, first_gap included.
 *
 * Out of scope: repairing, reordering or dropping anything (the reference only counts); header bytes 0-1 (the
 * reference tells the formats apart by the datagram's size alone); a shard form (one object per device).
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_seqcheck_batch csdr_seqcheck_batch;
/* NULL without a HIP device (no CPU fallback); channels >= 1 */
csdr_seqcheck_batch *csdr_seqcheck_batch_create(int device, int channels);
void csdr_seqcheck_batch_destroy(csdr_seqcheck_batch *s);
int csdr_seqcheck_batch_put(csdr_seqcheck_batch *s, const void *d_packets, int npackets, int pkt_len, void *stream);
int csdr_seqcheck_batch_clear(csdr_seqcheck_batch *s, int channel);   /* missed, events <- 0; last kept (mainwindow.cpp:703); channel < 0: all */
int csdr_seqcheck_batch_reset(csdr_seqcheck_batch *s, int channel);   /* and last <- 0 (netiobase.cpp:433) */
/* one receiver's record to the host (any pointer may be NULL) */
int csdr_seqcheck_batch_get(csdr_seqcheck_batch *s, int channel, long long *missed, long long *events, int *first_gap, int *last);
/* every receiver's into device arrays [channels] of the caller's (any may be NULL) */
int csdr_seqcheck_batch_get_all(csdr_seqcheck_batch *s, long long *d_missed, long long *d_events, int *d_first_gap, void *stream);

/* --------------------------------------------------------------------------------------
 * Batch NCO-spur calibration: C independent copies of CSdrInterface's NCO-spur state (reference
 * interface/sdrinterface.cpp:791-824 ManageNCOSpurOffsets, :829-848 NcoSpurCalibrate, :886-887 its call behind the
 * in-place blanker of :884), one per receiver, held on the device.  Per receiver: m_NCOSpurOffsetI / Q (doubles, 0
 * at create), m_NcoSpurCalCount and m_NcoSpurCalActive (0, false).  The offsets lie in a [channels][2] array of doubles,
 * csdr_spurcal_batch_dc(): the d_dc of csdr_ingest_unpack and of the four csdr_fft_batch_put_display_* calls.
 *
 * Commands (:791-824).  Every one first clears `active` (:793) -- a read too, which so stops a running calibration, as in
 * the reference.  channel -1 addresses every receiver (set, start_cal).
 *   set(i, q)   NCOSPUR_CMD_SET (:796-803).  StartSdr's NetSDR branch (:566-568) is set(0, 0).
 *   start_cal   NCOSPUR_CMD_STARTCAL (:804-812): an offset > 10.0 or < -10.0 becomes 0, each on its own; count = 0;
 *               active = true.  StartSdr's SDR-14 / SDR-IQ branch (:587) is start_cal.
 *   read        NCOSPUR_CMD_READ (:813-820): the offsets.
 *   get_state   no command of the reference's: offsets, count and active as they are, nothing touched (status lines, tests).
 *
 * Puts.  One reference call is one datagram (interface/netiobase.cpp:583, :593: 480 or 512 doubles).  On an active
 * receiver with count < SPUR_CAL_MAXSAMPLES (300000) the recurrence offset = (1 - 1/100000) offset + (1/100000) x runs
 * over the whole datagram (:833-840) and count += Length / 4 (:841: 120 or 128); on an active one with count >= 300000
 * the datagram clears `active` and nothing else (:843-847); an inactive receiver's offsets do not change by a bit.  So a
 * put of npackets datagrams on a receiver that arrives active with count c0 < 300000 runs the recurrence over the first
 * u = min(npackets, ceil((300000 - c0) / q)) datagrams, q = samples per datagram / 2; count = c0 + u q; active ends
 * false exactly when u < npackets (a put that ends on the limit leaves it true until the next datagram arrives).
 * 24 bit from 0: u = 2500, count 300000.  16 bit: u = 2344, count 300032.
 *   put_packets          the datagrams, decoded in the load
 *   put_stream           fp32 rows; call_len is the reference call's length in complex samples (call k covers samples
 *                        [k call_len, ...); a short last call of r samples adds (2 r) / 4 to count)
 *   put_packets_blanked  what the blanker of b's last blanked chain call handed over (:884), from that call's mask
 *   put_stream_blanked   the same on rows
 * The blanked pair has the sample rule, the contract and the refusals of csdr_fft_batch_put_display_*_blanked: right
 * behind that chain call, same stream, same buffer / count / packet length or stride, before the next call on b, same
 * width and device, strict or pipelined; CSDR_ESTATE / CSDR_EINVAL otherwise, nothing changed.  Datagram forms: pkt_len
 * 1028 or 1444, 4-byte aligned, below 2 GiB per channel; rows 8-byte aligned, in_stride >= n, call_len >= 1.  A put with
 * a count of 0 is legal.  The same samples give the same doubles whichever of the four forms delivered them.
 *
 * Ordering.  Puts are asynchronous on `stream`; commands are small launches on a stream of the object's own.  Each is
 * ordered behind the object's call before it by an event, so commands and puts take effect in the order they were issued
 * whatever their streams, and commands issued between two puts apply, in order, before the later put's first datagram
 * (set(50, -3) then start_cal leaves I = 0, Q = -3, active).  The host waits in read and get_state only.  A display or
 * unpack call that must see a command's offsets goes behind a put on its stream -- an empty one (count 0) will do: it
 * only puts what was commanded in front of that stream.
 *
 * Out of scope: per-datagram offsets in the display -- a display call subtracts the offsets as they stand after the put
 * from all of the put's samples, where the reference subtracts them as they stand at each datagram (the display stream
 * with csdr_ingest_spurcal* works the same way); m_Running; shard forms; the limit as a parameter.
 * -------------------------------------------------------------------------------------- */
typedef struct csdr_spurcal_batch csdr_spurcal_batch;
/* NULL without a HIP device (no CPU fallback); channels >= 1 */
csdr_spurcal_batch *csdr_spurcal_batch_create(int device, int channels);
void csdr_spurcal_batch_destroy(csdr_spurcal_batch *s);
int csdr_spurcal_batch_set(csdr_spurcal_batch *s, int channel, double offset_i, double offset_q);   /* :796-803 */
int csdr_spurcal_batch_start_cal(csdr_spurcal_batch *s, int channel);                                /* :804-812 */
int csdr_spurcal_batch_read(csdr_spurcal_batch *s, int channel, double *offset_i, double *offset_q); /* :813-820, :793 */
int csdr_spurcal_batch_get_state(csdr_spurcal_batch *s, int channel, double *offset_i, double *offset_q, int *count, int *active);
/* the offsets on the device, [channels][2] doubles (I, Q); valid until destroy; NULL for a NULL handle */
const double *csdr_spurcal_batch_dc(csdr_spurcal_batch *s);
/* :886-887 with :829-848 over the datagrams / rows of one call, every receiver */
int csdr_spurcal_batch_put_packets(csdr_spurcal_batch *s, const void *d_packets, int npackets, int pkt_len, void *stream);
int csdr_spurcal_batch_put_stream(csdr_spurcal_batch *s, const float *d_in, long long in_stride, int n, int call_len, void *stream);
/* ... behind :884 */
int csdr_spurcal_batch_put_packets_blanked(csdr_spurcal_batch *s, csdr_demod_batch *b, const void *d_packets, int npackets,
                                           int pkt_len, void *stream);
int csdr_spurcal_batch_put_stream_blanked(csdr_spurcal_batch *s, csdr_demod_batch *b, const float *d_in, long long in_stride,
                                          int n, int call_len, void *stream);

#ifdef __cplusplus
}
#endif
#endif
