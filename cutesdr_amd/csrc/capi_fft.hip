// capi_fft.hip -- C ABI for CFft (dsp/fft.h:24-85): display spectrum + plain transforms.
#include "capi_common.hpp"
#include "spectrum_kernels.h"
#include "display_stream_kernels.h"
#include "fft_batch_plain64_kernels.h"
#include "fft_tw64_host.hpp"
#include "display_plan.hpp"
#include "downconv_kernels.h"
#include "capi_internal.hpp"
#include "host_math.hpp"
#include <cstdint>
#include <cstring>
#include <vector>

using namespace csdr;

struct csdr_fft_batch {
    int device, channels;
    int size, last_size, ave_size, invert;       // m_FFTSize, m_LastFFTSize, m_AveSize, m_Invert
    double kc, kb, db_comp, fs;
    // screen mapping state (GetScreenIntegerFFTData)
    int start_hz, stop_hz, bin_min, bin_max, plot_w;
    std::vector<int> xlat;
    float *d_win, *d_tw1, *d_tw2, *d_sum, *d_pwr, *d_ave;
    float *d_work;                               // transform work space of the multi-launch sizes
    float *d_part = nullptr; size_t part_cap = 0; // frame-group partial sums
    int *d_cnt, *d_over;
    int *d_scr = nullptr; size_t scr_cap = 0;           // levels of a waterfall line (csdr_fft_batch_get_waterfall_all)
    std::vector<float> h_ave;
    std::vector<int> h_over;
    // the readers (GetScreenIntegerFFTData from the GUI thread, fft.cpp:308-410) wait for THIS object's last
    // PutInDisplayFFT only -- the copy rides on that call's stream -- not for whatever else the device is running
    hipStream_t last_stream = nullptr; bool have_stream = false;
    // the display stream of ProcessIQData (sdrinterface.cpp:889-907): frame position, skip counter and gate, one set for
    // every channel (each call brings the same samples to every row); the partial frame itself stays on the device
    DisplayState ds;
    double disp_fs = 0; int disp_rate = 0;       // m_SampleRate and m_MaxDisplayRate (set_params re-derives the skip value)
    float *d_carry = nullptr;                    // [channels][N] complex: m_DataBuf of each channel, DC-corrected
    float *d_stage = nullptr; size_t stage_cap = 0;   // [channels][used frames][N] complex: the frames a call uses
    // the batch form of FwdFFT / RevFFT at 32768 and 65536 points (csdr_fft_batch_fwd / _rev): the four-step form's
    // tables and its intermediate, plain_group frames of every row; display calls never touch them
    float *d_twp = nullptr, *d_pwork = nullptr;
    int plain_group = 0;
    // their fp64 form (csdr_fft_batch_fwd_f64 / _rev_f64): the table and, at the four-step sizes, the intermediate of
    // plain_group64 frames of every row, for the object's present size.  Built by csdr_fft_batch_prepare_f64 or the
    // first fp64 call, dropped by set_params: an object that never asks for fp64 holds none of it
    double *d_tw64 = nullptr, *d_work64 = nullptr;
    int plain_group64 = 0;
    bool ready64 = false;
    // the row form: averaging length (rows_ave) and skip value, counter, gate and ready (rows_disp) per row; the frame
    // position ds.pos and the carry stay one per object.  While a flag is clear, its rows follow ave_size / ds (copied in
    // front of a row-form put).  rate_r: each row's m_MaxDisplayRate, for set_params.
    bool rows_ave = false, rows_disp = false;
    std::vector<DisplayState> rs, rs_next;
    std::vector<int> ave_r, rate_r;
    // the frames each row used in the last put (a uniform put fills it with its count)
    std::vector<int> emits, emits_next;
    // the active-row tables of a row-form put travel as the plotter's parameters do (capi_plotter.hip): a ring of pinned
    // slots, [2][channels] entries each (gathered launch, loaded launch), copied on the caller's stream
    static constexpr int kTabRing = 16;
    SpecRow *h_tab[kTabRing] = {}, *d_tab[kTabRing] = {};
    hipEvent_t tab_ev[kTabRing] = {};
    bool tab_busy[kTabRing] = {};
    int tab_next = 0;
};
static bool fft_row_form(const csdr_fft_batch *f) { return f->rows_ave || f->rows_disp; }

// device -> host behind the object's own work: on the stream of its last put_display (until round 5: hipDeviceSynchronize)
static int fft_read(csdr_fft_batch *f, void *dst, const void *src, size_t bytes)
{
    if (!f->have_stream) { CSDR_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return CSDR_OK; }
    CSDR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, f->last_stream));
    CSDR_HIP(hipStreamSynchronize(f->last_stream));
    return CSDR_OK;
}

// a device buffer that only grows, to at least `need` elements: the stream's work on the old one ends before it goes
template <class E>
static hipError_t fft_grow(E *&buf, size_t &cap, size_t need, hipStream_t st)
{
    if (need <= cap) return hipSuccess;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (buf) (void)hipFree(buf);
    buf = nullptr; cap = 0;
    e = hipMalloc((void **)&buf, need * sizeof(E));
    if (e == hipSuccess) cap = need;
    return e;
}

static void fft_free_dev(csdr_fft_batch *f)
{
    float **ps[] = {&f->d_win, &f->d_tw1, &f->d_tw2, &f->d_sum, &f->d_pwr, &f->d_ave, &f->d_work, &f->d_carry, &f->d_twp, &f->d_pwork};
    for (auto p : ps) { if (*p) (void)hipFree(*p); *p = nullptr; }
}

static void fft64_drop(csdr_fft_batch *f)
{
    if (f->d_tw64) (void)hipFree(f->d_tw64);
    if (f->d_work64) (void)hipFree(f->d_work64);
    f->d_tw64 = f->d_work64 = nullptr;
    f->plain_group64 = 0; f->ready64 = false;
}

static int fft_reset(csdr_fft_batch *f)
{   // CFft::ResetFFT (fft.cpp:248-259): clears the averaged and summed buffers and both counters
    const size_t nb = (size_t)f->channels * f->size * 4;
    CSDR_HIP(hipMemset(f->d_ave, 0, nb));
    CSDR_HIP(hipMemset(f->d_sum, 0, nb));
    CSDR_HIP(hipMemset(f->d_cnt, 0, sizeof(int) * 2 * f->channels));
    return CSDR_OK;
}

// one row's part of ResetFFT
static int fft_reset_row(csdr_fft_batch *f, int row)
{
    const size_t nb = (size_t)f->size * 4;
    CSDR_HIP(hipMemset(f->d_ave + (size_t)row * f->size, 0, nb));
    CSDR_HIP(hipMemset(f->d_sum + (size_t)row * f->size, 0, nb));
    CSDR_HIP(hipMemset(f->d_cnt + 2 * row, 0, sizeof(int) * 2));
    return CSDR_OK;
}

// into the row form: the table ring on first use, and the rows of a still-uniform half take the object's values
static int fft_rows_enter(csdr_fft_batch *f, bool ave, bool disp)
{
    if (!f->h_tab[0]) {
        if (!device_ok(f->device)) return CSDR_EHIP;
        const size_t bytes = sizeof(SpecRow) * 2 * (size_t)f->channels;
        for (int i = 0; i < csdr_fft_batch::kTabRing; i++) {
            if (!f->h_tab[i] && hipHostMalloc((void **)&f->h_tab[i], bytes, hipHostMallocDefault) != hipSuccess)
                return fail(CSDR_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
            if (!f->d_tab[i]) CSDR_HIP(hipMalloc((void **)&f->d_tab[i], bytes));
            if (!f->tab_ev[i]) CSDR_HIP(hipEventCreateWithFlags(&f->tab_ev[i], hipEventDisableTiming));
        }
    }
    if (ave && !f->rows_ave) { f->ave_r.assign((size_t)f->channels, f->ave_size); f->rows_ave = true; }
    if (disp && !f->rows_disp) {
        f->rs.assign((size_t)f->channels, f->ds);
        f->rate_r.assign((size_t)f->channels, f->disp_rate);
        f->rows_disp = true;
    }
    return CSDR_OK;
}
// One put's slot of the table ring: acquire() waits, on that put's event only, when the put kTabRing before has not
// finished; send() copies the first n entries of a table behind the stream's work.  A slot that something was sent from
// is marked busy behind the stream when the put leaves, by whichever return: its copies may be in flight after an error
// too, and the ring moves on only past a used slot.
struct TabSlot {
    csdr_fft_batch *f; hipStream_t st; int slot; bool sent = false;
    TabSlot(csdr_fft_batch *f_, hipStream_t st_) : f(f_), st(st_), slot(f_->tab_next) {}
    TabSlot(const TabSlot &) = delete;
    SpecRow *host(int table = 0) const { return f->h_tab[slot] + (size_t)table * f->channels; }
    SpecRow *dev(int table = 0) const { return f->d_tab[slot] + (size_t)table * f->channels; }
    int acquire()
    {
        if (f->tab_busy[slot]) { CSDR_HIP(hipEventSynchronize(f->tab_ev[slot])); f->tab_busy[slot] = false; }
        return CSDR_OK;
    }
    hipError_t send(int table, int n)
    {
        sent = true;
        return hipMemcpyAsync(dev(table), host(table), sizeof(SpecRow) * (size_t)n, hipMemcpyHostToDevice, st);
    }
    int done()                           // the put's last use of the slot is on the stream
    {
        if (!sent) return CSDR_OK;
        sent = false;
        f->tab_next = (slot + 1) % csdr_fft_batch::kTabRing;
        CSDR_HIP(hipEventRecord(f->tab_ev[slot], st));
        f->tab_busy[slot] = true;
        return CSDR_OK;
    }
    ~TabSlot() { (void)done(); }         // (an error return)
};
// row < 0: every row (the plotter's view < 0); [lo, hi) or CSDR_EINVAL with nothing changed
static int fft_row_range(csdr_fft_batch *f, int row, int *lo, int *hi)
{
    if (!f) return have_device() ? fail(CSDR_EINVAL, "bad handle") : CSDR_EHIP;      // (an object has a device)
    if (row >= f->channels) return fail(CSDR_EINVAL, "row %d of %d", row, f->channels);
    *lo = row < 0 ? 0 : row; *hi = row < 0 ? f->channels : row + 1;
    return CSDR_OK;
}

static int fft_set_params(csdr_fft_batch *f, int size, int invert, double db_comp, double fs)
{   // CFft::SetFFTParams (fft.cpp:118-243)
    if (size == 0) return CSDR_OK;
    fft64_drop(f);
    f->bin_min = f->bin_max = 0; f->start_hz = f->stop_hz = 0; f->plot_w = 0;
    f->invert = invert; f->fs = fs;
    if (f->db_comp != db_comp) { f->last_size = 0; f->db_comp = db_comp; }
    int n = size < 512 ? 512 : (size > 65536 ? 65536 : size);
    const int l2 = log2_of(n);
    if (l2 < 0) return fail(CSDR_EINVAL, "FFT size %d is not a power of two", n);
    f->size = n;
    if (f->last_size != n) {
        f->last_size = n;
        fft_free_dev(f);
        const size_t nb = (size_t)f->channels * n * 4;
        CSDR_HIP(hipMalloc((void **)&f->d_win, (size_t)n * 4));
        CSDR_HIP(hipMalloc((void **)&f->d_tw1, 8192));
        CSDR_HIP(hipMalloc((void **)&f->d_tw2, 8192));
        CSDR_HIP(hipMalloc((void **)&f->d_sum, nb));
        CSDR_HIP(hipMalloc((void **)&f->d_pwr, nb));
        CSDR_HIP(hipMalloc((void **)&f->d_ave, nb));
        CSDR_HIP(hipMalloc((void **)&f->d_carry, nb * 2));
        if (!spectrum_single_launch(l2)) CSDR_HIP(hipMalloc((void **)&f->d_work, nb * 4));   // [2][channels][N] complex
        f->plain_group = 0;
        if (l2 > PLAIN_MAX_LOG2N) {
            // the work buffer holds 64 frames (a launch of 512 ... 1024 workgroups), and at least one of every row
            f->plain_group = f->channels < 64 ? 64 / f->channels : 1;
            CSDR_HIP(hipMalloc((void **)&f->d_twp, 512 * 8));
            CSDR_HIP(hipMalloc((void **)&f->d_pwork, nb * 2 * f->plain_group));
            std::vector<float> twp(1024);
            for (int i = 0; i < 256; i++) {
                const double a = kTwoPi * (double)i / 256.0, b = kTwoPi * (double)i / (double)n;
                twp[2 * i] = (float)std::cos(a); twp[2 * i + 1] = (float)std::sin(a);
                twp[512 + 2 * i] = (float)std::cos(b); twp[512 + 2 * i + 1] = (float)std::sin(b);
            }
            CSDR_HIP(hipMemcpy(f->d_twp, twp.data(), 512 * 8, hipMemcpyHostToDevice));
        }
        CSDR_HIP(hipMemset(f->d_pwr, 0, nb));
        f->kb = f->db_comp - 20 * std::log10((double)n * refc::FFT_K_AMPMAX / 2.0);
        f->kc = std::pow(10.0, (refc::FFT_K_MINDB - f->kb) / 10.0);
        f->kb = f->kb / 10.0;
        std::vector<float> win(n), tw1(2048), tw2(2048);
        for (int i = 0; i < n; i++) win[i] = (float)(2.0 * (.5 - .5 * std::cos((kTwoPi * i) / (n - 1))));
        for (int i = 0; i < 1024; i++) {
            const double a = kTwoPi * (double)i / (double)n;
            tw1[2 * i] = (float)std::cos(a); tw1[2 * i + 1] = (float)std::sin(a);
        }
        for (int k = 0; k < 32; k++)
            for (int i = 0; i < 32; i++) {
                const double a = kTwoPi * (double)(i * k) / 1024.0;
                tw2[2 * (k * 32 + i)] = (float)std::cos(a); tw2[2 * (k * 32 + i) + 1] = (float)std::sin(a);
            }
        CSDR_HIP(hipMemcpy(f->d_win, win.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        CSDR_HIP(hipMemcpy(f->d_tw1, tw1.data(), 8192, hipMemcpyHostToDevice));
        CSDR_HIP(hipMemcpy(f->d_tw2, tw2.data(), 8192, hipMemcpyHostToDevice));
        f->xlat.assign(n, 0);
    }
    return fft_reset(f);
}

extern "C" {

csdr_fft_batch *csdr_fft_batch_create(int device, int channels)
{
    if (channels < 1) { fail(CSDR_EINVAL, "channels >= 1"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_fft_batch *f = new csdr_fft_batch();
    f->device = device; f->channels = channels;
    f->size = 1024; f->last_size = 0; f->ave_size = 1; f->invert = 0; f->db_comp = 0.0; f->fs = 1000;
    f->d_win = f->d_tw1 = f->d_tw2 = f->d_sum = f->d_pwr = f->d_ave = f->d_work = nullptr;
    f->d_cnt = nullptr; f->d_over = nullptr;
    f->rs.assign((size_t)channels, f->ds); f->rs_next = f->rs;
    f->ave_r.assign((size_t)channels, 1); f->rate_r.assign((size_t)channels, 0);
    f->emits.assign((size_t)channels, 0); f->emits_next = f->emits;
    if (hipMalloc((void **)&f->d_cnt, sizeof(int) * 2 * channels) != hipSuccess ||
        hipMalloc((void **)&f->d_over, sizeof(int) * channels) != hipSuccess ||
        hipMemset(f->d_over, 0, sizeof(int) * channels) != hipSuccess ||     // (the row form clears a word with the row's frames only)
        fft_set_params(f, 2048, 0, 0.0, 1000) != CSDR_OK) {          // ctor, fft.cpp:41-62
        csdr_fft_batch_destroy(f);
        return nullptr;
    }
    return f;
}
void csdr_fft_batch_destroy(csdr_fft_batch *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    fft_free_dev(f);
    fft64_drop(f);
    if (f->d_cnt) (void)hipFree(f->d_cnt);
    if (f->d_over) (void)hipFree(f->d_over);
    if (f->d_scr) (void)hipFree(f->d_scr);
    if (f->d_part) (void)hipFree(f->d_part);
    if (f->d_stage) (void)hipFree(f->d_stage);
    for (int i = 0; i < csdr_fft_batch::kTabRing; i++) {
        if (f->tab_busy[i]) (void)hipEventSynchronize(f->tab_ev[i]);      // its put still reads the slot
        if (f->tab_ev[i]) (void)hipEventDestroy(f->tab_ev[i]);
        if (f->h_tab[i]) (void)hipHostFree(f->h_tab[i]);
        if (f->d_tab[i]) (void)hipFree(f->d_tab[i]);
    }
    delete f;
}
int csdr_fft_batch_set_params(csdr_fft_batch *f, int size, int invert, double db_comp, double fs)
{
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (!device_ok(f->device)) return CSDR_EHIP;
    const int rc = fft_set_params(f, size, invert, db_comp, fs);
    if (rc) return rc;
    // CSdrInterface::SetFftSize (sdrinterface.cpp:709-718): m_FftBufPos = 0, then SetMaxDisplayRate for the new size at
    // m_SampleRate -- the rate SetFFTParams is given too, so fs here
    f->ds.pos = 0;
    if (fs > 0) f->disp_fs = fs;
    if (f->disp_rate > 0) { f->ds.skip = display_skip_value(f->disp_fs, f->size, f->disp_rate); f->ds.counter = 0; }
    if (f->rows_disp)                                    // every row from ITS stored rate
        for (int r = 0; r < f->channels; r++)
            if (f->rate_r[r] > 0) { f->rs[r].skip = display_skip_value(f->disp_fs, f->size, f->rate_r[r]); f->rs[r].counter = 0; }
    return CSDR_OK;
}
int csdr_fft_batch_set_ave(csdr_fft_batch *f, int ave)
{   // CFft::SetFFTAve (fft.cpp:103-113); every row, and the averaging half of the row form ends
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (!device_ok(f->device)) return CSDR_EHIP;
    if (f->ave_size != ave) f->ave_size = ave > 0 ? ave : 1;
    f->rows_ave = false;
    return fft_reset(f);
}
int csdr_fft_batch_set_ave_row(csdr_fft_batch *f, int row, int ave)
{   // CFft::SetFFTAve of one row: its length, then ResetFFT of that row alone
    int lo, hi;
    if (int rc = fft_row_range(f, row, &lo, &hi)) return rc;
    if (!device_ok(f->device)) return CSDR_EHIP;
    if (int rc = fft_rows_enter(f, true, false)) return rc;
    for (int r = lo; r < hi; r++) {
        f->ave_r[r] = ave > 0 ? ave : 1;
        if (int rc = fft_reset_row(f, r)) return rc;
    }
    return CSDR_OK;
}
int csdr_fft_batch_reset_row(csdr_fft_batch *f, int row)
{
    int lo, hi;
    if (int rc = fft_row_range(f, row, &lo, &hi)) return rc;
    if (!device_ok(f->device)) return CSDR_EHIP;
    for (int r = lo; r < hi; r++)
        if (int rc = fft_reset_row(f, r)) return rc;
    return CSDR_OK;
}
int csdr_fft_batch_row_form(csdr_fft_batch *f) { return f ? (int)fft_row_form(f) : fail(CSDR_EINVAL, "bad handle"); }
int csdr_fft_batch_get_emits(csdr_fft_batch *f, int *out)
{   // host state only: the frames each row used in the last put
    if (!f || !out) return fail(CSDR_EINVAL, "bad argument");
    std::copy(f->emits.begin(), f->emits.end(), out);
    return CSDR_OK;
}
int csdr_fft_batch_reset(csdr_fft_batch *f)
{
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (!device_ok(f->device)) return CSDR_EHIP;
    return fft_reset(f);
}
int csdr_fft_batch_size(csdr_fft_batch *f) { return f ? f->size : fail(CSDR_EINVAL, "bad handle"); }

// where the frames of a display-stream launch come from (spectrum_stream_launch, 2048 ... 8192 points): frame f at
// sample start + f step of the call, DC subtracted, from fp32 rows or from datagrams (pk); blank: behind a blanked chain
// call, through the blanked loaders
struct FrameSrc {
    long long start, step;
    const double *dc;
    const unsigned char *pk; long pk_stride; int pkt_len;
    const DcBlank *blank;
};

// PutInDisplayFFT of nframes frames of `size` samples per channel, back to back in each row (src == nullptr), or as src
// says; asynchronous.  nframes >= 1.  The overload flag is the last put frame's (m_Overload = FALSE at the top of every
// PutInDisplayFFT, fft.cpp:270): every launch clears the words and its kernels set them for its last frame alone, so
// of the launches of one stream call the one that holds the last used frame decides.
// The row form (rows): the launch's table of active rows, nframes the largest frame count among them; each row's
// frames, averaging length, start and step are its entry's, and the launch clears the overload words of ITS rows.
struct RowTable { const SpecRow *dev, *host; int n; };
static int fft_put_frames(csdr_fft_batch *f, const float *d_in, long long in_stride, int nframes, void *stream,
                          const FrameSrc *src = nullptr, const RowTable *rows = nullptr)
{
    f->last_stream = (hipStream_t)stream; f->have_stream = true;
    if (!rows) CSDR_HIP(hipMemsetAsync(f->d_over, 0, sizeof(int) * f->channels, (hipStream_t)stream));
    SpectrumArgs a;
    a.in = d_in; a.in_stride = in_stride; a.win = f->d_win; a.tw1 = f->d_tw1; a.tw2 = f->d_tw2;
    a.sum = f->d_sum; a.pwr = f->d_pwr; a.ave = f->d_ave; a.counters = f->d_cnt; a.overload = f->d_over;
    a.channels = f->channels; a.nframes = nframes; a.ave_size = f->ave_size;
    if (rows) { a.rows = rows->dev; a.nrows = rows->n; }
    const int active = rows ? rows->n : f->channels;       // the channels that get workgroups
    // long calls on few channels: cut each channel's frames into groups so that ONE round of workgroups fills the chip
    a.nparts = 1; a.part = nullptr; a.alpha = nullptr;
    const int l2 = log2_of(f->size);
    const size_t np = (size_t)spectrum_groups(nframes, (spectrum_round_slots(l2) + active - 1) / active);
    if (np > 1) {
        const size_t need = (size_t)f->channels * np * f->size + (size_t)f->channels * (np + 1);   // + the group weights
        CSDR_HIP(fft_grow(f->d_part, f->part_cap, need, (hipStream_t)stream));
        a.nparts = (int)np; a.part = f->d_part;
        a.alpha = f->d_part + (size_t)f->channels * np * f->size;
    }
    a.kc = (float)f->kc; a.kb = f->kb;
    a.frame_start = src ? src->start : 0; a.frame_step = src ? src->step : f->size;
    a.dc = src ? src->dc : nullptr;
    a.pk = src ? src->pk : nullptr; a.pk_stride = src ? src->pk_stride : 0;
    const DcBlank *blank = src ? src->blank : nullptr;
    a.nb_mask = blank ? blank->mask : nullptr; a.nb_mask_stride = blank ? blank->mask_stride : 0;
    a.nb_state = blank ? (const NbChan *)blank->state : nullptr;
    if (src) CSDR_HIP(spectrum_stream_launch(l2, a, src->pkt_len, (hipStream_t)stream));
    else if (spectrum_single_launch(l2)) CSDR_HIP(spectrum_launch(l2, a, (hipStream_t)stream));
    else CSDR_HIP(spectrum_generic_launch(l2, a, f->d_work, (hipStream_t)stream, rows ? rows->host : nullptr));
    return CSDR_OK;
}
/* nframes frames of `size` samples per channel, back to back in each row; asynchronous */
int csdr_fft_batch_put_display(csdr_fft_batch *f, const float *d_in, long long in_stride, int nframes, void *stream)
{
    if (!f || !d_in || nframes < 0) return fail(CSDR_EINVAL, "bad argument");
    if (nframes == 0) return CSDR_OK;
    if (!device_ok(f->device)) return CSDR_EHIP;
    if (!fft_row_form(f)) {
        if (int rc = fft_put_frames(f, d_in, in_stride, nframes, stream)) return rc;
    } else {             // every row nframes frames, each with its own averaging length
        TabSlot slot(f, (hipStream_t)stream);
        if (int rc = slot.acquire()) return rc;
        SpecRow *h = slot.host();
        for (int r = 0; r < f->channels; r++)
            h[r] = SpecRow{r, nframes, f->rows_ave ? f->ave_r[r] : f->ave_size, 0, 0, f->size};
        CSDR_HIP(slot.send(0, f->channels));
        const RowTable tab{slot.dev(), h, f->channels};
        if (int rc = fft_put_frames(f, d_in, in_stride, nframes, stream, nullptr, &tab)) return rc;
        if (int rc = slot.done()) return rc;
    }
    f->emits.assign((size_t)f->channels, nframes);
    return CSDR_OK;
}

/* ---- the display stream (ProcessIQData, sdrinterface.cpp:886-907) ---- */
// n samples of every row (fp32 rows d_in, or the datagrams of `wire`) appended to the stream.  The frames the plan uses
// are read where they lie: at 2048 ... 8192 points by the spectrum kernels' stream loaders (datagrams decoded and DC
// subtracted in the frame load); plain fp32 rows without DC whose used frames lie back to back, at every size, by the
// plain launch in place.  The rest is gathered, DC-corrected, into the staging rows first: the frame that begins in the
// carried partial frame, and at the other sizes (16384, where the stream loaders spill, and the multi-launch sizes) every
// used frame.  The partial frame at the end stays in d_carry.
// blank: the call's samples as the blanker of the chain call that consumed them handed them over (StreamSrc in
// display_stream_kernels.h).  The blanked loaders (2048 and 4096 points; at 8192 they spilled) read no history: the choice
// here is that a frame whose delayed samples may reach in front of the call -- first sample below the largest
// delay_n + 1, NB_MAX_WIDTH / 2 + 1 -- is gathered like the frame that begins in the carry (with step >= N >= 2048
// that is at most the first two used frames of a call), instead of teaching the loaders the history branch.
// The row form of a stream call: display_rows_plan over the rows' states and the shared position, then at most two
// launches, each over its table of active rows: the gathered frames (the frame that begins in the carry; every frame at
// 16384 points, at the multi-launch sizes and behind a blanker), then the frames the stream loaders read where they lie,
// with each row's start and step.  A row that uses no frame is in neither table: nothing of it is read or written.
// the call's samples in front of the carried partial frame, as the gather and the carry read them
static StreamSrc fft_stream_src(const csdr_fft_batch *f, const float *d_in, long long in_stride, const WireIn &wire,
                                const double *d_dc, const DcBlank *blank)
{
    StreamSrc a;
    a.in = d_in; a.in_stride = (long)in_stride; a.wire = wire; a.dc = d_dc;
    a.carry = f->d_carry; a.pos = f->ds.pos; a.carry_stride = f->size; a.channels = f->channels;
    a.nb_mask = blank ? blank->mask : nullptr; a.nb_mask_stride = blank ? blank->mask_stride : 0;
    a.nb_state = blank ? (const NbChan *)blank->state : nullptr; a.nb_hist = blank ? blank->hist : nullptr;
    return a;
}
// m_DataBuf after a call of n samples: they are appended when no frame completed, else it holds the last next_pos of them
static int fft_carry(csdr_fft_batch *f, const StreamSrc &a, long long n, int next_pos, hipStream_t st)
{
    if (f->ds.pos + n < f->size) CSDR_HIP(display_carry_launch(a, f->d_carry, f->ds.pos, 0, (int)n, st));
    else CSDR_HIP(display_carry_launch(a, f->d_carry, 0, n - next_pos, next_pos, st));
    return CSDR_OK;
}

static int fft_put_stream_rows(csdr_fft_batch *f, const float *d_in, long long in_stride, const WireIn &wire, long long n,
                               const double *d_dc, void *stream, const DcBlank *blank)
{
    const int N = f->size, l2 = log2_of(N), C = f->channels;
    const bool loaders = !blank && spectrum_stream_loaders_ok(l2);
    hipStream_t st = (hipStream_t)stream;
    if (!f->rows_disp) f->rs.assign((size_t)C, f->ds);
    if (!f->rows_ave) f->ave_r.assign((size_t)C, f->ave_size);
    TabSlot slot(f, st);
    if (int rc = slot.acquire()) return rc;
    enum { GATH, LOAD };
    const DisplayRowsSplit d = display_rows_plan(f->rs.data(), f->ave_r.data(), C, f->ds.pos, n, N, loaders, 0,
                                                 !spectrum_single_launch(l2), f->rs_next.data(), f->emits_next.data(),
                                                 slot.host(GATH), slot.host(LOAD));
    const StreamSrc a = fft_stream_src(f, d_in, in_stride, wire, d_dc, blank);
    if (d.ngath > 0) {
        CSDR_HIP(fft_grow(f->d_stage, f->stage_cap, (size_t)C * d.max_gath * N * 2, st));
        CSDR_HIP(slot.send(GATH, d.ngath));
        CSDR_HIP(display_gather_rows_launch(a, slot.dev(GATH), d.ngath, d.max_gath, N, f->d_stage, st));
        const RowTable tab{slot.dev(GATH), slot.host(GATH), d.ngath};
        if (int rc = fft_put_frames(f, f->d_stage, (long long)d.max_gath * N, d.max_gath, stream, nullptr, &tab)) return rc;
    }
    if (d.nload > 0) {
        CSDR_HIP(slot.send(LOAD, d.nload));
        const FrameSrc src{0, 0, d_dc, wire.pk, wire.chan_stride, wire.pkt_len, nullptr};
        const RowTable tab{slot.dev(LOAD), slot.host(LOAD), d.nload};
        if (int rc = fft_put_frames(f, d_in, in_stride, d.max_load, stream, &src, &tab)) return rc;
    }
    if (int rc = slot.done()) return rc;
    if (int rc = fft_carry(f, a, n, d.next_pos, st)) return rc;
    f->rs.swap(f->rs_next);
    f->emits.swap(f->emits_next);
    if (!f->rows_disp) f->ds = f->rs[0];
    f->ds.pos = d.next_pos;
    return d.max_count;
}

static int fft_put_stream(csdr_fft_batch *f, const float *d_in, long long in_stride, const WireIn &wire, long long n,
                          const double *d_dc, void *stream, const DcBlank *blank = nullptr)
{
    if (n == 0) { f->emits.assign((size_t)f->channels, 0); return 0; }
    if (!device_ok(f->device)) return CSDR_EHIP;
    if (fft_row_form(f)) return fft_put_stream_rows(f, d_in, in_stride, wire, n, d_dc, stream, blank);
    const int N = f->size, l2 = log2_of(N);
    // (CSDR_DISPLAY_BLANKED_LOADERS=0: every used frame of a blanked call through the gather -- the A/B of
    // tools/bench_display_blanked.py; the words are the same)
    static const bool blanked_loaders = !(getenv("CSDR_DISPLAY_BLANKED_LOADERS") && atoi(getenv("CSDR_DISPLAY_BLANKED_LOADERS")) == 0);
    const bool loaders = blank ? blanked_loaders && spectrum_stream_blanked_ok(l2, wire.pk ? wire.pkt_len : 0)
                               : spectrum_stream_loaders_ok(l2);
    const long long first_loaded = blank ? NB_MAX_WIDTH / 2 + 1 : 0;       // the loaders take frames from here on
    const DisplayPlan p = display_plan(f->ds, n, N);
    hipStream_t st = (hipStream_t)stream;
    const StreamSrc a = fft_stream_src(f, d_in, in_stride, wire, d_dc, blank);
    long long start = p.start;
    int left = p.count;
    auto in_place = [&](int k) { return !blank && !wire.pk && !d_dc && start >= 0 && (k == 1 || p.step == N); };
    if (left > 0 && !in_place(left) && (start < first_loaded || !loaders)) {
        int ng = left;
        if (loaders)                                    // (unblanked: the one frame that begins in the carry)
            for (ng = 1; ng < left && start + ng * p.step < first_loaded; ) ng++;
        CSDR_HIP(fft_grow(f->d_stage, f->stage_cap, (size_t)f->channels * ng * N * 2, st));
        CSDR_HIP(display_gather_launch(a, start, p.step, ng, N, f->d_stage, st));
        const int rc = fft_put_frames(f, f->d_stage, (long long)ng * N, ng, stream);
        if (rc) return rc;
        start += (long long)ng * p.step; left -= ng;
    }
    if (left > 0) {
        int rc;
        if (in_place(left)) rc = fft_put_frames(f, d_in + 2 * start, in_stride, left, stream);
        else {
            const FrameSrc src{start, p.step, d_dc, wire.pk, wire.chan_stride, wire.pkt_len, blank};
            rc = fft_put_frames(f, d_in, in_stride, left, stream, &src);
        }
        if (rc) return rc;
    }
    if (int rc = fft_carry(f, a, n, p.next.pos, st)) return rc;
    f->ds = p.next;
    f->emits.assign((size_t)f->channels, p.count);
    return p.count;
}

int csdr_fft_batch_set_display_rate(csdr_fft_batch *f, double sample_rate, int max_display_rate, int gated)
{   // CSdrInterface::SetMaxDisplayRate (sdrinterface.h:112-114), and the m_ScreenUpateFinished handshake on or off
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (!(sample_rate > 0) || max_display_rate < 1) return fail(CSDR_EINVAL, "sample rate > 0, display rate >= 1");
    f->disp_fs = sample_rate; f->disp_rate = max_display_rate;
    f->ds.skip = display_skip_value(sample_rate, f->size, max_display_rate);
    f->ds.counter = 0;
    f->ds.gated = gated != 0;
    if (f->rows_disp) {          // every row takes these settings and the display half of the row form ends; the one gate
        f->ds.ready = 1;                                                         // left is open if every row's was
        for (int r = 0; r < f->channels; r++) f->ds.ready &= f->rs[r].ready;
        f->rows_disp = false;
    }
    return CSDR_OK;
}
int csdr_fft_batch_set_display_rate_row(csdr_fft_batch *f, int row, int max_display_rate, int gated)
{   // SetMaxDisplayRate of one row at the object's sample rate and size; its handshake on or off
    int lo, hi;
    if (int rc = fft_row_range(f, row, &lo, &hi)) return rc;
    if (max_display_rate < 1) return fail(CSDR_EINVAL, "display rate >= 1");
    if (int rc = fft_rows_enter(f, false, true)) return rc;
    const double fs = f->disp_fs > 0 ? f->disp_fs : f->fs;
    for (int r = lo; r < hi; r++) {
        f->rate_r[r] = max_display_rate;
        f->rs[r].skip = display_skip_value(fs, f->size, max_display_rate);
        f->rs[r].counter = 0;
        f->rs[r].gated = gated != 0;
    }
    return CSDR_OK;
}
int csdr_fft_batch_screen_update_done(csdr_fft_batch *f)
{   // CSdrInterface::ScreenUpdateDone (sdrinterface.h:67), of every listener
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    f->ds.ready = 1;
    if (f->rows_disp) for (auto &r : f->rs) r.ready = 1;
    return CSDR_OK;
}
int csdr_fft_batch_screen_update_done_row(csdr_fft_batch *f, int row)
{   // ScreenUpdateDone() of one listener
    int lo, hi;
    if (int rc = fft_row_range(f, row, &lo, &hi)) return rc;
    if (int rc = fft_rows_enter(f, false, true)) return rc;          // (host state only from the second call on)
    for (int r = lo; r < hi; r++) f->rs[r].ready = 1;
    return CSDR_OK;
}
int csdr_fft_batch_stream_reset(csdr_fft_batch *f)
{   // CSdrInterface::StartSdr (sdrinterface.cpp:512, 591): m_FftBufPos = 0, m_ScreenUpateFinished = TRUE (every row's)
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    f->ds.pos = 0; f->ds.ready = 1;
    if (f->rows_disp) for (auto &r : f->rs) r.ready = 1;
    return CSDR_OK;
}
int csdr_fft_batch_put_display_stream(csdr_fft_batch *f, const float *d_in, long long in_stride, int n,
                                      const double *d_dc, void *stream)
{
    if (!f || !d_in || n < 0 || in_stride < n) return fail(CSDR_EINVAL, "bad argument");
    if ((uintptr_t)d_in & 7) return fail(CSDR_EINVAL, "d_in must be 8-byte aligned");
    return fft_put_stream(f, d_in, in_stride, WireIn{nullptr, 0, 0, 0}, n, d_dc, stream);
}
// the datagram rules of csdr_demod_batch_process_packets: the samples per datagram, or the error
static int fft_datagram_samples(bool handles, const void *d_packets, int npackets, int pkt_len)
{
    if (!handles || !d_packets || npackets < 0) return fail(CSDR_EINVAL, "bad argument");
    if (pkt_len != 1028 && pkt_len != 1444) return fail(CSDR_EINVAL, "packet length %d", pkt_len);
    if ((long)npackets * pkt_len >= (1l << 31)) return fail(CSDR_EINVAL, "a channel's datagrams of one call must stay below 2 GiB");
    if ((uintptr_t)d_packets & 3) return fail(CSDR_EINVAL, "datagram buffer must be 4-byte aligned");
    return pkt_len == 1444 ? 240 : 256;
}
int csdr_fft_batch_put_display_packets(csdr_fft_batch *f, const void *d_packets, int npackets, int pkt_len,
                                       const double *d_dc, void *stream)
{
    const int per = fft_datagram_samples(f != nullptr, d_packets, npackets, pkt_len);
    if (per < 0) return per;
    return fft_put_stream(f, nullptr, 0, WireIn{(const unsigned char *)d_packets, (long)npackets * pkt_len, pkt_len, per},
                          (long long)npackets * per, d_dc, stream);
}
// the blanked pair: the chain `b` remembers its last blanked call (csdr__demod_batch_last_blank) -- the display reads the
// same input through the mask, state and history half that call's mask pass left, so it must be THAT call's input
static int fft_blank_of(csdr_fft_batch *f, csdr_demod_batch *b, int form, const void *src, long long stride, int n,
                        DcBlank *blank)
{
    return csdr__demod_batch_blank_for(b, "display", f->channels, f->device, form, src, stride, n, blank);
}
int csdr_fft_batch_put_display_stream_blanked(csdr_fft_batch *f, csdr_demod_batch *b, const float *d_in,
                                              long long in_stride, int n, const double *d_dc, void *stream)
{
    if (!f || !b || !d_in || n < 0 || in_stride < n) return fail(CSDR_EINVAL, "bad argument");
    if ((uintptr_t)d_in & 7) return fail(CSDR_EINVAL, "d_in must be 8-byte aligned");
    DcBlank blank;
    { const int rc = fft_blank_of(f, b, BLANK_CALL_ROWS, d_in, in_stride, n, &blank); if (rc) return rc; }
    return fft_put_stream(f, d_in, in_stride, WireIn{nullptr, 0, 0, 0}, n, d_dc, stream, &blank);
}
int csdr_fft_batch_put_display_packets_blanked(csdr_fft_batch *f, csdr_demod_batch *b, const void *d_packets,
                                               int npackets, int pkt_len, const double *d_dc, void *stream)
{
    const int per = fft_datagram_samples(f && b, d_packets, npackets, pkt_len);
    if (per < 0) return per;
    DcBlank blank;
    { const int rc = fft_blank_of(f, b, BLANK_CALL_PACKETS, d_packets, pkt_len, npackets * per, &blank); if (rc) return rc; }
    return fft_put_stream(f, nullptr, 0, WireIn{(const unsigned char *)d_packets, (long)npackets * pkt_len, pkt_len, per},
                          (long long)npackets * per, d_dc, stream, &blank);
}
/* copy of m_pFFTAveBuf of one channel (bels, display order), synchronises */
int csdr_fft_batch_get_ave(csdr_fft_batch *f, int channel, float *out)
{
    if (!f || !out || channel < 0 || channel >= f->channels) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->device)) return CSDR_EHIP;
    { const int rc = fft_read(f, out, f->d_ave + (size_t)channel * f->size, (size_t)f->size * 4); if (rc) return rc; }
    return f->size;
}
int csdr_fft_batch_get_total_count(csdr_fft_batch *f, int channel)
{
    if (!f || channel < 0 || channel >= f->channels) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->device)) return CSDR_EHIP;
    int c[2];
    { const int rc = fft_read(f, c, f->d_cnt + 2 * channel, sizeof(c)); if (rc) return rc; }
    return c[1];
}

// the display bins of start_hz ... stop_hz (fft.cpp:336-349)
static void fft_bin_range(const csdr_fft_batch *f, int start_hz, int stop_hz, int *bin_min, int *bin_max)
{
    const int n = f->size, maxbin = n - 1;
    *bin_min = (int)((double)start_hz * (double)n / f->fs) + n / 2;
    *bin_max = (int)((double)stop_hz * (double)n / f->fs) + n / 2;
    if (*bin_min < 0) *bin_min = 0;
    if (*bin_min >= maxbin) *bin_min = maxbin;
    if (*bin_max < 0) *bin_max = 0;
    if (*bin_max >= maxbin) *bin_max = maxbin;
}

/* CFft::GetScreenIntegerFFTData (fft.cpp:308-410) on the N-float read-back of one channel.
 * Returns 1 if the last PutInDisplayFFT saw an overload, 0 otherwise. */
int csdr_fft_batch_get_screen(csdr_fft_batch *f, int channel, int max_h, int max_w, double max_db, double min_db,
                              int start_hz, int stop_hz, int *out)
{
    if (!f || !out || channel < 0 || channel >= f->channels) return fail(CSDR_EINVAL, "bad argument");
    const int n = f->size;
    f->h_ave.resize(n);
    int rc = csdr_fft_batch_get_ave(f, channel, f->h_ave.data());
    if (rc < 0) return rc;
    int over = 0;
    { const int rc2 = fft_read(f, &over, f->d_over + channel, sizeof(int)); if (rc2) return rc2; }
    const float *ave = f->h_ave.data();
    int i, x, y, ymax = 10000, xprev = -1;
    const double off = max_db / 10.0, gain = -10.0 / (max_db - min_db);
    if (f->start_hz != start_hz || f->stop_hz != stop_hz || f->plot_w != max_w) {
        f->start_hz = start_hz; f->stop_hz = stop_hz; f->plot_w = max_w;
        fft_bin_range(f, start_hz, stop_hz, &f->bin_min, &f->bin_max);
        if ((f->bin_max - f->bin_min) > f->plot_w) {
            for (i = f->bin_min; i <= f->bin_max; i++)
                f->xlat[i] = ((i - f->bin_min) * f->plot_w) / (f->bin_max - f->bin_min);
        } else {
            for (i = 0; i < f->plot_w && i < n; i++)
                f->xlat[i] = f->bin_min + (i * (f->bin_max - f->bin_min)) / f->plot_w;
        }
    }
    auto level = [&](int bin) {
        int b = f->invert ? (n - bin) : bin;
        if (b >= n) b = n - 1;                         // the reference reads one past the end here
        int v = (int)((double)max_h * gain * ((double)ave[b] - off));
        if (v < 0) v = 0;
        if (v > max_h) v = max_h;
        return v;
    };
    if ((f->bin_max - f->bin_min) > f->plot_w) {
        for (i = f->bin_min; i <= f->bin_max; i++) {
            y = level(i);
            x = f->xlat[i];
            if (x >= f->plot_w) continue;              // the reference writes OutBuf[MaxWidth] here (one past the end)
            if (x == xprev) {
                if (y < ymax) { out[x] = y; ymax = y; }
            } else {
                out[x] = y; xprev = x; ymax = y;
            }
        }
    } else {
        for (x = 0; x < f->plot_w; x++) out[x] = level(f->xlat[x < n ? x : n - 1]);
    }
    return over ? 1 : 0;
}

int csdr_fft_batch_get_screen_all(csdr_fft_batch *f, int max_h, int max_w, double max_db, double min_db,
                                  int start_hz, int stop_hz, int *d_out, long long out_stride, int *d_overload,
                                  void *stream)
{
    if (!f || !d_out || max_w < 0 || out_stride < max_w) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->device)) return CSDR_EHIP;
    ScreenArgs a;
    a.ave = f->d_ave; a.out = d_out; a.out_stride = out_stride; a.n = f->size; a.channels = f->channels;
    fft_bin_range(f, start_hz, stop_hz, &a.bin_min, &a.bin_max);
    a.plot_w = max_w; a.max_h = max_h; a.invert = f->invert;
    a.off = max_db / 10.0; a.gain = -10.0 / (max_db - min_db);
    CSDR_HIP(screen_launch(a, (hipStream_t)stream));
    if (d_overload)
        CSDR_HIP(hipMemcpyAsync(d_overload, f->d_over, sizeof(int) * f->channels, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CSDR_OK;
}

void csdr_plotter_color_table(unsigned int *out256)
{
    if (out256) for (int i = 0; i < 256; i++) out256[i] = plotter_color(i);
}

int csdr_fft_batch_get_waterfall_all(csdr_fft_batch *f, int max_w, double max_db, double min_db, int start_hz,
                                     int stop_hz, unsigned int *d_rgb, long long out_stride, int *d_overload,
                                     void *stream)
{
    if (!f || !d_rgb || max_w < 0 || out_stride < max_w) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->device)) return CSDR_EHIP;
    if (max_w == 0) return CSDR_OK;
    const size_t need = (size_t)f->channels * max_w;
    CSDR_HIP(fft_grow(f->d_scr, f->scr_cap, need, (hipStream_t)stream));   // the levels of the line, [channels][max_w]
    CSDR_HIP(hipMemsetAsync(f->d_scr, 0xff, need * sizeof(int), (hipStream_t)stream));     // -1: not touched
    int rc = csdr_fft_batch_get_screen_all(f, 255, max_w, max_db, min_db, start_hz, stop_hz, f->d_scr, max_w, d_overload, stream);
    if (rc < 0) return rc;
    CSDR_HIP(waterfall_color_launch(f->d_scr, max_w, d_rgb, out_stride, max_w, f->channels, (hipStream_t)stream));
    return CSDR_OK;
}

/* CFft::FwdFFT / RevFFT (fft.cpp:416-426) of nframes frames of every row; asynchronous, nothing of the display state read
 * or written (not last_stream either: the readers wait for display calls only) */
static int fft_batch_plain(csdr_fft_batch *f, const float *d_in, long long in_stride, float *d_out, long long out_stride,
                           int nframes, void *stream, int sign)
{
    if (!f || !d_in || !d_out || nframes < 0) return fail(CSDR_EINVAL, "bad argument");
    if (nframes == 0) return CSDR_OK;
    const long long need = (long long)nframes * f->size;
    if (in_stride < need || out_stride < need) return fail(CSDR_EINVAL, "a row's stride must hold its %d frames of %d", nframes, f->size);
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) return fail(CSDR_EINVAL, "d_in and d_out must be 8-byte aligned");
    if (!(d_in == d_out && in_stride == out_stride)) {
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + (uintptr_t)((f->channels - 1) * in_stride + need) * 8;
        const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (uintptr_t)((f->channels - 1) * out_stride + need) * 8;
        if (a0 < b1 && b0 < a1) return fail(CSDR_EINVAL, "d_out overlaps d_in (in place is d_out == d_in with equal strides)");
    }
    if ((long long)f->channels * nframes > 0x7fffffffll) return fail(CSDR_EINVAL, "channels * nframes must stay below 2^31");
    if (!device_ok(f->device)) return CSDR_EHIP;
    PlainBatchArgs a;
    a.in = d_in; a.in_stride = (long)in_stride; a.out = d_out; a.out_stride = (long)out_stride;
    a.channels = f->channels; a.nframes = nframes; a.sign = sign;
    a.tw1 = f->d_tw1; a.tw2 = f->d_tw2; a.twp = f->d_twp; a.work = f->d_pwork; a.group = f->plain_group;
    CSDR_HIP(fft_batch_plain_launch(log2_of(f->size), a, (hipStream_t)stream));
    return CSDR_OK;
}
int csdr_fft_batch_fwd(csdr_fft_batch *f, const float *d_in, long long in_stride, float *d_out, long long out_stride,
                       int nframes, void *stream)
{ return fft_batch_plain(f, d_in, in_stride, d_out, out_stride, nframes, stream, +1); }
int csdr_fft_batch_rev(csdr_fft_batch *f, const float *d_in, long long in_stride, float *d_out, long long out_stride,
                       int nframes, void *stream)
{ return fft_batch_plain(f, d_in, in_stride, d_out, out_stride, nframes, stream, -1); }
int csdr_fft_batch_plain_group(csdr_fft_batch *f) { return f ? f->plain_group : fail(CSDR_EINVAL, "bad handle"); }

/* ---- the same in fp64 (K3q): the reference's own precision, TYPECPX = two doubles ---- */
// the table and the work buffer of the object's present size; allocates and waits, once per set_params
static int fft64_group(const csdr_fft_batch *f)
{   // as the fp32 form: 64 frames (a launch of 512 ... 1024 workgroups), and at least one of every row
    if (log2_of(f->size) <= PLAIN64_MAX_LOG2N) return 0;
    return f->channels < 64 ? 64 / f->channels : 1;
}
static int fft64_prepare(csdr_fft_batch *f)
{
    if (f->ready64) return CSDR_OK;
    if (!device_ok(f->device)) return CSDR_EHIP;
    fft64_drop(f);
    const int n = f->size, l2 = log2_of(n);
    const bool single = l2 <= PLAIN64_MAX_LOG2N;
    std::vector<double> tw;
    fft64_tables(n, single, tw);
    CSDR_HIP(hipMalloc((void **)&f->d_tw64, tw.size() * sizeof(double)));
    CSDR_HIP(hipMemcpy(f->d_tw64, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!single) {
        f->plain_group64 = fft64_group(f);
        CSDR_HIP(hipMalloc((void **)&f->d_work64, (size_t)f->channels * f->plain_group64 * n * 16));
    }
    f->ready64 = true;
    return CSDR_OK;
}
static int fft_batch_plain64(csdr_fft_batch *f, const double *d_in, long long in_stride, double *d_out, long long out_stride,
                             int nframes, void *stream, int sign)
{
    if (!f || !d_in || !d_out || nframes < 0) return fail(CSDR_EINVAL, "bad argument");
    if (nframes == 0) return CSDR_OK;
    const long long need = (long long)nframes * f->size;
    if (in_stride < need || out_stride < need) return fail(CSDR_EINVAL, "a row's stride must hold its %d frames of %d", nframes, f->size);
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 15) return fail(CSDR_EINVAL, "d_in and d_out must be 16-byte aligned");
    if (!(d_in == d_out && in_stride == out_stride)) {
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + (uintptr_t)((f->channels - 1) * in_stride + need) * 16;
        const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (uintptr_t)((f->channels - 1) * out_stride + need) * 16;
        if (a0 < b1 && b0 < a1) return fail(CSDR_EINVAL, "d_out overlaps d_in (in place is d_out == d_in with equal strides)");
    }
    if ((long long)f->channels * nframes > 0x7fffffffll) return fail(CSDR_EINVAL, "channels * nframes must stay below 2^31");
    if (fft64_group(f) > 0 && f->channels > 65535)           // (a grid dimension of the four-step launches)
        return fail(CSDR_EINVAL, "the fp64 transforms of 8192 points and above take at most 65535 rows");
    if (!device_ok(f->device)) return CSDR_EHIP;             // every call: the launch, its LDS attribute and a NULL stream are the current device's
    if (int rc = fft64_prepare(f)) return rc;
    PlainBatch64Args a;
    a.in = d_in; a.in_stride = (long)in_stride; a.out = d_out; a.out_stride = (long)out_stride;
    a.channels = f->channels; a.nframes = nframes; a.sign = sign;
    a.tw = f->d_tw64; a.work = f->d_work64; a.group = f->plain_group64;
    CSDR_HIP(fft_batch_plain64_launch(log2_of(f->size), a, (hipStream_t)stream));
    return CSDR_OK;
}
int csdr_fft_batch_prepare_f64(csdr_fft_batch *f) { return f ? fft64_prepare(f) : fail(CSDR_EINVAL, "bad handle"); }
int csdr_fft_batch_fwd_f64(csdr_fft_batch *f, const double *d_in, long long in_stride, double *d_out, long long out_stride,
                           int nframes, void *stream)
{ return fft_batch_plain64(f, d_in, in_stride, d_out, out_stride, nframes, stream, +1); }
int csdr_fft_batch_rev_f64(csdr_fft_batch *f, const double *d_in, long long in_stride, double *d_out, long long out_stride,
                           int nframes, void *stream)
{ return fft_batch_plain64(f, d_in, in_stride, d_out, out_stride, nframes, stream, -1); }
int csdr_fft_batch_plain_group_f64(csdr_fft_batch *f)
{
    return f ? fft64_group(f) : fail(CSDR_EINVAL, "bad handle");      // (of the present size, prepared or not)
}
// for the tests: the table csdr_fft_batch_prepare_f64 builds for an n-point transform, (cos, sin) pairs; returns the
// number of doubles (at most cap are written); no device needed
int csdr__host_fft_tw64(int n, double *out, int cap)
{
    if (log2_of(n) < 9 || log2_of(n) > 16 || (cap > 0 && !out)) return fail(CSDR_EINVAL, "bad argument");
    std::vector<double> tw;
    fft64_tables(n, log2_of(n) <= PLAIN64_MAX_LOG2N, tw);
    for (int i = 0; i < cap && i < (int)tw.size(); i++) out[i] = tw[i];
    return (int)tw.size();
}

// for the tests: one row's running sum [size] and {ave_count, total_count}, behind the object's last put
int csdr__fft_batch_row_state(csdr_fft_batch *f, int row, float *sum, int *counters2)
{
    if (!f || !sum || !counters2 || row < 0 || row >= f->channels) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->device)) return CSDR_EHIP;
    if (int rc = fft_read(f, sum, f->d_sum + (size_t)row * f->size, (size_t)f->size * 4)) return rc;
    return fft_read(f, counters2, f->d_cnt + 2 * row, 2 * sizeof(int));
}
// what csdr_plotter_batch_draw reads: nothing of the cached translate table, and nothing here is changed
int csdr__fft_batch_view(csdr_fft_batch *f, FftView *v)
{
    if (!f || !v) return fail(CSDR_EINVAL, "bad argument");
    v->device = f->device; v->channels = f->channels; v->size = f->size; v->invert = f->invert; v->fs = f->fs;
    v->d_ave = f->d_ave; v->d_over = f->d_over;
    return CSDR_OK;
}

}  // extern "C"

/* ---------------- single-channel host form: CFft drop-in ---------------- */
struct csdr_fft {
    csdr_fft_batch *b;
    float *d_buf; size_t cap;
    PinnedBuf pin;                   // page-locked fp32 staging of the frame (both directions of the plain transforms)
    hipStream_t s = nullptr;         // the object's stream: the frame's copy and its kernels in order, no host wait in PutInDisplayFFT
    hipEvent_t ev_h2d = nullptr;     // the last frame has left the pinned buffer
    bool h2d_busy = false;
    int total = 0;                   // m_TotalCount mirrored on the host: frames since the last reset (fft.cpp:515-517)
};

static int fft_host_buf(csdr_fft *f, size_t n)
{
    if (n <= f->cap) return CSDR_OK;
    if (f->d_buf) (void)hipFree(f->d_buf);
    f->d_buf = nullptr; f->cap = 0;
    CSDR_HIP(hipMalloc((void **)&f->d_buf, n * 8));
    f->cap = n;
    return CSDR_OK;
}

extern "C" {

csdr_fft *csdr_fft_create(int device)
{
    csdr_fft_batch *b = csdr_fft_batch_create(device, 1);
    if (!b) return nullptr;
    csdr_fft *f = new csdr_fft();
    f->b = b; f->d_buf = nullptr; f->cap = 0;
    if (hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&f->ev_h2d, hipEventDisableTiming) != hipSuccess) {
        if (f->s) (void)hipStreamDestroy(f->s);
        csdr_fft_batch_destroy(b); delete f; fail(CSDR_EHIP, "stream creation failed"); return nullptr;
    }
    return f;
}
void csdr_fft_destroy(csdr_fft *f)
{
    if (!f) return;
    (void)hipSetDevice(f->b->device);
    if (f->s) { (void)hipStreamSynchronize(f->s); (void)hipStreamDestroy(f->s); }
    if (f->ev_h2d) (void)hipEventDestroy(f->ev_h2d);
    if (f->d_buf) (void)hipFree(f->d_buf);
    csdr_fft_batch_destroy(f->b);
    delete f;
}
// (the setters below synchronise the device inside the batch object: nothing of this object's stream is in flight after them)
int csdr_fft_set_params(csdr_fft *f, int size, int invert, double db_comp, double fs)
{
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (f->s) CSDR_HIP(hipStreamSynchronize(f->s));
    f->total = 0;
    return csdr_fft_batch_set_params(f->b, size, invert, db_comp, fs);
}
int csdr_fft_set_ave(csdr_fft *f, int ave)
{
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (f->s) CSDR_HIP(hipStreamSynchronize(f->s));
    f->total = 0;                                        // SetFFTAve ends in ResetFFT (fft.cpp:103-113)
    return csdr_fft_batch_set_ave(f->b, ave);
}
int csdr_fft_reset(csdr_fft *f)
{
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    if (f->s) CSDR_HIP(hipStreamSynchronize(f->s));
    f->total = 0;
    return csdr_fft_batch_reset(f->b);
}

/* CFft::PutInDisplayFFT (fft.cpp:267-288): n should equal the FFT size; returns m_TotalCount */
int csdr_fft_put_display(csdr_fft *f, int n, const double *in_iq)
{
    if (!f || n < 0 || (n && !in_iq)) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->b->device)) return CSDR_EHIP;
    const int N = f->b->size;
    int rc = fft_host_buf(f, (size_t)N);
    if (rc) return rc;
    if ((rc = f->pin.reserve(2 * (size_t)N))) return rc;
    // The frame goes fp64 -> fp32 into pinned memory and from there to the device on the object's stream, the spectrum
    // kernels behind it: nothing here waits for the GPU (the reference's caller does not either -- the readers,
    // GetScreenIntegerFFTData / get_ave, synchronise).  The pinned buffer is reused once its last copy has left.
    if (f->h2d_busy) { CSDR_HIP(hipEventSynchronize(f->ev_h2d)); f->h2d_busy = false; }
    const int m = n < N ? n : N;
    cvt_to_f32(f->pin.p, in_iq, 2 * (size_t)m);
    if (m < N) memset(f->pin.p + 2 * (size_t)m, 0, 2 * (size_t)(N - m) * sizeof(float));   // the reference keeps stale data past n; zeros here
    CSDR_HIP(hipMemcpyAsync(f->d_buf, f->pin.p, (size_t)N * 8, hipMemcpyHostToDevice, f->s));
    CSDR_HIP(hipEventRecord(f->ev_h2d, f->s));
    f->h2d_busy = true;
    rc = csdr_fft_batch_put_display(f->b, f->d_buf, N, 1, (void *)f->s);
    if (rc) return rc;
    return ++f->total;                                   // m_TotalCount (fft.cpp:287): frames since the last reset
}
/* CFft::GetScreenIntegerFFTData (fft.cpp:308-410); returns the overload flag */
int csdr_fft_get_screen(csdr_fft *f, int max_h, int max_w, double max_db, double min_db, int start_hz,
                        int stop_hz, int *out)
{ return f ? csdr_fft_batch_get_screen(f->b, 0, max_h, max_w, max_db, min_db, start_hz, stop_hz, out)
           : fail(CSDR_EINVAL, "bad handle"); }
int csdr_fft_get_ave(csdr_fft *f, float *out)
{ return f ? csdr_fft_batch_get_ave(f->b, 0, out) : fail(CSDR_EINVAL, "bad handle"); }

/* CFft::FwdFFT / RevFFT (fft.cpp:416-426): in-place N-point transform of interleaved doubles.
 * The reference's FwdFFT also feeds the display average; this one does not. */
static int fft_plain(csdr_fft *f, double *inout, int sign)
{
    if (!f || !inout) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->b->device)) return CSDR_EHIP;
    const int N = f->b->size;
    int rc = fft_host_buf(f, (size_t)N);
    if (rc) return rc;
    if ((rc = f->pin.reserve(2 * (size_t)N))) return rc;
    if (f->h2d_busy) { CSDR_HIP(hipEventSynchronize(f->ev_h2d)); f->h2d_busy = false; }
    cvt_to_f32(f->pin.p, inout, 2 * (size_t)N);
    hipStream_t st = f->s;
    CSDR_HIP(hipMemcpyAsync(f->d_buf, f->pin.p, (size_t)N * 8, hipMemcpyHostToDevice, st));
    const int l2 = log2_of(N);
    if (spectrum_single_launch(l2)) CSDR_HIP(fft_plain_launch(l2, sign, f->d_buf, f->d_buf, f->b->d_tw1, f->b->d_tw2, st));
    else CSDR_HIP(fft_generic_plain_launch(l2, sign, f->d_buf, f->d_buf, f->b->d_work, st));
    CSDR_HIP(hipMemcpyAsync(f->pin.p, f->d_buf, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    CSDR_HIP(hipStreamSynchronize(st));
    cvt_to_f64(inout, f->pin.p, 2 * (size_t)N);
    return CSDR_OK;
}
int csdr_fft_fwd(csdr_fft *f, double *inout_iq) { return fft_plain(f, inout_iq, +1); }
int csdr_fft_rev(csdr_fft *f, double *inout_iq) { return fft_plain(f, inout_iq, -1); }

/* the same in fp64: the caller's doubles as they are, the batch kernel on one row, and back */
static int fft_plain64(csdr_fft *f, double *inout, int sign)
{
    if (!f || !inout) return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(f->b->device)) return CSDR_EHIP;
    const int N = f->b->size;
    int rc = fft_host_buf(f, 2 * (size_t)N);                 // (in units of 8 bytes)
    if (rc) return rc;
    if (f->h2d_busy) { CSDR_HIP(hipEventSynchronize(f->ev_h2d)); f->h2d_busy = false; }
    if ((rc = f->pin.reserve(4 * (size_t)N))) return rc;     // growing moves the buffer: nothing is in flight from it
    double *const pin = reinterpret_cast<double *>(f->pin.p), *const dev = reinterpret_cast<double *>(f->d_buf);
    memcpy(pin, inout, (size_t)N * 16);
    hipStream_t st = f->s;
    CSDR_HIP(hipMemcpyAsync(dev, pin, (size_t)N * 16, hipMemcpyHostToDevice, st));
    rc = fft_batch_plain64(f->b, dev, N, dev, N, 1, (void *)st, sign);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    CSDR_HIP(hipMemcpyAsync(pin, dev, (size_t)N * 16, hipMemcpyDeviceToHost, st));
    CSDR_HIP(hipStreamSynchronize(st));
    memcpy(inout, pin, (size_t)N * 16);
    return CSDR_OK;
}
int csdr_fft_fwd_f64(csdr_fft *f, double *inout_iq) { return fft_plain64(f, inout_iq, +1); }
int csdr_fft_rev_f64(csdr_fft *f, double *inout_iq) { return fft_plain64(f, inout_iq, -1); }

}  // extern "C"
