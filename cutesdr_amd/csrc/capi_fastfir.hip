// capi_fastfir.hip -- C ABI for CFastFIR (single-channel host form and batched device form).
#include "capi_common.hpp"
#include "capi_internal.hpp"
#include <algorithm>
#include "fastfir_kernels.h"
#include "fastfir_design_kernels.h"
#include "host_math.hpp"
#include "patch_queue.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace csdr;

struct csdr_fastfir_batch {
    int device, channels, n, log2n;
    int cus;                          // compute units of the device (run-length heuristic)
    hipStream_t last_stream;          // stream of the most recent process call (setup waits for it)
    bool per_channel;                 // false: one shared filter
    float *d_h;                       // [filters][n] complex fp32 in pass-F3 register order of the generic kernel
    float *d_h2;                      // the same responses in the pipelined kernel's order, at every size (it consumes H as
                                      // its tail groups finish bins); both are kept, a launch may go to either kernel
    float *d_gain;                    // [filters][n] fp32: the real gains of the same responses, Re(H[k] (-j)^k), in the
                                      // pipelined kernel's order (host_math.hpp: fastfir_gain) -- what its 16384-point
                                      // instantiation multiplies by while own_design holds
    bool own_design;                  // every response came from fastfir_design / the design kernel (linear phase): a setter
                                      // of raw responses would clear it and with it the real-gain kernel; today only the
                                      // test hook csdr__fastfir_set_own_design does
    int last_kernel;                  // FastFirKernel of the most recent process call (csdr__fastfir_last_kernel)
    float *d_hist;                    // 2 x [channels][n/2] complex fp32 (ping-pong)
    int hist_cur;                     // which half holds the previous call's tail
    int dbg_stage; float *dbg_out;    // diagnostics only (csdr__dbg_fastfir_stage)
    int variant;                      // 0: generic kernel (fastfir_kernels.hip); 2: pipelined build (fastfir2_kernels.hip), every size
    float *d_tw1, *d_tw2;
    double flo, fhi, off, fs;         // last shared-filter parameters (early-out like the reference)
    std::vector<std::vector<cd>> resp;   // natural-order fp64 response per filter
    std::vector<int> perm, perm2;     // device slot -> natural bin, generic / pipelined kernel
    std::vector<int> permg;           // gain slot -> natural bin
    // A new frequency response does not stop anything: SetupParameters designs it on the host and queues the fp32 words
    // of both kernel orders as patches; the NEXT process call applies them on its own stream in front of its launch
    // (patch_queue.hpp) -- in stream order behind every earlier call's reads of H, so one buffer per filter suffices.
    PatchQueue patches;
    // csdr_fastfir_batch_setup_many designs on the DEVICE instead (fastfir_design_kernels.hip): a job per slot -- two
    // doubles -- queued beside the patches and launched right behind the patch kernel of the same flush, on the same
    // stream.  At most one job per slot: a later job replaces it, a later host design (a patch of the slot's rows) cancels
    // it; a job queued behind a patch of its slot wins, because its launch follows the patch kernel.  resp[slot] is then
    // older than the device's fp64 row (stale[slot]) until a reader asks for it (fetch_mirror).
    std::vector<DesignJob> jobs;
    std::vector<int> job_of;          // slot -> index into jobs, or -1
    std::vector<char> stale;          // slot -> resp[slot] has to be fetched from d_resp
    double *d_win = nullptr, *d_tw = nullptr;     // fastfir_window and design_twiddles (host_math.hpp), fp64
    int *d_perm = nullptr, *d_perm2 = nullptr, *d_permg = nullptr;    // perm / perm2 / permg
    double *d_resp = nullptr;         // [channels][n] complex fp64, natural order; all five allocated by the first setup_many
    hipEvent_t ev_design = nullptr;   // behind the last design launch
};

static void cancel_job(csdr_fastfir_batch *b, int slot)
{
    const int i = b->job_of[slot];
    if (i < 0) return;
    b->job_of[slot] = -1;
    if ((size_t)i + 1 != b->jobs.size()) { b->jobs[i] = b->jobs.back(); b->job_of[b->jobs[i].slot] = i; }
    b->jobs.pop_back();
}

static void queue_job(csdr_fastfir_batch *b, int slot, double nfc, double nfs)
{
    const DesignJob j{slot, 0, nfc, nfs};
    if (b->job_of[slot] >= 0) b->jobs[b->job_of[slot]] = j;
    else { b->job_of[slot] = (int)b->jobs.size(); b->jobs.push_back(j); }
    b->stale[slot] = 1;
}

// the queued patches, then the queued design jobs, in `s`'s order (both queues are empty afterwards)
static int flush_control(csdr_fastfir_batch *b, hipStream_t s)
{
    if (b->jobs.empty()) return b->patches.flush(s);
    unsigned char *h = nullptr, *d = nullptr;
    int rc = b->patches.take(b->jobs.size() * sizeof(DesignJob), &h, &d);
    if (rc) return rc;
    memcpy(h, b->jobs.data(), b->jobs.size() * sizeof(DesignJob));
    // (launch() takes its own descriptor block from the same arena; take() adds a chunk when one is full)
    rc = b->patches.launch(s);
    hipError_t e = hipSuccess;
    if (!rc) {
        DesignArgs a;
        a.jobs = (const DesignJob *)d; a.win = b->d_win; a.tw = b->d_tw; a.perm = b->d_perm; a.perm2 = b->d_perm2;
        a.h = b->d_h; a.h2 = b->d_h2; a.resp = b->d_resp; a.permg = b->d_permg; a.gain = b->d_gain;
        e = fastfir_design_launch(b->log2n, a, (int)b->jobs.size(), s);
        if (e == hipSuccess) {
            for (const DesignJob &j : b->jobs) b->job_of[j.slot] = -1;
            b->jobs.clear();
            if (!b->ev_design) e = hipEventCreateWithFlags(&b->ev_design, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(b->ev_design, s);
        }
    }
    // on every path: the arena closes behind whatever of this flush did get launched
    const int rr = b->patches.retire(s);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CSDR_EHIP, "filter design launch: %s", hipGetErrorString(e));
    return rr;
}

// resp[slot] as the device has it: a slot designed on the device is fetched when somebody reads it (get_response, a
// receiver that takes its response to another plan group) -- the queue goes out on the object's last stream, in its order.
// The wait on ev_design comes before the copy on every path: at N = 16384 the kernel transforms inside the d_resp row.
static int fetch_mirror(csdr_fastfir_batch *b, int slot)
{
    if (!b->stale[slot]) return CSDR_OK;
    const int rc = flush_control(b, b->last_stream);
    if (rc) return rc;
    if (b->ev_design) CSDR_HIP(hipEventSynchronize(b->ev_design));
    CSDR_HIP(hipMemcpy(b->resp[slot].data(), b->d_resp + (size_t)slot * 2 * b->n, sizeof(cd) * (size_t)b->n, hipMemcpyDeviceToHost));
    b->stale[slot] = 0;
    return CSDR_OK;
}

// tables and rows of the device-side design, once in an object's life (the first setup_many: blocking allocations and
// copies, the only part of that call that waits).  d_resp has a row per CHANNEL from the start, so the later switch from
// a shared filter to per-channel filters has nothing to reallocate here.
static int design_state(csdr_fastfir_batch *b)
{
    if (b->d_resp) return CSDR_OK;
    const size_t n = (size_t)b->n, p = n / 2 + 1;
    const auto win = fastfir_window((int)p);
    const auto tw = design_twiddles(n);
    if (!b->d_win) CSDR_HIP(hipMalloc((void **)&b->d_win, p * sizeof(double)));
    if (!b->d_tw) CSDR_HIP(hipMalloc((void **)&b->d_tw, n * sizeof(double)));
    if (!b->d_perm) CSDR_HIP(hipMalloc((void **)&b->d_perm, n * sizeof(int)));
    if (!b->d_perm2) CSDR_HIP(hipMalloc((void **)&b->d_perm2, n * sizeof(int)));
    if (!b->d_permg) CSDR_HIP(hipMalloc((void **)&b->d_permg, n * sizeof(int)));
    CSDR_HIP(hipMemcpy(b->d_win, win->data(), p * sizeof(double), hipMemcpyHostToDevice));
    CSDR_HIP(hipMemcpy(b->d_tw, tw.data(), n * sizeof(double), hipMemcpyHostToDevice));
    CSDR_HIP(hipMemcpy(b->d_perm, b->perm.data(), n * sizeof(int), hipMemcpyHostToDevice));
    CSDR_HIP(hipMemcpy(b->d_perm2, b->perm2.data(), n * sizeof(int), hipMemcpyHostToDevice));
    CSDR_HIP(hipMemcpy(b->d_permg, b->permg.data(), n * sizeof(int), hipMemcpyHostToDevice));
    CSDR_HIP(hipMalloc((void **)&b->d_resp, (size_t)b->channels * n * sizeof(cd)));
    return CSDR_OK;
}

static void build_perm(csdr_fastfir_batch *b)
{
    const int T = b->n / 32;
    b->perm.resize(b->n);
    // slot layout: float4 index j*T + t holds registers r = 2j, 2j+1 of thread t
    for (int j = 0; j < 16; j++)
        for (int t = 0; t < T; t++)
            for (int e = 0; e < 2; e++)
                b->perm[(j * T + t) * 2 + e] = fastfir_bin_of(b->log2n, t, 2 * j + e);
    b->perm2.clear();
    // (the pipelined kernel's two orders with the rotation of its shared pass twiddles composed in, fastfir2_slot_bin:
    // host design, device design, re-commits and copy_row all go through these two tables)
    {
        b->perm2.resize(b->n);
        for (int j = 0; j < 16; j++)
            for (int t = 0; t < T; t++)
                for (int e = 0; e < 2; e++) b->perm2[(j * T + t) * 2 + e] = fastfir2_slot_bin(b->log2n, t, j, e);
    }
    b->permg.resize(b->n);
    for (int i = 0; i < 8; i++)
        for (int t = 0; t < T; t++)
            for (int c = 0; c < 4; c++) b->permg[(i * T + t) * 4 + c] = fastfir2_gain_slot_bin(b->log2n, t, i, c);
}

static int upload_response(csdr_fastfir_batch *b, int slot, const std::vector<cd> &H)
{
    std::vector<float> dev(2 * (size_t)b->n);
    for (int pass = 0; pass < 2; pass++) {
        const std::vector<int> &perm = pass ? b->perm2 : b->perm;
        float *dst = pass ? b->d_h2 : b->d_h;
        if (perm.empty() || !dst) continue;
        for (int i = 0; i < b->n; i++) {
            const cd v = H[perm[i]];
            dev[2 * i] = (float)v.real();
            dev[2 * i + 1] = (float)v.imag();
        }
        const int rc = b->patches.add(dst + (size_t)slot * 2 * b->n, dev.data(), dev.size() * sizeof(float));
        if (rc) return rc;
    }
    for (int i = 0; i < b->n; i++) dev[i] = (float)fastfir_gain(H[b->permg[i]], b->permg[i]);
    return b->patches.add(b->d_gain + (size_t)slot * b->n, dev.data(), (size_t)b->n * sizeof(float));
}

// a response designed on the HOST becomes slot `slot`'s: its words queued as patches, the mirror current, a design job
// still queued for the slot cancelled (the later call wins)
static int set_response(csdr_fastfir_batch *b, int slot, const std::vector<cd> &H)
{
    cancel_job(b, slot);
    const int rc = upload_response(b, slot, H);
    if (rc) return rc;
    b->resp[slot] = H;
    b->stale[slot] = 0;
    return CSDR_OK;
}

extern "C" {

csdr_fastfir_batch *csdr_fastfir_batch_create(int device, int channels, int fft_size)
{
    const int l2 = log2_of(fft_size);
    if (l2 < 11 || l2 > 14 || channels < 1) {
        fail(CSDR_EINVAL, "fft_size must be 2048..16384 (power of two), channels >= 1");
        return nullptr;
    }
    if (!device_ok(device)) return nullptr;
    csdr_fastfir_batch *b = new csdr_fastfir_batch();
    b->device = device; b->channels = channels; b->n = fft_size; b->log2n = l2;
    b->per_channel = false; b->hist_cur = 0; b->dbg_stage = 0; b->dbg_out = nullptr;
    b->last_stream = nullptr;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        b->cus = cus;
    }
    {
        // every size and block count runs the software-pipelined build; the generic kernel is reached only through
        // CSDR_FASTFIR_VARIANT=0 / csdr__fastfir_set_variant (diagnostics, and the form the pipelined one is tested against)
        const char *v = getenv("CSDR_FASTFIR_VARIANT");
        b->variant = (v && atoi(v) == 0) ? 0 : 2;
    }
    b->d_h = b->d_h2 = b->d_gain = b->d_hist = b->d_tw1 = b->d_tw2 = nullptr;
    b->own_design = true;
    b->last_kernel = FASTFIR_KERNEL_NONE;
    b->flo = -1.0; b->fhi = 1.0; b->off = 1.0; b->fs = 1.0;      // fastfir.cpp:126-129
    build_perm(b);
    const size_t hbytes = (size_t)fft_size * 8, histbytes = 2 * (size_t)channels * (fft_size / 2) * 8;
    std::vector<float> tw1(2 * 1024), tw2(2 * 1024);
    for (int i = 0; i < 1024; i++) {
        const double a = kTwoPi * (double)i / (double)fft_size;
        tw1[2 * i] = (float)std::cos(a); tw1[2 * i + 1] = (float)std::sin(a);
    }
    for (int k = 0; k < 32; k++)
        for (int i = 0; i < 32; i++) {
            const double a = kTwoPi * (double)(i * k) / 1024.0;
            tw2[2 * (k * 32 + i)] = (float)std::cos(a); tw2[2 * (k * 32 + i) + 1] = (float)std::sin(a);
        }
    bool ok = hipMalloc((void **)&b->d_h, hbytes) == hipSuccess &&
              hipMalloc((void **)&b->d_h2, hbytes) == hipSuccess && hipMemset(b->d_h2, 0, hbytes) == hipSuccess &&
              hipMalloc((void **)&b->d_gain, hbytes / 2) == hipSuccess && hipMemset(b->d_gain, 0, hbytes / 2) == hipSuccess &&
              hipMalloc((void **)&b->d_hist, histbytes) == hipSuccess &&
              hipMalloc((void **)&b->d_tw1, 8192) == hipSuccess &&
              hipMalloc((void **)&b->d_tw2, 8192) == hipSuccess &&
              hipMemset(b->d_h, 0, hbytes) == hipSuccess &&
              hipMemset(b->d_hist, 0, histbytes) == hipSuccess &&
              hipMemcpy(b->d_tw1, tw1.data(), 8192, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(b->d_tw2, tw2.data(), 8192, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        fail(CSDR_ENOMEM, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        csdr_fastfir_batch_destroy(b);
        return nullptr;
    }
    b->resp.assign(1, std::vector<cd>(fft_size, cd(0, 0)));
    b->job_of.assign(channels, -1);          // (slot 0 alone while the filter is shared)
    b->stale.assign(channels, 0);
    return b;
}

void csdr_fastfir_batch_destroy(csdr_fastfir_batch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->d_h) (void)hipFree(b->d_h);
    if (b->d_h2) (void)hipFree(b->d_h2);
    if (b->d_gain) (void)hipFree(b->d_gain);
    if (b->d_hist) (void)hipFree(b->d_hist);
    if (b->d_tw1) (void)hipFree(b->d_tw1);
    if (b->d_tw2) (void)hipFree(b->d_tw2);
    if (b->ev_design) { (void)hipEventSynchronize(b->ev_design); (void)hipEventDestroy(b->ev_design); }
    if (b->d_win) (void)hipFree(b->d_win);
    if (b->d_tw) (void)hipFree(b->d_tw);
    if (b->d_perm) (void)hipFree(b->d_perm);
    if (b->d_perm2) (void)hipFree(b->d_perm2);
    if (b->d_permg) (void)hipFree(b->d_permg);
    if (b->d_resp) (void)hipFree(b->d_resp);
    delete b;
}

int csdr_fastfir_batch_setup(csdr_fastfir_batch *b, int channel, double flo, double fhi,
                             double offset, double fs)
{
    if (!b || channel < -1 || channel >= b->channels) return fail(CSDR_EINVAL, "bad handle/channel");
    if (!device_ok(b->device)) return CSDR_EHIP;
    if (channel < 0) {
        // shared filter: same early-out as the reference (fastfir.cpp:182-186)
        if (!b->per_channel && flo == b->flo && fhi == b->fhi && offset == b->off && fs == b->fs) return 0;
        b->flo = flo; b->fhi = fhi; b->off = offset; b->fs = fs;
    }
    std::vector<cd> H;
    if (!fastfir_design(b->n, flo, fhi, offset, fs, H))
        return fail(CSDR_EINVAL, "filter parameter error (reference keeps the previous taps)");
    if (channel >= 0 && !b->per_channel) {
        // switch to one filter per channel, seeded with the shared one: a reallocation, once in an object's life -- the
        // only part of a set-up that waits (for this handle's queued patches and design jobs and whatever still reads the
        // old buffer; a shared response that was designed on the device is fetched first: it seeds every mirror row)
        { const int rcm = fetch_mirror(b, 0); if (rcm) return rcm; }
        { const int rcp = flush_control(b, b->last_stream); if (rcp) return rcp; }
        CSDR_HIP(hipDeviceSynchronize());
        // one row per channel in place of the shared row, every row a copy of it
        auto per_channel_rows = [&](float *&d, size_t row) -> int {
            float *rows = nullptr;
            CSDR_HIP(hipMalloc((void **)&rows, row * b->channels));
            for (int c = 0; c < b->channels; c++)
                CSDR_HIP(hipMemcpy((char *)rows + row * c, d, row, hipMemcpyDeviceToDevice));
            CSDR_HIP(hipFree(d));
            d = rows;
            return 0;
        };
        const size_t one = (size_t)b->n * 8;
        { const int rc = per_channel_rows(b->d_h, one); if (rc) return rc; }
        { const int rc = per_channel_rows(b->d_h2, one); if (rc) return rc; }
        { const int rc = per_channel_rows(b->d_gain, one / 2); if (rc) return rc; }
        b->resp.resize(b->channels, b->resp[0]);
        b->per_channel = true;
    }
    if (channel < 0 && b->per_channel) {
        for (int c = 0; c < b->channels; c++) {
            int rc = set_response(b, c, H);
            if (rc) return rc;
        }
    } else {
        int rc = set_response(b, channel < 0 ? 0 : channel, H);
        if (rc) return rc;
    }
    return 1;
}

/* CFastFIR::SetupParameters for many filters of the object at once, designed on the DEVICE: per entry the host does the
 * reference's sanity check and two divisions and queues a job; the next process call launches all of them right behind
 * its patch kernel (see include/cutesdr_mi.h). */
int csdr_fastfir_batch_setup_many(csdr_fastfir_batch *b, int n, const int *channel, const double *flo, const double *fhi,
                                  const double *offset, const double *fs, int *status)
{
    if (!have_device()) return CSDR_EHIP;
    if (!b || n < 0 || (n > 0 && (!channel || !flo || !fhi || !offset || !fs || !status)))
        return fail(CSDR_EINVAL, "bad handle, negative count or null array");
    for (int i = 0; i < n; i++)
        if (channel[i] < -1 || channel[i] >= b->channels) return fail(CSDR_EINVAL, "entry %d: channel %d", i, channel[i]);
    if (n == 0) return CSDR_OK;
    if (!device_ok(b->device)) return CSDR_EHIP;
    { const int rc = design_state(b); if (rc) return rc; }
    for (int i = 0; i < n; i++) {
        const int ch = channel[i];
        if (ch < 0) {
            // shared filter: same early-out as the reference (fastfir.cpp:182-186)
            if (!b->per_channel && flo[i] == b->flo && fhi[i] == b->fhi && offset[i] == b->off && fs[i] == b->fs) { status[i] = 0; continue; }
            b->flo = flo[i]; b->fhi = fhi[i]; b->off = offset[i]; b->fs = fs[i];
        }
        double nfc, nfs;
        if (!fastfir_design_job(flo[i], fhi[i], offset[i], fs[i], nfc, nfs)) { status[i] = CSDR_EINVAL; continue; }   // old taps kept
        if (ch >= 0 && !b->per_channel) {
            // the object turns per-channel by the one-filter call's reallocation path (once in its life: that call
            // designs this entry on the host and waits for the device); the job queued below gives the same filter
            const int rc = csdr_fastfir_batch_setup(b, ch, flo[i], fhi[i], offset[i], fs[i]);
            if (rc < 0) { for (int j = i; j < n; j++) status[j] = rc; return rc; }
        }
        if (ch < 0 && b->per_channel) for (int c = 0; c < b->channels; c++) queue_job(b, c, nfc, nfs);
        else queue_job(b, ch < 0 ? 0 : ch, nfc, nfs);
        status[i] = 1;
    }
    return CSDR_OK;
}

int csdr_fastfir_batch_reset(csdr_fastfir_batch *b)
{
    if (!b) return fail(CSDR_EINVAL, "bad handle");
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipMemset(b->d_hist, 0, 2 * (size_t)b->channels * (b->n / 2) * 8));
    return CSDR_OK;
}

int csdr_fastfir_batch_get_response(csdr_fastfir_batch *b, int channel, double *h_out)
{
    if (!b || !h_out || channel < 0 || channel >= b->channels) return fail(CSDR_EINVAL, "bad argument");
    const int slot = b->per_channel ? channel : 0;
    if (b->stale[slot]) {                  // designed on the device: flush, wait for the object's stream, fetch
        if (!device_ok(b->device)) return CSDR_EHIP;
        const int rc = fetch_mirror(b, slot);
        if (rc) return rc;
    }
    const std::vector<cd> &H = b->resp[slot];
    memcpy(h_out, H.data(), sizeof(cd) * H.size());
    return CSDR_OK;
}

int csdr_fastfir_batch_process(csdr_fastfir_batch *b, const float *d_in, long long in_stride,
                               int n_per_channel, float *d_out, long long out_stride,
                               void *stream, int blocks_per_wg)
{
    if (!b || !d_in || !d_out) return fail(CSDR_EINVAL, "bad handle or null buffer");
    const int L = b->n / 2;
    if (n_per_channel <= 0 || n_per_channel % L != 0)
        return fail(CSDR_EINVAL, "n_per_channel (%d) must be a positive multiple of the hop %d", n_per_channel, L);
    if (in_stride < n_per_channel || out_stride < n_per_channel)
        return fail(CSDR_EINVAL, "channel stride shorter than n_per_channel");
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 15 || (in_stride & 1) || (out_stride & 1))
        return fail(CSDR_EINVAL, "buffers must be 16-byte aligned and strides even");
    // the kernels address a channel row through a 32-bit buffer descriptor range and byte offsets
    if ((long long)n_per_channel * 8 >= (1ll << 31))
        return fail(CSDR_EINVAL, "n_per_channel (%d) too large for one call: at most %d samples", n_per_channel, (1 << 28) - L);
    if (!device_ok(b->device)) return CSDR_EHIP;
    hipStream_t s = (hipStream_t)stream;
    b->last_stream = s;
    { const int rcp = flush_control(b, s); if (rcp) return rcp; }      // responses set up since the last call: patches, then designs
    FastFirArgs a;
    const size_t hist_half = (size_t)b->channels * L * 2;      // floats
    a.in = (const v2f_h *)d_in; a.out = (v2f_h *)d_out;
    a.hist = (const v2f_h *)(b->d_hist + b->hist_cur * hist_half);
    a.hist_next = (v2f_h *)(b->d_hist + (b->hist_cur ^ 1) * hist_half);
    a.h = (const v4f_h *)b->d_h; a.tw1 = (const v2f_h *)b->d_tw1; a.tw2 = (const v2f_h *)b->d_tw2;
    a.gain = nullptr;
    a.in_stride = in_stride; a.out_stride = out_stride;
    a.h_stride = b->per_channel ? b->n / 2 : 0;
    a.channels = b->channels;
    a.nblocks = n_per_channel / L;
    if (blocks_per_wg <= 0) {
        // One workgroup walks a run of consecutive blocks of one channel.  Runs per channel: the count
        // whose workgroups fill whole rounds of the resident slots best (CUs of the device x workgroups per CU
        // at this size: the LDS block is N*8.5 bytes), fewest runs on a tie -- longer runs re-read
        // less overlap.  C3 (256 channels, N=16384): one run of 64 blocks per channel.
        // (N = 4096, pipelined build: two workgroups per CU of two blocks each)
        const long per_cu = b->n >= 16384 ? 1 : (b->n >= 8192 ? 2 : (b->n >= 4096 ? 4 : 8));   // (4096 / 2048: 2 workgroups x 2 / 4 blocks)
        const long slots = (long)b->cus * per_cu;
        long best_runs = 1; double best_eff = -1.0;
        const long max_runs = std::min<long>(a.nblocks, std::max<long>(1, 4 * ((slots + b->channels - 1) / b->channels)));
        for (long runs = 1; runs <= max_runs; runs++) {
            const long wgs = runs * b->channels;
            const double eff = (double)wgs / (double)(((wgs + slots - 1) / slots) * slots);
            if (eff > best_eff + 1e-9) { best_eff = eff; best_runs = runs; }
        }
        blocks_per_wg = (int)((a.nblocks + best_runs - 1) / best_runs);
    }
    if (blocks_per_wg > a.nblocks) blocks_per_wg = a.nblocks;
    a.blocks_per_run = blocks_per_wg;
    a.runs = (a.nblocks + blocks_per_wg - 1) / blocks_per_wg;
    a.dbg_stage = b->dbg_stage; a.dbg = (v2f_h *)b->dbg_out;
    if (b->variant >= 2) {
        a.h = (const v4f_h *)b->d_h2;         // its own H order
        // N = 16384 on the library's own (linear-phase) designs: real gains and a quarter-block shift instead of complex H
        if (b->log2n == 14 && b->own_design) a.gain = (const v4f_h *)b->d_gain;
        b->last_kernel = FASTFIR_KERNEL_NONE;
        CSDR_HIP(fastfir2_launch(b->log2n, a, s, &b->last_kernel));     // any block count (pairs, then a single trailing block)
    }
    else {
        b->last_kernel = FASTFIR_KERNEL_NONE;
        CSDR_HIP(fastfir_launch(b->log2n, a, s));
        b->last_kernel = FASTFIR_KERNEL_GENERIC;
    }
    b->hist_cur ^= 1;        // the kernel left this call's tail in the other half
    return CSDR_OK;
}

/* internal (csdr_demod_batch_set_demod moving a receiver to another plan group): row `sr` of `src` continues as row
 * `dr` of `dst` -- the overlap of the stream so far and the frequency response in use (a later SetupParameters with a
 * parameter error keeps it, fastfir.cpp:195-203).  Same FFT size, both handles idle. */
int csdr__fastfir_batch_copy_row(csdr_fastfir_batch *dst, int dr, csdr_fastfir_batch *src, int sr)
{
    if (!dst || !src || dst->n != src->n || dr < 0 || dr >= dst->channels || sr < 0 || sr >= src->channels)
        return fail(CSDR_EINVAL, "bad argument");
    if (!device_ok(dst->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());
    const int L = dst->n / 2;
    const size_t shalf = (size_t)src->channels * L * 2, dhalf = (size_t)dst->channels * L * 2;
    CSDR_HIP(hipMemcpy(dst->d_hist + dst->hist_cur * dhalf + (size_t)dr * L * 2,
                       src->d_hist + src->hist_cur * shalf + (size_t)sr * L * 2, (size_t)L * 8, hipMemcpyDeviceToDevice));
    const int sslot = src->per_channel ? sr : 0;
    { const int rcm = fetch_mirror(src, sslot); if (rcm) return rcm; }      // the response in use may exist on the device only
    const std::vector<cd> &H = src->resp[sslot];
    if (dst->channels > 1 && !dst->per_channel) return fail(CSDR_ESTATE, "destination rows share one filter");
    const int slot = dst->per_channel ? dr : 0;
    int rc = set_response(dst, slot, H);
    if (rc) return rc;
    dst->own_design = dst->own_design && src->own_design;      // (the gains set_response derived hold for a design only)
    dst->flo = dst->fhi = dst->off = dst->fs = std::nan("");      // parameters unknown: the next setup always designs
    return CSDR_OK;
}

/* test-only hook, not part of the public ABI: choose the kernel build of this object (A/B timing in one process) */
int csdr__fastfir_set_variant(csdr_fastfir_batch *b, int variant)
{
    if (!b || (variant != 0 && variant != 2)) return CSDR_EINVAL;
    b->variant = variant;
    return CSDR_OK;
}

/* test-only hook, not part of the public ABI: say whether the object's responses are all the library's own design (the
 * flag a setter of raw responses would clear): 0 sends a 16384-point launch to the pipelined kernel on complex H */
int csdr__fastfir_set_own_design(csdr_fastfir_batch *b, int own)
{
    if (!b) return CSDR_EINVAL;
    b->own_design = own != 0;
    return CSDR_OK;
}

/* test-only hook, not part of the public ABI: *kernel = which kernel the most recent process call launched (FastFirKernel,
 * fastfir_kernels.h: -1 none yet, 0 generic, 1 pipelined on complex H, 2 pipelined on real gains -- written by the code
 * that chooses), *twreg = the K1_TWREG the pipelined kernels were compiled with */
int csdr__fastfir_last_kernel(const csdr_fastfir_batch *b, int *kernel, int *twreg)
{
    if (!b || !kernel || !twreg) return CSDR_EINVAL;
    *kernel = b->last_kernel;
    *twreg = fastfir2_twreg();
    return CSDR_OK;
}

/* test-only hook, not part of the public ABI: both halves of the ping-pong history to the host, 2 x [channels][n/2] complex
 * fp32 as they lie on the device, and *cur = the half the next call reads (the one the last call wrote) */
int csdr__fastfir_read_history(csdr_fastfir_batch *b, float *out, int *cur)
{
    if (!b || !out || !cur) return CSDR_EINVAL;
    if (!device_ok(b->device)) return CSDR_EHIP;
    CSDR_HIP(hipDeviceSynchronize());
    CSDR_HIP(hipMemcpy(out, b->d_hist, 2 * (size_t)b->channels * (b->n / 2) * 8, hipMemcpyDeviceToHost));
    *cur = b->hist_cur;
    return CSDR_OK;
}

/* test-only hook, not part of the public ABI: dump the LDS image after a pass */
int csdr__dbg_fastfir_stage(csdr_fastfir_batch *b, int stage, float *d_dbg)
{
    if (!b) return CSDR_EINVAL;
    b->dbg_stage = stage; b->dbg_out = d_dbg;
    return CSDR_OK;
}

/* ---------------- single-channel host form: CFastFIR drop-in ---------------- */
}  // extern "C"

struct csdr_fastfir {
    csdr_fastfir_batch *b;
    int n, pending;                  // pending < n/2 input samples not yet processed (they sit at the front of pin_in)
    PinnedBuf pin_in, pin_out;       // page-locked fp32 staging, both directions
    hipStream_t s = nullptr;         // the object's stream: H2D copy, filter, D2H copy in order, ONE wait per call
    float *d_in, *d_out;
    size_t cap;                      // device staging capacity in samples
};

static int ensure_cap(csdr_fastfir *f, size_t samples)
{
    if (samples <= f->cap) return CSDR_OK;
    if (f->d_in) (void)hipFree(f->d_in);
    if (f->d_out) (void)hipFree(f->d_out);
    f->d_in = f->d_out = nullptr; f->cap = 0;
    CSDR_HIP(hipMalloc((void **)&f->d_in, samples * 8));
    CSDR_HIP(hipMalloc((void **)&f->d_out, samples * 8));
    f->cap = samples;
    return CSDR_OK;
}

extern "C" {

csdr_fastfir *csdr_fastfir_create(int device, int fft_size)
{
    csdr_fastfir_batch *b = csdr_fastfir_batch_create(device, 1, fft_size);
    if (!b) return nullptr;
    csdr_fastfir *f = new csdr_fastfir();
    f->b = b; f->n = fft_size; f->pending = 0; f->d_in = f->d_out = nullptr; f->cap = 0;
    if (hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) != hipSuccess) { csdr_fastfir_destroy(f); fail(CSDR_EHIP, "stream creation failed"); return nullptr; }
    return f;
}

void csdr_fastfir_destroy(csdr_fastfir *f)
{
    if (!f) return;
    (void)hipSetDevice(f->b->device);
    if (f->d_in) (void)hipFree(f->d_in);
    if (f->d_out) (void)hipFree(f->d_out);
    if (f->s) { (void)hipStreamSynchronize(f->s); (void)hipStreamDestroy(f->s); }
    csdr_fastfir_batch_destroy(f->b);
    delete f;
}

int csdr_fastfir_setup(csdr_fastfir *f, double flo, double fhi, double offset, double fs)
{
    if (!f) return fail(CSDR_EINVAL, "bad handle");
    return csdr_fastfir_batch_setup(f->b, -1, flo, fhi, offset, fs);
}

int csdr_fastfir_process(csdr_fastfir *f, int n, const double *in_iq, double *out_iq)
{
    if (!f || n < 0 || (n > 0 && (!in_iq || !out_iq))) return fail(CSDR_EINVAL, "bad argument");
    if (n == 0) return 0;
    if (!device_ok(f->b->device)) return CSDR_EHIP;
    const int L = f->n / 2;
    // append to the pending (not yet hop-complete) samples, fp64 -> fp32 at the boundary, straight into pinned memory
    int rc = f->pin_in.reserve(2 * ((size_t)f->pending + n));
    if (rc) return rc;
    cvt_to_f32(f->pin_in.p + 2 * (size_t)f->pending, in_iq, 2 * (size_t)n);
    const int avail = f->pending + n;
    const int nproc = (avail / L) * L;
    if (nproc == 0) { f->pending = avail; return 0; }
    // (an error below keeps the call's samples: they are appended to the pending ones, and a later call retries the hops)
    if ((rc = ensure_cap(f, (size_t)nproc))) { f->pending = avail; return rc; }
    if ((rc = f->pin_out.reserve(2 * (size_t)nproc))) { f->pending = avail; return rc; }
    CSDR_HIP(hipMemcpyAsync(f->d_in, f->pin_in.p, (size_t)nproc * 8, hipMemcpyHostToDevice, f->s));
    rc = csdr_fastfir_batch_process(f->b, f->d_in, nproc, nproc, f->d_out, nproc, (void *)f->s, 0);
    if (rc) {                                             // the copy above may still be reading the pinned buffer
        (void)hipStreamSynchronize(f->s);
        f->pending = avail;
        return rc;
    }
    CSDR_HIP(hipMemcpyAsync(f->pin_out.p, f->d_out, (size_t)nproc * 8, hipMemcpyDeviceToHost, f->s));
    CSDR_HIP(hipStreamSynchronize(f->s));
    cvt_to_f64(out_iq, f->pin_out.p, 2 * (size_t)nproc);
    f->pending = avail - nproc;
    if (f->pending > 0) memmove(f->pin_in.p, f->pin_in.p + 2 * (size_t)nproc, 2 * (size_t)f->pending * sizeof(float));
    return nproc;
}

}  // extern "C"
