// capi_plotter.hip -- C ABI of the batch plotter: V views, each one CPlotter's display state (reference gui/plotter.cpp:
// constructor :100-114, resizeEvent :374-389, draw :408-480, DrawOverlay's m_MindB :597; setters gui/plotter.h:32-44),
// over the rows of a csdr_fft_batch.  State and ordering as capi_scope.hip: the settings (pl::View) live on the host
// behind one mutex, a setter touches no device memory and waits for nothing, and what it changed travels with the next
// draw through a ring of pinned parameter slots copied on the caller's stream; the readers wait for the event of the
// last call only, on a stream of the object's own.  On the device live the trace and the ring of waterfall lines of
// every view (one allocation per view, made by resize / set_percent_2d) and the three pen words (pl::ViewState).
//
// The waterfall is never copied or cleared by a draw or a resize: the host keeps the ring's head and the number of
// lines drawn since the last resizeEvent, hands the draw the row that receives the new line, and the readers show
// black below the drawn lines -- m_WaterfallPixmap.fill(Qt::black) costs nothing and is in order by construction,
// because head and count travel with each call.
#include "capi_common.hpp"
#include "capi_internal.hpp"
#include "plotter_kernels.h"
#include "spectrum_kernels.h"
#include <mutex>
#include <vector>

using namespace csdr;
using pl::RowParam;
using pl::View;
using pl::ViewParam;
using pl::ViewState;

namespace {
constexpr int kRing = 16;
static_assert(sizeof(RowParam) <= sizeof(ViewParam), "the readers' rows travel in the draw's slots");
}

struct csdr_plotter_batch {
    int device = 0, views = 0;
    std::vector<View> v;
    std::vector<unsigned *> buf;         // per view: trace [w], then the ring [wf_h][w]
    std::vector<size_t> cap;             // words
    std::mutex mu;                       // setters, draw and the readers exclude each other
    ViewParam *h_par[kRing] = {};        // pinned
    ViewParam *d_par[kRing] = {};
    hipEvent_t ev[kRing] = {};
    bool busy[kRing] = {};
    int next = 0, last = -1;             // last: the slot whose event marks the end of the latest launch
    ViewState *d_state = nullptr;
    unsigned *d_pal = nullptr;           // m_ColorTbl
    hipStream_t rd = nullptr;            // the readers' stream
};

static int plb_alloc(csdr_plotter_batch *p)
{
    const size_t bytes = sizeof(ViewParam) * (size_t)p->views;
    for (int i = 0; i < kRing; i++) {
        if (hipHostMalloc((void **)&p->h_par[i], bytes, hipHostMallocDefault) != hipSuccess)
            return fail(CSDR_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        CSDR_HIP(hipMalloc((void **)&p->d_par[i], bytes));
        CSDR_HIP(hipEventCreateWithFlags(&p->ev[i], hipEventDisableTiming));
    }
    CSDR_HIP(hipMalloc((void **)&p->d_state, sizeof(ViewState) * (size_t)p->views));
    CSDR_HIP(hipMemset(p->d_state, 0, sizeof(ViewState) * (size_t)p->views));      // :107-108
    CSDR_HIP(hipMalloc((void **)&p->d_pal, 256 * sizeof(unsigned)));
    unsigned pal[256];
    for (int i = 0; i < 256; i++) pal[i] = plotter_color(i);
    CSDR_HIP(hipMemcpy(p->d_pal, pal, sizeof(pal), hipMemcpyHostToDevice));
    CSDR_HIP(hipStreamCreateWithFlags(&p->rd, hipStreamNonBlocking));
    return CSDR_OK;
}

// a free slot of the pinned ring: waits, on that launch's event only, when the launch kRing before has not finished
static int plb_slot(csdr_plotter_batch *p, int *slot)
{
    *slot = p->next;
    if (p->busy[*slot]) { CSDR_HIP(hipEventSynchronize(p->ev[*slot])); p->busy[*slot] = false; }
    return CSDR_OK;
}
static int plb_sent(csdr_plotter_batch *p, int slot, hipStream_t st)
{
    CSDR_HIP(hipEventRecord(p->ev[slot], st));
    p->busy[slot] = true;
    p->last = slot;
    p->next = (slot + 1) % kRing;
    return CSDR_OK;
}
// `st` behind the object's latest launch, whatever stream that ran on
static int plb_follow(csdr_plotter_batch *p, hipStream_t st)
{
    if (p->last >= 0) CSDR_HIP(hipStreamWaitEvent(st, p->ev[p->last], 0));
    return CSDR_OK;
}

template <class F> static int plb_each(csdr_plotter_batch *p, int view, F f)
{
    if (!p || view >= p->views) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(p->mu);
    for (int i = view < 0 ? 0 : view; i < (view < 0 ? p->views : view + 1); i++) f(p->v[i]);
    return CSDR_OK;
}

// resizeEvent / SetPercent2DScreen: the views' new geometry, with room for trace and ring made first
template <class F> static int plb_reshape(csdr_plotter_batch *p, int view, F f)
{
    if (!p || view >= p->views) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(p->mu);
    const int lo = view < 0 ? 0 : view, hi = view < 0 ? p->views : view + 1;
    std::vector<unsigned *> grown((size_t)(hi - lo), nullptr);          // every new allocation first: a failure changes nothing
    std::vector<size_t> need((size_t)(hi - lo), 0);
    bool any = false;
    for (int i = lo; i < hi; i++) {
        View t = p->v[i];
        f(t);
        need[i - lo] = (size_t)t.w * (size_t)(1 + t.wf_h);
        if (need[i - lo] <= p->cap[i]) continue;
        int rc = CSDR_OK;
        if (!have_device()) rc = CSDR_EHIP;
        else if (hipSetDevice(p->device) != hipSuccess || hipMalloc((void **)&grown[i - lo], need[i - lo] * sizeof(unsigned)) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(CSDR_ENOMEM, "hipMalloc(%zu) failed", need[i - lo] * sizeof(unsigned));
        }
        if (rc) {
            for (unsigned *q : grown)
                if (q) (void)hipFree(q);
            return rc;
        }
        any = true;
    }
    if (any && p->last >= 0 && p->busy[p->last] && hipEventSynchronize(p->ev[p->last]) != hipSuccess) {   // launches in flight use the old rows
        for (unsigned *q : grown)
            if (q) (void)hipFree(q);
        return fail(CSDR_EHIP, "hipEventSynchronize failed");
    }
    for (int i = lo; i < hi; i++) {
        if (grown[i - lo]) {
            if (p->buf[i]) (void)hipFree(p->buf[i]);
            p->buf[i] = grown[i - lo]; p->cap[i] = need[i - lo];
            p->v[i].traced = 0;                          // the old trace went with the old rows; f never sets it
        }
        f(p->v[i]);
    }
    return CSDR_OK;
}

static int plb_view_ok(csdr_plotter_batch *p, int view)
{
    if (!p || view < 0 || view >= p->views) return fail(CSDR_EINVAL, "bad argument");
    return CSDR_OK;
}

// the device readers: one row per view through plotter_rows_kernel, the rows' sources travelling as a draw's views do
template <class F> static int plb_rows(csdr_plotter_batch *p, unsigned *d_out, long long stride, int *d_pen, void *stream, F row)
{
    if (!have_device()) return CSDR_EHIP;
    if (!p || !d_out) return fail(CSDR_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(p->mu);
    int slot = 0, max_w = 0;
    RowParam *hp = nullptr;
    for (int pass = 0; pass < 2; pass++) {               // pass 0 only measures: a refusal changes nothing
        for (int i = 0; i < p->views; i++) {
            const RowParam r = row(p->v[i], p->buf[i]);
            if (pass) hp[i] = r;
            else if (r.w > max_w) max_w = r.w;
        }
        if (pass) break;
        if (stride < max_w) return fail(CSDR_EINVAL, "stride must be >= the widest view, %d", max_w);
        CSDR_HIP(hipSetDevice(p->device));
        if (int rc = plb_slot(p, &slot)) return rc;
        hp = (RowParam *)p->h_par[slot];
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = plb_follow(p, st)) return rc;
    CSDR_HIP(hipMemcpyAsync(p->d_par[slot], hp, sizeof(RowParam) * (size_t)p->views, hipMemcpyHostToDevice, st));
    CSDR_HIP(pl::plotter_rows_launch((const RowParam *)p->d_par[slot], p->views, max_w, d_out, stride, p->d_state, d_pen, st));
    return plb_sent(p, slot, st);
}

extern "C" {

csdr_plotter_batch *csdr_plotter_batch_create(int device, int views)
{
    if (views < 1 || views > 4096) { fail(CSDR_EINVAL, "views 1..4096"); return nullptr; }
    if (!device_ok(device)) return nullptr;
    csdr_plotter_batch *p = new csdr_plotter_batch();
    p->device = device; p->views = views;
    p->v.resize((size_t)views);
    for (int i = 0; i < views; i++) p->v[i].row = i;
    p->buf.assign((size_t)views, nullptr);
    p->cap.assign((size_t)views, 0);
    if (plb_alloc(p) != CSDR_OK) {
        const std::string e = last_error_ref();
        csdr_plotter_batch_destroy(p);
        fail(CSDR_EHIP, "%s", e.c_str());
        return nullptr;
    }
    return p;
}
void csdr_plotter_batch_destroy(csdr_plotter_batch *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    for (int i = 0; i < kRing; i++) {
        if (p->busy[i]) (void)hipEventSynchronize(p->ev[i]);          // its launch still reads the slot
        if (p->ev[i]) (void)hipEventDestroy(p->ev[i]);
        if (p->h_par[i]) (void)hipHostFree(p->h_par[i]);
        if (p->d_par[i]) (void)hipFree(p->d_par[i]);
    }
    if (p->rd) { (void)hipStreamSynchronize(p->rd); (void)hipStreamDestroy(p->rd); }
    if (p->d_state) (void)hipFree(p->d_state);
    if (p->d_pal) (void)hipFree(p->d_pal);
    for (unsigned *q : p->buf)
        if (q) (void)hipFree(q);
    delete p;
}
int csdr_plotter_batch_set_source(csdr_plotter_batch *p, int view, int fft_row)
{
    if (fft_row < 0) return fail(CSDR_EINVAL, "row >= 0");
    return plb_each(p, view, [=](View &k) { k.row = fft_row; });
}
int csdr_plotter_batch_resize(csdr_plotter_batch *p, int view, int w, int h)
{
    if (w < 0 || w > pl::kMaxW || h < 0 || h > pl::kMaxW) return fail(CSDR_EINVAL, "size: 0 <= w, h <= 4096");
    return plb_reshape(p, view, [=](View &k) { k.resize(w, h); });
}
int csdr_plotter_batch_set_percent_2d(csdr_plotter_batch *p, int view, int percent)
{
    if (percent < 0 || percent > 100) return fail(CSDR_EINVAL, "percent 0..100");
    return plb_reshape(p, view, [=](View &k) { k.set_percent(percent); });
}
int csdr_plotter_batch_set_span(csdr_plotter_batch *p, int view, int span_hz)
{ return plb_each(p, view, [=](View &k) { k.span = span_hz; }); }
int csdr_plotter_batch_set_max_db(csdr_plotter_batch *p, int view, int max_db)
{ return plb_each(p, view, [=](View &k) { k.max_db = max_db; }); }
int csdr_plotter_batch_set_db_step(csdr_plotter_batch *p, int view, int step)
{
    if (step < 1) return fail(CSDR_EINVAL, "dB step >= 1");
    return plb_each(p, view, [=](View &k) { k.step = step; });
}
int csdr_plotter_batch_update_overlay(csdr_plotter_batch *p, int view)
{ return plb_each(p, view, [](View &k) { k.update_overlay(); }); }
int csdr_plotter_batch_set_ad_overload(csdr_plotter_batch *p, int view, int on)
{ return plb_each(p, view, [=](View &k) { k.ad_cmd = on ? 1 : 0; }); }
int csdr_plotter_batch_set_running(csdr_plotter_batch *p, int view, int on)
{ return plb_each(p, view, [=](View &k) { k.running = on ? 1 : 0; }); }

// draw of every view (emitted_only: of the running views whose row used a frame in f's last put; the others are skipped
// whole, a pending pen command included)
static int plb_draw(csdr_plotter_batch *p, csdr_fft_batch *f, void *stream, bool emitted_only)
{
    if (!have_device()) return CSDR_EHIP;
    if (!p || !f) return fail(CSDR_EINVAL, "bad argument");
    FftView fv;
    if (int rc = csdr__fft_batch_view(f, &fv)) return rc;
    if (fv.device != p->device) return fail(CSDR_EINVAL, "views on device %d over spectra on device %d", p->device, fv.device);
    std::lock_guard<std::mutex> lock(p->mu);
    for (int i = 0; i < p->views; i++)
        if (p->v[i].running && p->v[i].row >= fv.channels)
            return fail(CSDR_EINVAL, "view %d plots row %d of %d", i, p->v[i].row, fv.channels);
    std::vector<int> emits;
    if (emitted_only) {
        emits.resize((size_t)fv.channels);
        if (int rc = csdr_fft_batch_get_emits(f, emits.data())) return rc;
    }
    CSDR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;
    if (int rc = plb_slot(p, &slot)) return rc;
    ViewParam *hp = p->h_par[slot];
    std::vector<View> nv = p->v;                         // the views after the call; kept only when it went out
    pl::DrawArgs a;
    a.par = p->d_par[slot]; a.count = 0; a.state = p->d_state; a.ave = fv.d_ave; a.over = fv.d_over; a.palette = p->d_pal;
    a.n = fv.size; a.invert = fv.invert; a.max_tiles = 1;
    int drawn = 0;
    for (int i = 0; i < p->views; i++) {
        View &k = nv[i];
        if (!k.running && k.ad_cmd < 0) continue;
        if (emitted_only && !(k.running && emits[k.row] > 0)) continue;
        ViewParam &q = hp[a.count++];
        memset(&q, 0, sizeof(q));
        q.view = i; q.row = k.running ? k.row : 0; q.draws = k.running; q.ad_cmd = k.ad_cmd; q.group = 1;
        k.ad_cmd = -1;
        if (!k.running || k.w < 1) continue;             // w == 0: no pixmaps, the pen step only
        drawn++;
        k.scroll(); k.traced = 1;
        const pl::Map m = pl::make_map(fv.size, fv.fs, k.span, k.w);
        q.w = k.w; q.h2d = k.h2d; q.wf_h = k.wf_h; q.head = k.head;
        q.bin_min = m.bin_min; q.bin_max = m.bin_max; q.bins = m.bins; q.group = pl::group_lanes(m, k.w);
        q.gain = pl::db_gain(k.max_db, k.min_db); q.off = pl::db_off(k.max_db);
        q.smallest = pl::run_keeps_smallest(k.max_db, k.min_db);
        q.trace = (int *)p->buf[i]; q.ring = p->buf[i] + k.w;
        const int per = 256 / q.group, tiles = (k.w + per - 1) / per;
        if (tiles > a.max_tiles) a.max_tiles = tiles;
    }
    if (a.count == 0) return 0;
    if (int rc = plb_follow(p, st)) return rc;           // trace, rings and pen words follow the previous call, whatever its stream
    CSDR_HIP(hipMemcpyAsync(p->d_par[slot], hp, sizeof(ViewParam) * (size_t)a.count, hipMemcpyHostToDevice, st));
    CSDR_HIP(pl::plotter_draw_launch(a, st));
    if (int rc = plb_sent(p, slot, st)) return rc;
    p->v.swap(nv);
    return drawn;
}
int csdr_plotter_batch_draw(csdr_plotter_batch *p, csdr_fft_batch *f, void *stream) { return plb_draw(p, f, stream, false); }
int csdr_plotter_batch_draw_emitted(csdr_plotter_batch *p, csdr_fft_batch *f, void *stream) { return plb_draw(p, f, stream, true); }

int csdr_plotter_batch_get_geometry(csdr_plotter_batch *p, int view, int *w, int *h2d, int *wf_h, int *min_db)
{
    if (int rc = plb_view_ok(p, view)) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    const View &k = p->v[view];
    if (w) *w = k.w;
    if (h2d) *h2d = k.h2d;
    if (wf_h) *wf_h = k.wf_h;
    if (min_db) *min_db = k.min_db;
    return CSDR_OK;
}
int csdr_plotter_batch_get_trace(csdr_plotter_batch *p, int view, int *out_y, int *pen_red)
{
    if (!have_device()) return CSDR_EHIP;
    if (int rc = plb_view_ok(p, view)) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    const View &k = p->v[view];
    if (k.w > 0 && !out_y) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP(hipSetDevice(p->device));
    if (int rc = plb_follow(p, p->rd)) return rc;
    ViewState st;
    if (k.traced) CSDR_HIP(hipMemcpyAsync(out_y, p->buf[view], sizeof(int) * (size_t)k.w, hipMemcpyDeviceToHost, p->rd));
    else if (k.w > 0) memset(out_y, 0, sizeof(int) * (size_t)k.w);
    CSDR_HIP(hipMemcpyAsync(&st, p->d_state + view, sizeof(st), hipMemcpyDeviceToHost, p->rd));
    CSDR_HIP(hipStreamSynchronize(p->rd));
    if (pen_red) *pen_red = st.pen;
    return k.w;
}
int csdr_plotter_batch_get_waterfall(csdr_plotter_batch *p, int view, unsigned int *out_rgb)
{
    if (!have_device()) return CSDR_EHIP;
    if (int rc = plb_view_ok(p, view)) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    const View &k = p->v[view];
    const size_t w = (size_t)k.w;
    if (w == 0 || k.wf_h == 0) return k.wf_h;
    if (!out_rgb) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP(hipSetDevice(p->device));
    if (int rc = plb_follow(p, p->rd)) return rc;
    const unsigned *ring = p->buf[view] + w;
    const int first = k.head + k.filled <= k.wf_h ? k.filled : k.wf_h - k.head;      // lines up to the ring's end
    if (first > 0) CSDR_HIP(hipMemcpyAsync(out_rgb, ring + (size_t)k.head * w, first * w * 4, hipMemcpyDeviceToHost, p->rd));
    if (k.filled > first) CSDR_HIP(hipMemcpyAsync(out_rgb + first * w, ring, (k.filled - first) * w * 4, hipMemcpyDeviceToHost, p->rd));
    for (size_t i = (size_t)k.filled * w; i < (size_t)k.wf_h * w; i++) out_rgb[i] = pl::kBlack;
    CSDR_HIP(hipStreamSynchronize(p->rd));
    return k.wf_h;
}

int csdr_plotter_batch_get_traces_all(csdr_plotter_batch *p, int *d_y, long long stride, int *d_pen, void *stream)
{
    return plb_rows(p, (unsigned *)d_y, stride, d_pen, stream, [](const View &k, const unsigned *buf) {
        return RowParam{k.traced ? buf : nullptr, k.w, 0u}; });
}
int csdr_plotter_batch_get_lines_all(csdr_plotter_batch *p, unsigned int *d_rgb, long long stride, void *stream)
{
    return plb_rows(p, d_rgb, stride, nullptr, stream, [](const View &k, const unsigned *buf) {
        return RowParam{k.filled > 0 ? buf + (size_t)k.w * (size_t)(1 + k.head) : nullptr, k.wf_h > 0 ? k.w : 0, pl::kBlack}; });
}
int csdr_plotter_batch_get_waterfall_dev(csdr_plotter_batch *p, int view, unsigned int *d_rgb, void *stream)
{
    if (!have_device()) return CSDR_EHIP;
    if (int rc = plb_view_ok(p, view)) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    const View &k = p->v[view];
    if (k.w == 0 || k.wf_h == 0) return k.wf_h;
    if (!d_rgb) return fail(CSDR_EINVAL, "bad argument");
    CSDR_HIP(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    int slot;                                            // for its event: a later draw must not overwrite a line being read
    if (int rc = plb_slot(p, &slot)) return rc;
    if (int rc = plb_follow(p, st)) return rc;
    CSDR_HIP(pl::plotter_unroll_launch(p->buf[view] + k.w, k.w, k.wf_h, k.head, k.filled, d_rgb, st));
    if (int rc = plb_sent(p, slot, st)) return rc;
    return k.wf_h;
}

}  // extern "C"
