/*
 * fr_ctx.h — internal (C++) state shared by the translation units of the C ABI:
 *   fr_api.hip    the single-device entry points (get_image / get_recursive_pixel / recursive)
 *   fr_host.hip   getting a finished image from HBM into the caller's Vec<RGB>-shaped host buffer
 *   fr_multi.hip  get_image across a set of devices from ONE process (src/lib.rs:253 has one caller)
 * Not installed; the public boundary is include/fractal_hip.h.
 */
#ifndef FR_CTX_H
#define FR_CTX_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fractal_hip.h"
#include "fr_kernels.h"
#include "fr_wide.h"

namespace fr {

/* ---- errors: code + thread-local message (fr_last_error) ----------------------------------- */
int fail(int code, const char *what);
int fail(int code, const std::string &what);
int fail_hip(hipError_t e, const char *what);
const std::string &last_error();

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return ::fr::fail_hip(e_, #expr); \
    } while (0)

/* ---- implementation selectors of one render (fr_render_opts resolved against the defaults) --- */
struct Opts {
    int tile = 0;
    int loop_mode = -1;
    int palette = 1;
    int cycle_shortcut = 0;
    int refill_minrun = -1, refill_quit16 = -1; /* -1: each kernel's own default */
    int colour_filter = 1;
    /* the default dispatch's choice of kernel, when the caller has made it for a whole image that it renders in several
     * launches (bands of the host path, chunks of the multi-device path): -2 = decide per launch (fr_api.hip:
     * choose_kernel), else choose_kernel's answer (-1 none, 0 strips, 1 two passes, 2 first pass alone) and its
     * one-strip-per-workgroup flag */
    int kernel_hint = -2;
    bool one_band = false;
    bool no_spec = false; /* with kernel_hint >= 0: the view's statistics say nothing stays — no speculative blocks (fr_api.hip: decide_from_sample) */
    uint32_t strip_tiles = 0; /* with kernel_hint >= 0: the strip length the view's statistics call for (0 = by launch size) */
    /* a non-blocking view sample the caller still has to post BEHIND its render (Ctx::post_sample): slot index, -1 none */
    int pending_sample = -1;
};
Opts default_opts();                             /* what the fr_set_* calls have set */
int resolve_opts(const fr_render_opts *o, Opts &out); /* NULL = defaults; validates */

/* ---- one logical device: a HIP device + the library's streams and scratch on it -------------- */
struct Scratch {
    void *ptr = nullptr;
    size_t cap = 0;
};

/* Palette scratch for smooth == false renders: a small ring of device buffers owned by the context
 * (no allocation on the render path, usable from any stream of that device).  A slot is handed out
 * only after the event recorded behind its last user has completed. */
struct PaletteSlot {
    uint32_t *dev = nullptr; /* FR_MAX_PALETTE_ENTRIES palette words, then the work-queue kernel's claim counters */
    hipEvent_t done = nullptr;
    bool pending = false; /* `done` was recorded and not yet waited for */
    bool busy = false;    /* a thread is between acquire and its event record */
};
constexpr int kPaletteSlots = 16;

/* Survivor lists of the two-pass render (fr_kernels.hip): a ring of three buffers cut from ONE device allocation
 * (Ctx::surv_block), made with the context for frames up to 3840 x 2160 and re-made only for a launch that needs more
 * than a slot holds — the one allocation the device-pointer entry points can block on (a larger two-pass frame than
 * any before); handed out like the palette slots. */
struct SurvSlot {
    void *dev = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false, busy = false;
};
constexpr int kSurvSlots = 3;

struct PtOrbit;  /* fr_pt.hip */
struct BlaTable; /* fr_bla.hip */

struct Ctx {
    int hip_device = -1;
    std::mutex mu; /* serialises the host-buffer entry points (they share streams + scratch) */
    hipStream_t stream = nullptr;      /* kernels of the host-buffer entry points */
    hipStream_t stream2 = nullptr;     /* band / chunk kernels alternate between stream and stream2 */
    hipStream_t copy_stream = nullptr; /* D2H / peer copies, overlapped with the next band's kernel */
    std::vector<hipEvent_t> events;
    Scratch rgb, z, iters, misc;
    Scratch ss_work; /* fr_ss.hip: the host road's band workspace (at most 256 MiB) / fr_box_filter_rgb8's source */
    PaletteSlot palette_slots[kPaletteSlots];
    SurvSlot surv_slots[kSurvSlots];
    void *surv_block = nullptr; /* kSurvSlots x surv_slot_cap bytes */
    size_t surv_slot_cap = 0;
    bool surv_regrowing = false; /* a thread is re-making the ring with palette_mu dropped (acquire_surv) */
    uint32_t *palette_block = nullptr; /* kPaletteSlots slots, allocated with the context */
    /* view samples (fr_api.hip: choose_kernel).  Large launches: a BLOCKING sample on aux_stream — a stream of its own: the
     * sample must not wait behind whatever the caller has queued on its stream.  GUI-sized launches: a NON-BLOCKING one on
     * aux2_stream, behind the render of the frame it was asked for (an event of the caller's stream), read by the NEXT
     * frame of the same view.  Each has its own eight device counters; every remembered view its own eight result words
     * (host-mapped; the kernel writes the view's key into the eighth LAST), plus one set for fr_debug_sample_view. */
    hipStream_t aux_stream = nullptr, aux2_stream = nullptr;
    unsigned long long *sample_counters = nullptr; /* device: 2 x 8 words */
    unsigned long long *sample_result = nullptr;   /* pinned host memory, mapped: (kViewChoices + 1) x 8 words */
    std::mutex sample_mu; /* the view table AND the order of launches on the two sample streams */
    struct ViewChoice {
        uint64_t key = 0;
        int state = 0; /* 0 free, 1 a sample is (about to be) in flight, 2 decided */
        int two_pass = -1; /* -1 no opinion, 0 strips, 1 two passes, 2 the first pass alone */
        bool one_band = false;
        bool no_spec = false;
        uint32_t strip_tiles = 0;
        double lane_fraction = 0.0;
        fr_kparams grid; /* state 1: what the sample is launched with */
        int precision = 0;
        hipEvent_t after = nullptr; /* recorded on the caller's stream behind the render the sample follows */
    };
    static constexpr int kViewChoices = 32; /* (a rank of a multi-GPU run renders its share in up to a dozen chunk launches per image, each its own view) */
    ViewChoice view_choices[kViewChoices];
    unsigned view_next = 0;
    /* enqueue slot `idx`'s sample behind everything `stream` holds now; never blocks, never fails the render (a sample that
     * cannot be posted frees its slot) */
    void post_sample(int idx, hipStream_t stream);
    std::mutex palette_mu; /* guards both rings */
    std::condition_variable slot_cv; /* a slot of either ring was released */
    unsigned palette_next = 0, surv_next = 0;

    /* GUI-sized host-buffer renders (fr_host.hip: host_render_staged): a pinned staging buffer of the library's own — the
     * device never maps, pins or DMAs into the CALLER's pages for frames up to 3840 x 2160 RGBA — and a few copy threads */
    void *stage = nullptr;       /* pinned host memory (hipHostMalloc, mapped) */
    void *stage_dev = nullptr;   /* its device address: bands leave HBM through a copy KERNEL (fr_launch_copy_out) */
    size_t stage_cap = 0;
    unsigned int *stage_counters = nullptr;     /* device: one per band in flight (4) */
    unsigned long long *stage_flags = nullptr;  /* pinned, mapped: the bands' completion flags (4) + their device address */
    unsigned long long *stage_flags_dev = nullptr;
    unsigned long long stage_seq = 0;           /* flags carry the sequence number of the band that set them */
    struct CopyPool *copy_pool = nullptr;
    int reserve_stage(size_t bytes);

    /* FR_PRECISION_PT (fr_pt.hip): the last view's reference orbits in device memory, shared with the launches that read
     * them (the last reference frees the memory, after the device has finished with it) */
    std::mutex pt_mu;
    std::shared_ptr<PtOrbit> pt_orbit;
    /* BLA-PT (fr_bla.hip): the skip tables of the last BLA view in device memory, kept and shared like the orbit they
     * were built from, under pt_mu */
    std::shared_ptr<BlaTable> bla_table;

    int create(int device); /* hipSetDevice + streams; the calling thread stays on `device` */
    void destroy();         /* frees everything (caller made sure nothing is in flight) */
    int reserve(Scratch &s, size_t bytes);
    int event(size_t k, hipEvent_t *out); /* k-th reusable event (created on demand) */
    int acquire_palette(PaletteSlot **out);
    void release_palette(PaletteSlot *slot, hipStream_t stream); /* record + make reusable */
    int acquire_surv(size_t bytes, SurvSlot **out);
    void release_surv(SurvSlot *slot, hipStream_t stream);
};

/* calc::Config -> kernel arguments (the local grid is filled in by the caller) and the loop plan */
void fill_params(const fr_config *cfg, const Opts &o, fr_kparams &p);
void plan_loop(const fr_config *cfg, int precision, const Opts &o, fr_kparams &p);
/* fill_params with rows [y0, y1) of the image as the local grid, one block of whole rows; channels == 4: RGBA output
 * (0 for the calls that write no pixels) */
void rows_params(const fr_config *cfg, const Opts &o, uint32_t y0, uint32_t y1, unsigned channels, fr_kparams &p);

/* device-pointer render of the local grid set in `p`; `ctx` lends the palette slot (it must live
 * on the device `stream` belongs to).  No host synchronisation. */
int render_device(Ctx &ctx, const fr_config *cfg, fr_kparams &p, int precision, const Opts &o, void *d_out,
                  hipStream_t stream);

/* row-block-cyclic chunk: blocks first_block, first_block + stride, ... (at most max_blocks; 0 = all) */
int render_block_cyclic(Ctx &ctx, const fr_config *cfg, int precision, const Opts &o, uint32_t block_rows,
                        uint32_t first_block, uint32_t block_stride, uint32_t max_blocks, int dest_is_image,
                        void *d_out, size_t out_len, hipStream_t stream, uint64_t *rows_written);

int check_precision(int precision);
/* cfg not NULL and 0 <= y0 <= y1 <= height; channels 3 or 4 */
int check_rows(const fr_config *cfg, uint32_t y0, uint32_t y1);
int check_channels(int channels);

/* FR_PRECISION_DD (fr_dd.hip): the domain check of include/fractal_hip.h (pos_lo NULL = (0, 0)); no device needed */
int check_dd(const fr_config *cfg, const fr_imaginary *pos_lo);
/* FR_PRECISION_PT: DD's domain plus iterations <= FR_PT_MAX_ITERATIONS (include/fractal_hip.h); no device needed */
int check_pt(const fr_config *cfg, const fr_imaginary *pos_lo);
/* check_dd / check_pt (pos_lo = 0) for FR_PRECISION_DD / FR_PRECISION_PT, else check_precision: the single-device calls
 * that accept the deep-zoom precisions */
int check_precision_or_deep(const fr_config *cfg, int precision);
/* check_dd / check_pt with pos_lo for the deep-zoom precisions, else check_precision */
int check_precision_lo(const fr_config *cfg, int precision, const fr_imaginary *pos_lo);

/* The view centre of a deep call: (cfg->pos, pos_lo) in double-double (pos_lo NULL = (0, 0)), or — FR_PRECISION_PT only —
 * the wide centre that stands in their place (include/fractal_hip.h, "WIDE PT").  The public entry points build one on
 * their first line; every road below them takes it whole, so none can drop the wide half on the way. */
struct Centre {
    const fr_imaginary *pos_lo; /* an aggregate, always written Centre{pos_lo, wide}, or Centre{nullptr, wide, true} */
    const fr_wide_centre *wide;
    bool scaled = false; /* a SCALED PT call: `wide` is required and checked against SCALED PT's domain */
    double lo_re() const { return pos_lo ? pos_lo->re : 0.0; }
    double lo_im() const { return pos_lo ? pos_lo->im : 0.0; }
    /* the domain check: check_pt_wide (fr_wide.h) for a wide centre or a scaled call, else check_precision_lo; no device
     * needed */
    int check(const fr_config *cfg, int precision) const;
};

/* profiling (fr_set_profiling) around the launches of one call on `stream`: prof_begin creates the thread's events on first
 * use and records the first; prof_end, called only after a successful launch, records the second and the name
 * fr_last_kernel_name reports.  Both do nothing while profiling is off. */
int prof_begin(hipStream_t stream);
int prof_end(hipStream_t stream, const char *kernel_name);

/* DD or PT rows [y0, y1) as RGB (bpp 3) / RGBA (bpp 4) into device memory on `stream`; arguments already checked.
 * Records the profiling events and the kernel's name like render_device.  No host synchronisation (PT: apart from
 * computing and uploading the view's reference orbit when the context does not hold it yet). */
int render_deep_device(Ctx &ctx, int precision, const fr_config *cfg, const Centre &c, const Opts &o, uint32_t y0, uint32_t y1,
                       unsigned bpp, void *d_out, hipStream_t stream);
/* The bodies of the deep row calls (fr_api.hip) that the PT entry points of fr_pt.hip share with the DD ones: every check,
 * then render_deep_device / the escape launch.  zw: doubles of z per pixel (4: DD with its low parts). */
int render_rows_device(const fr_config *cfg, int precision, const Centre &c, uint32_t y0, uint32_t y1, void *d_out, size_t out_len,
                       void *hip_stream, unsigned bytes_per_pixel, const fr_render_opts *opts);
int escape_rows(const fr_config *cfg, int precision, const Centre &c, uint32_t y0, uint32_t y1, double *z, uint32_t *iters,
                unsigned zw);
/* FR_PRECISION_PT (fr_pt.hip: escape_pt_kernel): the launch's local grid, colour and limit from `p` as for DD; the view's
 * reference orbits from ctx's cache (computed and uploaded on a miss).  MODE ESCAPE writes re, im per pixel. */
int launch_pt(Ctx &ctx, const fr_config *cfg, const Centre &c, const fr_kparams &p, int mode, const fr_kout &out,
              hipStream_t stream, const char **kernel_name);

/* For BLA-PT (fr_bla.hip), from fr_pt.hip: the view's orbits in device memory as launch_pt finds them (the context's cache,
 * computed and uploaded on a miss) — `keep` holds them alive and is their identity, v.k == v.x for Mandelbrot — and orbit
 * `which` (0: R or V, 1: K) on the host as re, im pairs appended to `out`, no device needed.  Arguments already checked.
 * `ended`: bit 0 = X, bit 1 = K is ended by escape (PtOrbit::ended(); the state kernels' rebase rule reads it). */
struct PtOrbitView {
    const double2 *x = nullptr, *k = nullptr;
    uint32_t x_last = 0, k_last = 0;
    uint32_t ended = 0;
};
int pt_orbit_view(Ctx &ctx, const fr_config *cfg, const Centre &c, std::shared_ptr<PtOrbit> &keep, PtOrbitView &v);
void pt_host_orbit(const fr_config *cfg, const Centre &c, int which, std::vector<double> &out);

/* choose_kernel for rows [y0, y1) of the image as ONE launch, recorded in `o` (tile 0 only): callers that render those
 * rows in several launches then sample the view once, not once per launch.  The calling thread must be on ctx's device. */
void decide_kernel(Ctx &ctx, const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, Opts &o, hipStream_t stream,
                   bool allow_async);

/* the primary context (what fr_init selected); locks and lazily creates it.  Callers hold
 * `life_shared()` while they use it. */
int primary(Ctx **out);
/* the primary context if it exists, else nullptr: creates nothing and touches no device (test hooks) */
Ctx *primary_if_created();

/* Lifetime lock: entry points that enqueue on library state hold it shared; fr_init (device switch),
 * fr_init_devices and fr_shutdown hold it exclusively, so state is never torn down under a call. */
struct LifeShared {
    LifeShared();
    ~LifeShared();
};
struct LifeExclusive {
    LifeExclusive();
    ~LifeExclusive();
};

/* ---- host buffers (fr_host.hip) ------------------------------------------------------------- */

/* Walks a host buffer in page-aligned chunks of 64 MiB, making each DMA-able in turn: where the pages
 * do not exist yet (a fresh Vec) a background thread faults them in ahead of the walk (huge-page hint,
 * several threads), then the chunk is pinned with hipHostRegister.  `portable` = for every device. */
class ChunkPinner {
  public:
    /* byte_order (optional): image byte offsets in the order the caller will need them, so that the first
     * touch runs ahead in that order */
    ChunkPinner(uint8_t *out, size_t need, bool portable, const std::vector<size_t> *byte_order = nullptr);
    ~ChunkPinner();
    size_t chunks() const { return bounds_.size() - 1; }
    size_t bound(size_t k) const { return bounds_[k]; } /* chunk k = bytes [bound(k), bound(k + 1)) */
    size_t chunk_of(size_t byte) const;
    /* waits for the chunk's first touch, pins it once; false: it cannot be pinned (plain copy).  Different chunks
     * may be pinned from different threads at the same time (fr_multi.hip's pool); one chunk by one thread. */
    bool pin(size_t k);
    /* the chunks in address order: pins the next one, bytes [a, b); returns false when the walk is over */
    bool next(size_t &a, size_t &b, bool &pinned);
    void release(); /* unpin everything (the caller drained its streams first) */
    /* where the chunk starting at byte `a` ends: a pure function of (out, need, a), so that other threads
     * can split their copies at the same places (one DMA must not span two pins) */
    static size_t chunk_end(const uint8_t *out, size_t need, size_t a);
    double t_touch = 0.0, t_reg = 0.0; /* ms spent waiting for the toucher / in hipHostRegister */

  private:
    uint8_t *out_;
    size_t need_, pos_ = 0;
    unsigned flags_;
    std::vector<size_t> bounds_;
    std::unique_ptr<std::atomic<int>[]> state_; /* 0: pages may not exist yet, 1: touched */
    std::vector<char> pinned_;                  /* 0: not tried, 1: pinned, 2: cannot be pinned */
    std::thread toucher_;
    std::mutex reg_mu_; /* regs_ and the two timers, when chunks are pinned from several threads */
    std::vector<uint8_t *> regs_;
};
void prefault(void *ptr, size_t len);
void destroy_copy_pool(CopyPool *pool); /* stops and joins the threads (fr_host.hip) */

/* per-thread kernel timing (fr_set_profiling / fr_last_kernel_ms) */
struct Profiling {
    bool enabled = false;
    bool have = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const char *kernel = "";
    ~Profiling();
};
Profiling &profiling();

/* ---- the host-buffer form of a call: the primary context under ctx->mu, its scratch, one launch on ctx->stream, the
 * copy back, one synchronisation.  `launch` is any callable (a lambda: no allocation on the call path); every argument
 * check comes before these. ------------------------------------------------------------------------------------------- */

/* RGB: launch(ctx, d_out, stream) fills `need` bytes of ctx->rgb */
template <class Launch>
int host_rgb(uint8_t *out, size_t need, Launch &&launch) {
    LifeShared ls;
    Ctx *ctx;
    int rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rc = ctx->reserve(ctx->rgb, need);
    if (rc == FR_OK) rc = launch(*ctx, ctx->rgb.ptr, ctx->stream);
    if (rc != FR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->rgb.ptr, need, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

/* Raw results: launch(ctx, d_z, d_iters, d_dz, d_m, d_der, stream) over z (zb bytes) and iters (ib bytes) — either may be
 * NULL, its device pointer then is too — and, where they are given, the PT state's second pair dz / m and DE's derivative
 * der of the same sizes behind them in the same two scratch buffers: z, dz, der in the context's z scratch, iters, m in its
 * iters scratch, an array that is not given taking no room.  upload: the arrays go to the device first (the extensions
 * continue them). */
template <class Launch>
int host_raw(double *z, size_t zb, uint32_t *iters, size_t ib, double *dz, uint32_t *m, double *der, bool upload, Launch &&launch) {
    LifeShared ls;
    Ctx *ctx;
    int rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (z) rc = ctx->reserve(ctx->z, (1 + (dz != nullptr) + (der != nullptr)) * zb);
    if (rc == FR_OK && iters) rc = ctx->reserve(ctx->iters, m ? 2 * ib : ib);
    if (rc != FR_OK) return rc;
    char *const d_z = z ? static_cast<char *>(ctx->z.ptr) : nullptr, *const d_iters = iters ? static_cast<char *>(ctx->iters.ptr) : nullptr;
    const struct {
        void *host, *dev;
        size_t bytes;
    } arrays[5] = {{z, d_z, zb}, {iters, d_iters, ib}, {dz, dz ? d_z + zb : nullptr, zb}, {m, m ? d_iters + ib : nullptr, ib},
                   {der, der ? d_z + (dz ? 2 : 1) * zb : nullptr, zb}};
    if (upload)
        for (const auto &a : arrays)
            if (a.host) HIP_TRY(hipMemcpyAsync(a.dev, a.host, a.bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = launch(*ctx, static_cast<double *>(arrays[0].dev), static_cast<uint32_t *>(arrays[1].dev), static_cast<double *>(arrays[2].dev),
                static_cast<uint32_t *>(arrays[3].dev), static_cast<double *>(arrays[4].dev), ctx->stream);
    if (rc != FR_OK) return rc;
    for (const auto &a : arrays)
        if (a.host) HIP_TRY(hipMemcpyAsync(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

/* the calls without a derivative: launch(ctx, d_z, d_iters, d_dz, d_m, stream) */
template <class Launch>
int host_raw(double *z, size_t zb, uint32_t *iters, size_t ib, double *dz, uint32_t *m, bool upload, Launch &&launch) {
    return host_raw(z, zb, iters, ib, dz, m, nullptr, upload,
                    [&](Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_dz, uint32_t *d_m, double *, hipStream_t stream) {
                        return launch(ctx, d_z, d_iters, d_dz, d_m, stream);
                    });
}

/* ---- the pieces the row calls are made of.  An entry point builds its Centre, runs its road's domain check and hands one
 * of these the road's launch, a callable (a lambda: no allocation on the call path).  Each keeps the order of its checks and
 * their texts: they are behaviour (tests/golden/deep_call_errors.json). ------------------------------------------------- */

/* Rows [y0, y1) as one launch on `stream` between the profiling events (fr_set_profiling): launch(p, kname) gets the rows'
 * parameters (it may go on to plan its loop in them) and names its kernel for fr_last_kernel_name. */
template <class Launch>
int profiled_rows(const fr_config *cfg, const Opts &o, uint32_t y0, uint32_t y1, unsigned channels, hipStream_t stream, Launch &&launch) {
    fr_kparams p;
    rows_params(cfg, o, y0, y1, channels, p);
    int rc = prof_begin(stream);
    if (rc != FR_OK) return rc;
    const char *kname = "";
    rc = launch(p, kname);
    if (rc != FR_OK) return rc;
    return prof_end(stream, kname);
}

/* The device-pointer form of a call: the primary context under the lifetime lock and the caller's stream; no ctx->mu, no
 * scratch, no synchronisation.  body(ctx, stream). */
template <class Body>
int device_form(void *hip_stream, Body &&body) {
    LifeShared ls;
    Ctx *ctx;
    const int rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    return body(*ctx, static_cast<hipStream_t>(hip_stream));
}

/* The four row calls of a road, after its domain check: RGB / RGBA and raw results (z: zw doubles per pixel), each into
 * device memory on the caller's stream and into a host buffer.  launch(ctx, ko, stream) renders the rows into `ko`. */
template <class Launch>
int rgb_rows_device(const fr_config *cfg, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *hip_stream,
                    Launch &&launch) {
    const size_t need = (size_t)channels * cfg->width * (size_t)(y1 - y0);
    if (need == 0) return FR_OK;
    if (!d_out) return fail(FR_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*(y1-y0)");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output must be 4-byte aligned");
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) {
        fr_kout ko{};
        ko.rgb = static_cast<uint8_t *>(d_out);
        return launch(ctx, ko, stream);
    });
}

template <class Launch>
int rgb_rows_host(const fr_config *cfg, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len, Launch &&launch) {
    const size_t need = (size_t)channels * cfg->width * (size_t)(y1 - y0);
    if (need == 0) return FR_OK;
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*(y1-y0)");
    return host_rgb(out, need, [&](Ctx &ctx, void *d_out, hipStream_t stream) {
        fr_kout ko{};
        ko.rgb = static_cast<uint8_t *>(d_out);
        return launch(ctx, ko, stream);
    });
}

template <class Launch>
int raw_rows_device(const fr_config *cfg, uint32_t y0, uint32_t y1, void *d_z, void *d_iters, void *hip_stream, Launch &&launch) {
    const size_t npx = (size_t)cfg->width * (size_t)(y1 - y0);
    if (npx == 0 || (!d_z && !d_iters)) return FR_OK;
    if (reinterpret_cast<uintptr_t>(d_z) & 7u) return fail(FR_ERR_INVALID_ARGUMENT, "d_z must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_iters) & 3u) return fail(FR_ERR_INVALID_ARGUMENT, "d_iters must be 4-byte aligned");
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) {
        fr_kout ko{};
        ko.z = static_cast<double *>(d_z);
        ko.iters = static_cast<uint32_t *>(d_iters);
        return launch(ctx, ko, stream);
    });
}

template <class Launch>
int raw_rows_host(const fr_config *cfg, uint32_t y0, uint32_t y1, double *z, uint32_t *iters, unsigned zw, Launch &&launch) {
    const size_t npx = (size_t)cfg->width * (size_t)(y1 - y0);
    if (npx == 0 || (!z && !iters)) return FR_OK;
    return host_raw(z, npx * zw * sizeof(double), iters, npx * sizeof(uint32_t), nullptr, nullptr, false,
                    [&](Ctx &ctx, double *d_z, uint32_t *d_iters, double *, uint32_t *, hipStream_t stream) {
                        fr_kout ko{};
                        ko.z = d_z;
                        ko.iters = d_iters;
                        return launch(ctx, ko, stream);
                    });
}

/* MODE COUNT read back: launch(ctx, ko, stream) adds into GROUPS x FR_COUNT_SLOTS zeroed partial sums at ko.count (ctx->misc,
 * on ctx->stream under ctx->mu); group g's slots are then added to *sums[g]. */
template <size_t GROUPS, class Launch>
int count_rows(uint64_t *const (&sums)[GROUPS], Launch &&launch) {
    LifeShared ls;
    Ctx *ctx;
    int rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    constexpr size_t bytes = sizeof(unsigned long long) * GROUPS * FR_COUNT_SLOTS;
    rc = ctx->reserve(ctx->misc, bytes);
    if (rc != FR_OK) return rc;
    HIP_TRY(hipMemsetAsync(ctx->misc.ptr, 0, bytes, ctx->stream));
    fr_kout ko{};
    ko.count = static_cast<unsigned long long *>(ctx->misc.ptr);
    rc = launch(*ctx, ko, ctx->stream);
    if (rc != FR_OK) return rc;
    unsigned long long host[GROUPS * FR_COUNT_SLOTS];
    HIP_TRY(hipMemcpyAsync(host, ctx->misc.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t g = 0; g < GROUPS; g++)
        for (uint32_t s = 0; s < FR_COUNT_SLOTS; s++) *sums[g] += host[g * FR_COUNT_SLOTS + s];
    return FR_OK;
}

/* The resumable state of a perturbation road — z, iters, the offset d (PT: dz, SCALED PT: w) and m — after the road's
 * domain check.  `from` = nullptr: the state render, else the extension from *from.  check_state is what is left of the
 * calls' domain (include/fractal_hip.h), before any device work; its texts name the road and the offset.  *work = false: a
 * legal call with nothing to do (no rows; for the extension also M == N or an algorithm without orbits).  (Internal linkage:
 * the library's dynamic symbols stay what they were.)
 * launch(ctx, d_z, d_iters, d_d, d_m, stream): host_raw's; the host form keeps z and d in the context's z scratch, iters and
 * m in its iters scratch, and uploads them first for an extension. */
static inline int check_state(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, const void *z, const void *iters,
                              const void *d, const void *m, const char *road, const char *d_name, bool *work) {
    *work = false;
    if (from && cfg->iterations < *from)
        return fail(FR_ERR_INVALID_ARGUMENT, "cfg->iterations < from_iterations: a lower cap cannot be derived from a stored state");
    if ((size_t)cfg->width * (size_t)(y1 - y0) == 0) return FR_OK;
    if (!z || !iters || !d || !m)
        return fail(FR_ERR_INVALID_ARGUMENT, std::string("NULL array: the ") + road + " state is z, iters, " + d_name + " and m, all four");
    if ((reinterpret_cast<uintptr_t>(z) & 7u) || (reinterpret_cast<uintptr_t>(d) & 7u) || (reinterpret_cast<uintptr_t>(iters) & 3u) ||
        (reinterpret_cast<uintptr_t>(m) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, std::string("z and ") + d_name + " must be 8-byte aligned, iters and m 4-byte aligned");
    *work = !from || (cfg->iterations != *from && (cfg->algo == FR_ALGO_MANDELBROT || cfg->algo == FR_ALGO_JULIA));
    return FR_OK;
}

template <class Launch>
int state_device(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z, void *d_iters, void *d_d, void *d_m,
                 void *hip_stream, const char *road, const char *d_name, Launch &&launch) {
    bool work;
    const int rc = check_state(cfg, y0, y1, from, d_z, d_iters, d_d, d_m, road, d_name, &work);
    if (rc != FR_OK || !work) return rc;
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) {
        return launch(ctx, static_cast<double *>(d_z), static_cast<uint32_t *>(d_iters), static_cast<double *>(d_d),
                      static_cast<uint32_t *>(d_m), stream);
    });
}

template <class Launch>
int state_host(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, double *z, uint32_t *iters, double *d, uint32_t *m,
               const char *road, const char *d_name, Launch &&launch) {
    bool work;
    const int rc = check_state(cfg, y0, y1, from, z, iters, d, m, road, d_name, &work);
    if (rc != FR_OK || !work) return rc;
    const size_t npx = (size_t)cfg->width * (size_t)(y1 - y0);
    return host_raw(z, npx * 2 * sizeof(double), iters, npx * sizeof(uint32_t), d, m, from != nullptr, launch);
}

/* multi-device teardown hook, called by fr_shutdown / fr_init_devices with the exclusive lock held */
void multi_shutdown_locked();

}  // namespace fr

/* shared body of the host-buffer row renders (fr_host.hip) */
int fr_host_render_rows(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint8_t *out, size_t out_len,
                        unsigned bytes_per_pixel, const fr_render_opts *opts);
/* the same for FR_PRECISION_DD / FR_PRECISION_PT with the view's centre (fr_host.hip) */
int fr_host_render_rows_deep(const fr_config *cfg, int precision, const fr::Centre &c, uint32_t y0, uint32_t y1, uint8_t *out,
                             size_t out_len, unsigned bytes_per_pixel, const fr_render_opts *opts);

#endif
