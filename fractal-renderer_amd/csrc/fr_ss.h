/*
 * fr_ss.h — internal: what the supersampled renders share on the host ("3.32").  The plan of a supersampled render
 * (fr_ss.hip) — cfg_s, the source rows and the band rule of fr_ss_workspace_bytes — which the supersampled DE roads (fr_ss_de.hip)
 * run at 36 bytes per sample in place of 3; the band loop of every banded render (ss_bands); the two halves of a banded call
 * behind its domain check (ss_rows_device, ss_rows_host); and the thickness and the pixels of the distance shade, for both DE
 * files.  Host code only.
 */
#ifndef FR_SS_H
#define FR_SS_H

#include <algorithm>
#include <cmath>

#include "fr_ctx.h"

namespace fr {

constexpr size_t kSsBestCap = (size_t)1 << 30;       /* best_bytes of fr_ss_workspace_bytes and fr_ss_de_workspace_bytes */
constexpr size_t kSsHostWorkCap = (size_t)256 << 20; /* the host roads' workspace: the context keeps it */
size_t ss_host_work_cap();                           /* kSsHostWorkCap, or what fr_debug_ss_host_work_cap set */
constexpr uint32_t kDeSampleBytes = 36;              /* a sample of a DE band: z 16 + der 16 + iters 4 */

struct SsPlan {
    fr_config cfg_s;      /* cfg with width * s, height * s */
    uint64_t src_rows;    /* s * (y1 - y0) */
    uint64_t row_bytes;   /* sample_bytes * s * width: one source row */
    size_t min_bytes, best_bytes;
};

/* The part of the domain that needs no precision — cfg, s, the sizes, the rows — and the workspace of rows [y0, y1):
 * min_bytes = one band of 8 * s source rows (or all the rows, if fewer), best_bytes = the whole range, at most 1 GiB.
 * sample_bytes 3: a band is packed r,g,b, and s = 1 renders straight into the output and needs no workspace; 36: a band is
 * the DE arrays (z, der, iters), which s = 1 needs too.  A range without pixels needs none either: min_bytes is 0. */
int ss_plan(const fr_config *cfg, uint32_t s, uint32_t y0, uint32_t y1, SsPlan &pl, uint32_t sample_bytes = 3);

/* LINEAR-LIGHT SUPERSAMPLING: the `transfer` argument of every _tf call, refused before anything else is looked at */
int check_transfer(int transfer);

/* Source rows per band for a workspace of work_len >= min_bytes: the largest multiple of 8 * s that fits (or all the
 * rows), then evened out — nb = ceil(rows / Bmax) bands of ceil(rows / nb) rows rounded up to 8 * s. */
uint64_t ss_band_rows(const SsPlan &pl, uint32_t s, size_t work_len);

/* the workspace a host form reserves in the context's scratch: the whole range under the cap, one band at the least */
inline size_t ss_host_work_len(const SsPlan &pl) { return std::max(pl.min_bytes, std::min(pl.best_bytes, ss_host_work_cap())); }

/* Rows [y0, y1) supersampled into d_out on `stream`: the band loop of every banded render.  band(ctx, ya, yb, dst, out_rows,
 * stream) renders source rows [ya, yb) of cfg_s into the workspace — a road's row launch (fr_bla.hip: bla_rows; DESIGN.md,
 * "3.17") between the profiling events — and launches the filter that puts their out_rows output rows at dst.  Profiling: the
 * span of the whole call — the first band records the start and the render kernel's name, the later bands record nothing, the
 * end goes behind the last filter.  pending_sample: a view sample to post behind the last band and in front of that end (-1
 * none; the F64 road's, which takes it out of its opts).  Arguments already checked, the range and the width not empty.  No
 * host synchronisation beyond what the band's launch has. */
template <class Band>
int ss_bands(Ctx &ctx, const SsPlan &pl, uint32_t s, uint32_t y0, unsigned bpp, void *d_out, size_t work_len, hipStream_t stream,
             int pending_sample, Band &&band) {
    const uint32_t width = pl.cfg_s.width / s;
    const uint64_t rows = ss_band_rows(pl, s, work_len);
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + pl.src_rows);
    Profiling &pr = profiling();
    struct ProfGuard {
        Profiling &pr;
        bool was;
        ~ProfGuard() { pr.enabled = was; }
    } prof_guard{pr, pr.enabled};
    int rc = FR_OK;
    for (uint64_t ya = Y0; ya < Y1 && rc == FR_OK; ya += rows) {
        const uint32_t yb = (uint32_t)std::min<uint64_t>(ya + rows, Y1);
        uint8_t *dst = static_cast<uint8_t *>(d_out) + (uint64_t)(((uint32_t)ya - Y0) / s) * width * bpp;
        rc = band(ctx, (uint32_t)ya, yb, dst, (yb - (uint32_t)ya) / s, stream);
        pr.enabled = false; /* (no filter records an event: the first band's render has recorded the start) */
    }
    ctx.post_sample(pending_sample, stream);
    if (rc == FR_OK && prof_guard.was && pr.have) HIP_TRY(hipEventRecord(pr.e1, stream));
    return rc;
}

/* The device form of a banded call behind its domain check: the workspace's refusals, then rgb_rows_device's.  A plan without
 * a workspace (s = 1 of the packed bands, no pixels) has min_bytes 0 and no rule.  too_small names the call that plans the
 * workspace; aligned8: d_work holds doubles.  launch(ctx, ko, d_work, work_len, stream). */
template <class Launch>
int ss_rows_device(const fr_config *cfg, const SsPlan &pl, const char *too_small, bool aligned8, uint32_t y0, uint32_t y1, int channels,
                   void *d_out, size_t out_len, void *d_work, size_t work_len, void *hip_stream, Launch &&launch) {
    if (pl.min_bytes != 0) {
        if (work_len < pl.min_bytes) return fail(FR_ERR_BUFFER_TOO_SMALL, too_small);
        if (!d_work) return fail(FR_ERR_INVALID_ARGUMENT, "d_work is NULL");
        if (aligned8 && (reinterpret_cast<uintptr_t>(d_work) & 7u))
            return fail(FR_ERR_INVALID_ARGUMENT, "d_work must be 8-byte aligned (z and der lie in it)");
    }
    return rgb_rows_device(cfg, y0, y1, channels, d_out, out_len, hip_stream,
                           [&](Ctx &ctx, const fr_kout &ko, hipStream_t stream) { return launch(ctx, ko, d_work, work_len, stream); });
}

/* The host form of a supersampled call behind its domain check: rgb_rows_host with work_len bytes of the context's ss_work
 * for the launch, and a synchronisation when it fails, because the next call reuses that scratch. */
template <class Launch>
int ss_rows_host(const fr_config *cfg, size_t work_len, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len, Launch &&launch) {
    return rgb_rows_host(cfg, y0, y1, channels, out, out_len, [&](Ctx &ctx, const fr_kout &ko, hipStream_t stream) {
        int rc = ctx.reserve(ctx.ss_work, work_len);
        if (rc != FR_OK) return rc;
        rc = launch(ctx, ko, ctx.ss_work.ptr, work_len, stream);
        if (rc != FR_OK) (void)hipStreamSynchronize(stream);
        return rc;
    });
}

/* ---- the distance shade of the supersampled DE calls (fr_ss_de.hip, fr_ss_adaptive_de.hip) ---- */

/* Ts = T * s, one product; the domain keeps it inside fr_colour_de_rows_device's own */
inline int ss_de_thickness(double thickness, uint32_t s, double &ts) {
    ts = thickness * (double)s;
    if (!(thickness >= 0.0 && ts <= 0x1p20))
        return fail(FR_ERR_INVALID_ARGUMENT, "thickness must be finite with 0 <= thickness * supersample <= 2^20 (output pixels; 0 = no shading)");
    return FR_OK;
}

/* sample pixels per unit of the plane along the tighter axis: the last factor of D on cfg_s, one product */
inline double ss_de_pixels(const fr_config *cfg, uint32_t s, double scale_re, double scale_im) {
    return (double)(s * cfg->height) * std::fmin(std::fabs(scale_re), std::fabs(scale_im));
}
inline double ss_de_pixels(const fr_config *cfg, uint32_t s) { return ss_de_pixels(cfg, s, cfg->scale.re, cfg->scale.im); }

}  // namespace fr

#endif
