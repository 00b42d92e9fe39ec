/*
 * fr_scaled.h — internal: what the scaled kernels of fr_scaled.hip (SCALED PT) and fr_de_scaled.hip (DE ON SCALED PT, RESUMABLE
 * SCALED DE) share, one copy of each: the orbits, tables and scale as a kernel sees them (ScaledDev) with their fill from the
 * context's caches, the BIG threshold, the on-K bit of a stored state's m, the rebase test on one arithmetic path and the staging
 * of woff.  Everything here has internal linkage: each of the two translation units compiles its own copy into its own kernels.
 */
#ifndef FR_SCALED_H
#define FR_SCALED_H

#include <memory>

#include "fr_bla.h"
#include "fr_ctx.h"

namespace {

constexpr double kBig = 0x1p500; /* max(|w.re|, |w.im|) >= kBig: w is "big" and the comparisons scale w down, not z up */
constexpr uint32_t kOnK = 0x80000000u; /* bit 31 of a stored state's m: the pixel follows K (RESUMABLE SCALED PT, RESUMABLE SCALED DE) */

/* the orbits, the tables (escape_bla_scaled_kernel only) and the scale as the kernels see them; Mandelbrot: the k fields
 * repeat the x fields */
struct ScaledDev {
    const double2 *x_orbit, *k_orbit;
    const double *x_R, *k_R;       /* R of the levels >= 1 */
    const double *x_coef, *k_coef; /* Mandelbrot: A.re, A.im, B.re, B.im per entry; Julia: A.re, A.im */
    uint32_t x_last, k_last;
    uint32_t x_n0, k_n0; /* entries of level 0: last - 1, or 0 for an empty table */
    double S, Sinv;      /* 2^e, 2^-e */
};

__device__ __forceinline__ bool is_big(double wr, double wi) {
    const double a = __builtin_fabs(wr), b = __builtin_fabs(wi);
    return (a > b ? a : b) >= kBig;
}

/* the rebase test of the definition on one arithmetic path: (z fl)^2 < (w fr)^2 with the factors selected by `big` */
__device__ __forceinline__ bool rebase_test(double zr, double zi, double wr, double wi, double S, double Sinv) {
    const bool big = is_big(wr, wi);
    const double fl = big ? 1.0 : S, fr = big ? Sinv : 1.0;
    const double lr = zr * fl, li = zi * fl, rr = wr * fr, ri = wi * fr;
    return lr * lr + li * li < rr * rr + ri * ri;
}

/* 16 column and 16 row values of woff for the workgroup's pixels into LDS (scaled_body's staging: p.scale_re and p.scale_im
 * hold sre and sim); the caller synchronises */
__device__ __forceinline__ void stage_woff(const fr_kparams &p, uint32_t tid, uint32_t col0, uint32_t row0, double *s_re, double *s_im) {
    if (tid < kDeepBlockW + kDeepBlockH) {
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kDeepBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            s_re[tid] = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        } else {
            const uint32_t r = row0 + (tid - kDeepBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            s_im[tid - kDeepBlockW] = (((double)y / height) - 0.5) / p.scale_im;
        }
    }
}

}  // namespace

namespace fr {
namespace {

/* The view's orbits and — bits >= 0 — its scaled table from the context's caches (pt_orbit_view, bla_table_for with scaled =
 * true: computed, built and uploaded on a miss) as the kernels take them, with the scale of `k`.  The caller keeps `orbit` and
 * `table` alive until its launch has been enqueued.  Arguments already checked. */
int scaled_dev_fill(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const ScaledConsts &k, std::shared_ptr<PtOrbit> &orbit,
                    std::shared_ptr<BlaTable> &table, ScaledDev &t) {
    PtOrbitView v;
    t = ScaledDev{};
    if (bits >= 0) {
        const int rc = bla_table_for(ctx, cfg, c, bits, true, orbit, v, table);
        if (rc != FR_OK) return rc;
        const BlaTableDev &d = table->view;
        t.x_R = d.x_rad, t.k_R = d.k_rad;
        t.x_coef = d.x_coef, t.k_coef = d.k_coef;
        t.x_n0 = d.x_n0, t.k_n0 = d.k_n0;
    } else {
        const int rc = pt_orbit_view(ctx, cfg, c, orbit, v);
        if (rc != FR_OK) return rc;
    }
    t.x_orbit = v.x;
    t.k_orbit = v.k;
    t.x_last = v.x_last;
    t.k_last = v.k_last;
    t.S = k.S;
    t.Sinv = k.Sinv;
    return FR_OK;
}

}  // namespace
}  // namespace fr

#endif
