/*
 * fr_bla.h — internal: what BLA-PT (fr_bla.hip) and SCALED PT (fr_scaled.hip) share — the device layout of a view's skip
 * tables, the cached tables of a context, and the constants of a scaled view.  The host build of both tables lives in
 * fr_bla.hip; fr_scaled.hip holds the scaled kernels and their calls.
 */
#ifndef FR_BLA_H
#define FR_BLA_H

#include <cmath>
#include <memory>

#include "fr_ctx.h"

/* first entry of level k >= 1 among the levels 1, 2, ... of a table whose level 0 has n0 entries: the sum of n0 >> l over
 * l = 1 .. k-1, from the identity  sum over l >= 1 of (n >> l) = n - popcount(n)  applied to n0 and to n0 >> (k-1) */
__host__ __device__ __forceinline__ uint32_t bla_level_offset(uint32_t n0, uint32_t k) {
    const uint32_t t = n0 >> (k - 1);
#ifdef __HIP_DEVICE_COMPILE__
    return (n0 - (uint32_t)__popc(n0)) - (t - (uint32_t)__popc(t));
#else
    return (n0 - (uint32_t)__builtin_popcount(n0)) - (t - (uint32_t)__builtin_popcount(t));
#endif
}

namespace fr {

/* a view's tables in device memory as the kernels find them; Mandelbrot: the k fields repeat the x fields */
struct BlaTableDev {
    const double *x_rad, *k_rad;   /* per entry of the levels >= 1: r2 (BLA-PT), or the scaled radius R (SCALED PT) */
    const double *x_coef, *k_coef; /* Mandelbrot: A.re, A.im, B.re, B.im per entry; Julia: A.re, A.im */
    uint32_t x_n0, k_n0;           /* entries of level 0: last - 1, or 0 for an empty table */
};

/* the tables of one view in device memory: one allocation, coefficients first (32-byte entries stay aligned) */
struct BlaTable {
    std::weak_ptr<PtOrbit> orbit; /* identity of the orbits the tables were built from; holds no device memory alive */
    double D = 0.0;               /* D, or Dw of a scaled table */
    double S = 1.0;               /* S = 2^e of a scaled table (eps and every stored R are proportional to it); BLA-PT: 1 */
    int bits = 0;
    bool scaled = false; /* SCALED PT's table: R in place of r2 */
    void *dev = nullptr;
    BlaTableDev view{};
    uint32_t x_levels = 0, entries = 0; /* fr_debug_bla_cache */
    bool built = false;                 /* the last request built the tables */
    ~BlaTable() {
        if (dev) (void)hipFree(dev); /* hipFree waits for the device: no kernel still reads the tables */
    }
};

/* The constants of a scaled view (include/fractal_hip.h, "SCALED PT"): max(|scale.re|, |scale.im|) = f 2^e with
 * 0.5 <= f < 1, S = 2^e, Sinv = 2^-e, sre = scale.re Sinv and sim = scale.im Sinv (both exact). */
struct ScaledConsts {
    int e;
    double S, Sinv, sre, sim;
};
inline ScaledConsts scaled_consts(const fr_config *cfg) {
    ScaledConsts c;
    const double a = std::fabs(cfg->scale.re), b = std::fabs(cfg->scale.im);
    (void)std::frexp(a > b ? a : b, &c.e);
    c.S = std::ldexp(1.0, c.e);
    c.Sinv = std::ldexp(1.0, -c.e);
    c.sre = cfg->scale.re * c.Sinv;
    c.sim = cfg->scale.im * c.Sinv;
    return c;
}

/* The view's orbits (`orbit` holds them, `v` points into them) and tables — BLA-PT's, or SCALED PT's when `scaled` — from
 * the context's caches or built and uploaded (fr_bla.hip); the caller keeps `orbit` and `out` alive until its launch has
 * been enqueued.  Arguments already checked. */
int bla_table_for(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, bool scaled, std::shared_ptr<PtOrbit> &orbit,
                  PtOrbitView &v, std::shared_ptr<BlaTable> &out);

/* The body of fr_debug_bla_table and fr_debug_bla_table_scaled (host only): level `level` of the table of orbit `which`, 5
 * doubles per entry, the fifth r2 or — `scaled` — R.  cfg, c and bits already checked. */
int bla_debug_table(const fr_config *cfg, const Centre &c, int bits, bool scaled, int which, uint32_t level, double *out, size_t cap,
                    uint32_t *len);

/* For the supersampled form of the roads (fr_ss.hip: fr_render_rows_ss_pt), which renders the rows of cfg_s band by band:
 * bla_check / scaled_check — the domain checks the roads' own calls run (the file-local check_bla / check_scaled), bits
 * resolved in place — and bla_render_rows / scaled_render_rows — the roads' row launch (the file-local bla_rows / scaled_rows)
 * in MODE RGB, called: rows [y0, y1) into out.rgb on `stream` between the profiling events (fr_bla.hip, fr_scaled.hip). */
int bla_check(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1);
int bla_render_rows(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, unsigned channels,
                    const fr_kout &out, hipStream_t stream);
int scaled_check(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1);
int scaled_render_rows(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, unsigned channels,
                       const fr_kout &out, hipStream_t stream);

}  // namespace fr

#endif
