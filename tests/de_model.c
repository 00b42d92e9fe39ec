/*
 * de_model.c — host restatement of DE, distance estimation (include/fractal_hip.h, fr_precision: "DE"), written from the
 * definition alone: the checker the kernels of fractal-renderer_amd/csrc/fr_de.hip are compared with bit for bit.
 *
 *   dem_f64_rows   the F64 road: recursive() (calc/src/lib.rs:245-257) with the derivative beside it
 *   dem_pt_rows    PT's step sequence over reference orbits that are PASSED IN (tests/pt_model.py gives a dd centre's,
 *                  tests/pt_wide_model.py a wide centre's: the roads differ only there), with the derivative beside it
 *   dem_distance   (z, iters, der) -> D in pixels
 *   dem_shade      the shading of colour bytes that the reference's colour map produced (tests/de_model.py takes them from
 *                  the oracle)
 *
 * Compiled by tests/de_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused multiply-add but the
 * explicit fma() calls), into a temporary directory.  log2 is the software log2 of the colour map, from the oracle's copy.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "soft_log2.h" /* oracle/: fr_log2_tab and the table's initialiser */

static const double dem_log2_table[FR_LOG2_N][3] = FR_LOG2_TABLE_INIT;

static double dem_log2(double x) { return fr_log2_tab(x, &dem_log2_table[0][0]); }

typedef struct {
    double re, im;
} dem_imaginary;

typedef struct {
    uint8_t r, g, b;
} dem_rgb;

/* fr_config, field for field (104 bytes) */
typedef struct {
    uint32_t algo, width, height, iterations;
    double limit, stable_limit;
    dem_imaginary pos, scale;
    double exposure;
    uint8_t inside, smooth;
    dem_rgb primary_color, secondary_color;
    double color_weight;
    dem_imaginary julia_set;
} dem_config;

int dem_config_size(void) { return (int)sizeof(dem_config); }

/* nd = 2 z d + b0, with the definition's operations */
static void derivative_step(double zr, double zi, double b0, double *dr, double *di) {
    const double tr = zr + zr, ti = zi + zi;
    const double ndr = fma(tr, *dr, fma(-ti, *di, b0));
    const double ndi = fma(tr, *di, ti * *dr);
    *dr = ndr;
    *di = ndi;
}

/* ---- the F64 road ---- */

static uint32_t f64_pixel(const dem_config *cfg, uint64_t x, uint64_t y, double out[4]) {
    const int julia = cfg->algo == 2;
    const double w = (double)cfg->width, h = (double)cfg->height;
    double re = (((double)x / h) - ((w / h) / 2.0)) / cfg->scale.re + cfg->pos.re; /* coord_to_space, :181-197 */
    double im = (((double)y / h) - 0.5) / cfg->scale.im + cfg->pos.im;
    const double cre = julia ? cfg->julia_set.re : re, cim = julia ? cfg->julia_set.im : im;
    const double b0 = julia ? 0.0 : 1.0;
    const double squared = cfg->limit * cfg->limit;
    double dr = 1.0, di = 0.0;
    uint32_t i;
    for (i = 0; i < cfg->iterations; i++) {
        const double nre = ((re * re) - (im * im)) + cre; /* square() :87-91, then + c */
        const double nim = ((2.0 * re) * im) + cim;
        derivative_step(re, im, b0, &dr, &di); /* from the position before the step */
        re = nre;
        im = nim;
        if (nre * nre + nim * nim > squared) break; /* (next, i, nd) */
    }
    out[0] = re, out[1] = im, out[2] = dr, out[3] = di;
    return i;
}

void dem_f64_rows(const dem_config *cfg, uint32_t y0, uint32_t y1, double *z, uint32_t *iters, double *der) {
    const int esc = cfg->algo == 0 || cfg->algo == 2;
    for (uint64_t y = y0; y < y1; y++)
        for (uint32_t x = 0; x < cfg->width; x++) {
            const uint64_t k = (y - y0) * cfg->width + x;
            double o[4] = {0.0, 0.0, 0.0, 0.0};
            iters[k] = esc ? f64_pixel(cfg, x, y, o) : 0u;
            z[2 * k] = o[0], z[2 * k + 1] = o[1], der[2 * k] = o[2], der[2 * k + 1] = o[3];
        }
}

/* ---- PT ---- */

typedef struct {
    const double *x, *k; /* the orbit a pixel starts on, and the one it rebases onto (Mandelbrot: the same) */
    uint32_t x_last, k_last;
} dem_orbits;

static uint32_t pt_pixel(const dem_config *cfg, const dem_orbits *o, uint64_t x, uint64_t y, double out[4]) {
    const int julia = cfg->algo == 2;
    const double w = (double)cfg->width, h = (double)cfg->height;
    const double off_re = (((double)x / h) - ((w / h) / 2.0)) / cfg->scale.re;
    const double off_im = (((double)y / h) - 0.5) / cfg->scale.im;
    const double squared = cfg->limit * cfg->limit;
    const double b0 = julia ? 0.0 : 1.0;
    const double *X = o->x;
    uint32_t last = o->x_last;
    uint32_t m = julia ? 0u : 1u;
    double dzr = off_re, dzi = off_im;
    const double dcr = julia ? 0.0 : off_re, dci = julia ? 0.0 : off_im;
    double zr = X[2 * m] + dzr, zi = X[2 * m + 1] + dzi;
    double dr = 1.0, di = 0.0;
    uint32_t i;
    for (i = 0; i < cfg->iterations; i++) {
        const double tr = X[2 * m] + zr, ti = X[2 * m + 1] + zi;
        const double ndr = fma(tr, dzr, fma(-ti, dzi, dcr));
        const double ndi = fma(tr, dzi, fma(ti, dzr, dci));
        derivative_step(zr, zi, b0, &dr, &di); /* from the z the loop holds before the step */
        m++;
        zr = X[2 * m] + ndr;
        zi = X[2 * m + 1] + ndi;
        dzr = ndr;
        dzi = ndi;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break;
        if (dist < dzr * dzr + dzi * dzi || m == last) {
            dzr = zr;
            dzi = zi;
            m = 0;
            X = o->k;
            last = o->k_last;
        }
    }
    out[0] = zr, out[1] = zi, out[2] = dr, out[3] = di;
    return i;
}

void dem_pt_rows(const dem_config *cfg, const double *x_orbit, uint32_t x_last, const double *k_orbit, uint32_t k_last, uint32_t y0,
                 uint32_t y1, double *z, uint32_t *iters, double *der) {
    const int esc = cfg->algo == 0 || cfg->algo == 2;
    const dem_orbits o = {x_orbit, k_orbit, x_last, k_last};
    for (uint64_t y = y0; y < y1; y++)
        for (uint32_t x = 0; x < cfg->width; x++) {
            const uint64_t k = (y - y0) * cfg->width + x;
            double r[4] = {0.0, 0.0, 0.0, 0.0};
            iters[k] = esc ? pt_pixel(cfg, &o, x, y, r) : 0u;
            z[2 * k] = r[0], z[2 * k + 1] = r[1], der[2 * k] = r[2], der[2 * k + 1] = r[3];
        }
}

/* ---- distance ---- */

static double distance(const dem_config *cfg, const double *z, uint32_t it, const double *d) {
    if (it == cfg->iterations) return 0.0;
    const double n2 = z[0] * z[0] + z[1] * z[1];
    const double dn2 = d[0] * d[0] + d[1] * d[1];
    const double num = (sqrt(n2) * dem_log2(n2)) * 0x1.62e42fefa39efp-2;
    const double pixels = (double)cfg->height * fmin(fabs(cfg->scale.re), fabs(cfg->scale.im));
    double D = (num / sqrt(dn2)) * pixels;
    if (!(D > 0.0)) D = 0.0;
    return D;
}

void dem_distance(const dem_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double *out) {
    for (size_t k = 0; k < n; k++) out[k] = distance(cfg, z + 2 * k, iters[k], der + 2 * k);
}

/* ---- shading: base = the colour map's r,g,b per pixel; out = channels (3 or 4) bytes per pixel ---- */

void dem_shade(const dem_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double thickness,
               const uint8_t *base, int channels, uint8_t *out) {
    for (size_t k = 0; k < n; k++) {
        uint8_t c[3] = {base[3 * k], base[3 * k + 1], base[3 * k + 2]};
        if (iters[k] < cfg->iterations && thickness > 0.0) {
            const double s = distance(cfg, z + 2 * k, iters[k], der + 2 * k) / thickness;
            if (s < 1.0)
                for (int j = 0; j < 3; j++) c[j] = (uint8_t)((double)c[j] * s);
        }
        for (int j = 0; j < 3; j++) out[(size_t)channels * k + j] = c[j];
        if (channels == 4) out[4 * k + 3] = 255;
    }
}
