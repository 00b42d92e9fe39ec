/*
 * de_state_model.c — host restatement of RESUMABLE DE (include/fractal_hip.h, fr_precision: "RESUMABLE DE"), written from the
 * definition alone: the checker escape_extend_de_kernel, escape_pt_de_state_kernel and escape_extend_pt_de_kernel
 * (fractal-renderer_amd/csrc/fr_de.hip) are compared with bit for bit, and itself compared with tests/de_model.c (DE) and
 * tests/pt_state_model.c (RESUMABLE PT) in tests/test_de_state_model_cpu.py.
 *
 *   desm_f64_continue   the F64 road: stored (z, iters, der) at cap `from` continued in place to cfg->iterations
 *   desm_pt_rows        PT: the state run with the derivative from the initial state (fresh), or the stored state at cap `from`
 *                       continued in place, over reference orbits that are PASSED IN (tests/pt_model.py gives a dd centre's,
 *                       tests/pt_wide_model.py a wide centre's).  Whether an orbit is ended by escape is read off its last
 *                       stored entry, as the definition says.
 *
 * Compiled by tests/de_state_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused multiply-add but
 * the explicit fma() calls), into a temporary directory.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

typedef struct {
    double re, im;
} desm_imaginary;

typedef struct {
    uint8_t r, g, b;
} desm_rgb;

/* fr_config, field for field (104 bytes) */
typedef struct {
    uint32_t algo, width, height, iterations;
    double limit, stable_limit;
    desm_imaginary pos, scale;
    double exposure;
    uint8_t inside, smooth;
    desm_rgb primary_color, secondary_color;
    double color_weight;
    desm_imaginary julia_set;
} desm_config;

int desm_config_size(void) { return (int)sizeof(desm_config); }

/* nd = 2 z d + b0, with the definition's operations */
static void derivative_step(double zr, double zi, double b0, double *dr, double *di) {
    const double tr = zr + zr, ti = zi + zi;
    const double ndr = fma(tr, *dr, fma(-ti, *di, b0));
    const double ndi = fma(tr, *di, ti * *dr);
    *dr = ndr;
    *di = ndi;
}

static int escape_algo(const desm_config *cfg) { return cfg->algo == 0 || cfg->algo == 2; }

/* ---- the F64 road: (previous, N, d) of a pixel with iters == from, continued for cfg->iterations - from steps ---- */

void desm_f64_continue(const desm_config *cfg, uint32_t y0, uint32_t y1, uint32_t from, double *z, uint32_t *iters, double *der) {
    if (!escape_algo(cfg)) return;
    const int julia = cfg->algo == 2;
    const double w = (double)cfg->width, h = (double)cfg->height;
    const double b0 = julia ? 0.0 : 1.0;
    const double squared = cfg->limit * cfg->limit;
    for (uint64_t y = y0; y < y1; y++)
        for (uint32_t x = 0; x < cfg->width; x++) {
            const uint64_t k = (y - y0) * cfg->width + x;
            if (iters[k] != from) continue; /* finished, or foreign: not touched */
            /* c: coord_to_space (calc/src/lib.rs:181-197), the render's own */
            const double cre = julia ? cfg->julia_set.re : (((double)x / h) - ((w / h) / 2.0)) / cfg->scale.re + cfg->pos.re;
            const double cim = julia ? cfg->julia_set.im : (((double)y / h) - 0.5) / cfg->scale.im + cfg->pos.im;
            double re = z[2 * k], im = z[2 * k + 1], dr = der[2 * k], di = der[2 * k + 1];
            uint32_t i;
            for (i = from; i < cfg->iterations; i++) {
                const double nre = ((re * re) - (im * im)) + cre;
                const double nim = ((2.0 * re) * im) + cim;
                derivative_step(re, im, b0, &dr, &di);
                re = nre;
                im = nim;
                if (nre * nre + nim * nim > squared) break;
            }
            z[2 * k] = re, z[2 * k + 1] = im, der[2 * k] = dr, der[2 * k + 1] = di;
            iters[k] = i;
        }
}

/* ---- PT ---- */

typedef struct {
    const double *v; /* re, im pairs */
    uint32_t last;
    int ended; /* by escape; else cut by the cap */
} desm_orbit;

static desm_orbit make_orbit(const double *v, uint32_t last, int julia) {
    const uint32_t kmin = julia ? 1u : 2u;
    desm_orbit o = {v, last, 0};
    o.ended = last >= kmin && v[2 * last] * v[2 * last] + v[2 * last + 1] * v[2 * last + 1] > 4.0;
    return o;
}

typedef struct {
    double zr, zi, dzr, dzi, dr, di;
    uint32_t m;
    int on_k;
} desm_state;

/* steps from .. to - 1 of the state run on a running pixel.  Returns the escape index, or `to`.  *violations counts the steps
 * that began with m >= last of the orbit followed (the definition needs X_{m+1}); such a pixel is left where it is. */
static uint32_t run(const desm_config *cfg, const desm_orbit *ox, const desm_orbit *ok, double off_re, double off_im, uint32_t from,
                    uint32_t to, desm_state *s, uint64_t *violations) {
    const int julia = cfg->algo == 2;
    const double squared = cfg->limit * cfg->limit;
    const double dcr = julia ? 0.0 : off_re, dci = julia ? 0.0 : off_im;
    const double b0 = julia ? 0.0 : 1.0;
    const desm_orbit *X = s->on_k ? ok : ox;
    for (uint32_t i = from; i < to; i++) {
        if (s->m >= X->last) {
            (*violations)++;
            return to;
        }
        const double tr = X->v[2 * s->m] + s->zr, ti = X->v[2 * s->m + 1] + s->zi;
        const double ndr = fma(tr, s->dzr, fma(-ti, s->dzi, dcr));
        const double ndi = fma(tr, s->dzi, fma(ti, s->dzr, dci));
        derivative_step(s->zr, s->zi, b0, &s->dr, &s->di); /* from the z before the step */
        s->m++;
        s->zr = X->v[2 * s->m] + ndr;
        s->zi = X->v[2 * s->m + 1] + ndi;
        s->dzr = ndr;
        s->dzi = ndi;
        const double dist = s->zr * s->zr + s->zi * s->zi;
        if (dist > squared) { /* (next, i, dz = 0, m = 0, nd) */
            s->dzr = s->dzi = 0.0;
            s->m = 0;
            s->on_k = 0;
            return i;
        }
        if (dist < s->dzr * s->dzr + s->dzi * s->dzi || (s->m == X->last && X->ended)) {
            s->dzr = s->zr;
            s->dzi = s->zi;
            s->m = 0;
            if (julia) {
                X = ok;
                s->on_k = 1;
            }
        }
    }
    return to;
}

#define ON_K 0x80000000u

/* Rows [y0, y1) from cap `from` to cfg->iterations on the orbits given (those of cfg's cap; Mandelbrot: k_orbit is x_orbit).
 * fresh != 0: from the initial state (`from` is 0 then), every pixel written.  Otherwise the arrays hold the state at `from`
 * and are continued in place: a pixel with iters != from is not touched.  z, dz, der: re, im per pixel; m: bit 31 = on K. */
void desm_pt_rows(const desm_config *cfg, const double *x_orbit, uint32_t x_last, const double *k_orbit, uint32_t k_last, uint32_t y0,
                  uint32_t y1, uint32_t from, int fresh, double *z, uint32_t *iters, double *dz, uint32_t *m, double *der,
                  uint64_t *violations) {
    const int esc = escape_algo(cfg), julia = cfg->algo == 2;
    const double w = (double)cfg->width, h = (double)cfg->height;
    desm_orbit ox = {0, 0, 0}, ok = {0, 0, 0};
    uint64_t viol = 0;
    if (esc) {
        ox = make_orbit(x_orbit, x_last, julia);
        ok = julia ? make_orbit(k_orbit, k_last, julia) : ox;
    }
    for (uint64_t y = y0; y < y1; y++)
        for (uint32_t x = 0; x < cfg->width; x++) {
            const uint64_t k = (y - y0) * cfg->width + x;
            if (!esc) {
                if (fresh) z[2 * k] = z[2 * k + 1] = dz[2 * k] = dz[2 * k + 1] = der[2 * k] = der[2 * k + 1] = 0.0, iters[k] = m[k] = 0;
                continue;
            }
            const double off_re = (((double)x / h) - ((w / h) / 2.0)) / cfg->scale.re;
            const double off_im = (((double)y / h) - 0.5) / cfg->scale.im;
            desm_state s;
            if (fresh) {
                s.m = julia ? 0u : 1u;
                s.on_k = 0;
                s.dzr = off_re, s.dzi = off_im;
                s.zr = ox.v[2 * s.m] + s.dzr, s.zi = ox.v[2 * s.m + 1] + s.dzi;
                s.dr = 1.0, s.di = 0.0;
            } else {
                if (iters[k] != from) continue;
                s.zr = z[2 * k], s.zi = z[2 * k + 1], s.dzr = dz[2 * k], s.dzi = dz[2 * k + 1], s.dr = der[2 * k], s.di = der[2 * k + 1];
                s.m = m[k] & ~ON_K;
                s.on_k = (m[k] & ON_K) != 0;
            }
            iters[k] = run(cfg, &ox, &ok, off_re, off_im, from, cfg->iterations, &s, &viol);
            z[2 * k] = s.zr, z[2 * k + 1] = s.zi, dz[2 * k] = s.dzr, dz[2 * k + 1] = s.dzi, der[2 * k] = s.dr, der[2 * k + 1] = s.di;
            m[k] = s.m | (s.on_k ? ON_K : 0u);
        }
    if (violations) *violations = viol;
}
