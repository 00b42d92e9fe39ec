/*
 * de_scaled_model.c — host restatement of DE ON SCALED PT (include/fractal_hip.h, "DE ON SCALED PT"), written from the
 * definition alone: SCALED PT's pixel loop (tests/pt_scaled_model.c restates it; the lines are repeated here so that z, iters
 * and the passes can be compared with that model bit for bit) with the scaled derivative u carried beside it.  The checker the
 * kernels of fractal-renderer_amd/csrc/fr_de_scaled.hip are compared with bit for bit.
 *
 * Nothing is built here: the orbits are PASSED IN (tests/pt_wide_model.py computes them on Python integers) and so are their
 * tables, as tests/pt_scaled_model.c's ptsm_build_table lays them out — 5 doubles per entry (A.re, A.im, B.re, B.im, R), level
 * after level from level 0.  levels == 0: an empty table, or none (bits = -1, the plain scaled loop).
 *
 * Beside the results the model watches the u chain: every value the derivative's operations produce (the products B Sinv, the
 * inner fma or product and both components of nu) — the smallest and the largest nonzero finite magnitude among them, and
 * whether any of them was subnormal.
 *
 * Compiled by tests/de_scaled_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused multiply-add but
 * the explicit fma() calls), into a temporary directory.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>

typedef struct {
    uint32_t width, height, iterations;
    int julia;
    double limit, scale_re, scale_im;
} desm_view;

typedef struct {
    double are, aim, bre, bim, R;
} desm_entry;

typedef struct {
    const double *x;
    uint32_t last;
    uint32_t levels;
    uint32_t n[33];
    uint64_t off[33];
    const desm_entry *e;
} desm_orbit;

/* what the u chain went through: [0] the smallest, [1] the largest nonzero finite magnitude; sub: a subnormal was seen */
typedef struct {
    double lo, hi;
    int sub;
} desm_range;

#define BIG 0x1p500

static void orbit_init(desm_orbit *o, const double *x, uint32_t last, const double *table, const uint32_t *n, uint32_t levels) {
    o->x = x;
    o->last = last;
    o->levels = levels;
    o->e = (const desm_entry *)table;
    uint64_t off = 0;
    for (uint32_t k = 0; k < levels; k++) {
        o->n[k] = n[k];
        o->off[k] = off;
        off += n[k];
    }
}

static double seen(desm_range *r, double v) {
    const double a = fabs(v);
    if (a != 0.0 && isfinite(a)) {
        if (a < r->lo) r->lo = a;
        if (a > r->hi) r->hi = a;
        if (a < DBL_MIN) r->sub = 1;
    }
    return v;
}

static int is_big(double wr, double wi) {
    const double a = fabs(wr), b = fabs(wi);
    return (a > b ? a : b) >= BIG;
}

/* out: z.re, z.im, u.re, u.im */
static uint32_t pixel(const desm_view *v, const desm_orbit *ox, const desm_orbit *ok, uint64_t x, uint64_t y, double out[4],
                      uint32_t *passes, uint32_t *skips, desm_range *rg) {
    /* the constants of a view */
    int e;
    const double sa = fabs(v->scale_re), sb = fabs(v->scale_im);
    (void)frexp(sa > sb ? sa : sb, &e);
    const double S = ldexp(1.0, e), Sinv = ldexp(1.0, -e);
    const double sre = v->scale_re * Sinv, sim = v->scale_im * Sinv;
    const double w = (double)v->width, h = (double)v->height;
    const double ore = (((double)x / h) - ((w / h) / 2.0)) / sre;
    const double oim = (((double)y / h) - 0.5) / sim;
    const double squared = v->limit * v->limit;
    const double bs0 = v->julia ? 0.0 : Sinv;
    const uint32_t iterations = v->iterations;
    const desm_orbit *o = ox;
    uint32_t m = v->julia ? 0u : 1u;
    double wr = ore, wi = oim;
    const double wcr = v->julia ? 0.0 : ore, wci = v->julia ? 0.0 : oim;
    double zr = fma(wr, Sinv, o->x[2 * m]), zi = fma(wi, Sinv, o->x[2 * m + 1]);
    double ur = Sinv, ui = 0.0; /* u0 = (Sinv, 0) */
    uint32_t i = 0, np = 0, ns = 0, result = iterations;
    while (i < iterations) {
        np++;
        /* 1. the level: SCALED PT's search */
        uint32_t K = 0;
        if (m >= 1 && o->levels) {
            const uint32_t j = m - 1;
            const double f = is_big(wr, wi) ? Sinv : 1.0;
            const double ar = wr * f, ai = wi * f;
            const double d2 = ar * ar + ai * ai;
            for (uint32_t k = 1; k < o->levels; k++) {
                if (j % (1u << k) != 0) break;
                if ((j >> k) >= o->n[k]) break;
                if ((uint64_t)i + (1u << k) > iterations) break;
                const double Rf = o->e[o->off[k] + (j >> k)].R * f;
                if (!(d2 < Rf * Rf)) break;
                K = k;
            }
        }
        /* 2. the step, and the scaled derivative's beside it */
        double nwr, nwi, nur, nui;
        if (K == 0) {
            const double tr = o->x[2 * m] + zr, ti = o->x[2 * m + 1] + zi;
            nwr = fma(tr, wr, fma(-ti, wi, wcr));
            nwi = fma(tr, wi, fma(ti, wr, wci));
            const double gr = zr + zr, gi = zi + zi; /* from the z the loop holds before the step */
            nur = seen(rg, fma(gr, ur, seen(rg, fma(-gi, ui, bs0))));
            nui = seen(rg, fma(gr, ui, seen(rg, gi * ur)));
            m += 1;
            i += 1;
        } else {
            const desm_entry *en = &o->e[o->off[K] + ((m - 1) >> K)];
            nwr = fma(en->are, wr, fma(-en->aim, wi, fma(en->bre, wcr, -(en->bim * wci))));
            nwi = fma(en->are, wi, fma(en->aim, wr, fma(en->bre, wci, en->bim * wcr)));
            const double br = v->julia ? 0.0 : seen(rg, en->bre * Sinv), bi = v->julia ? 0.0 : seen(rg, en->bim * Sinv);
            nur = seen(rg, fma(en->are, ur, seen(rg, fma(-en->aim, ui, br))));
            nui = seen(rg, fma(en->are, ui, seen(rg, fma(en->aim, ur, bi))));
            m += 1u << K;
            i += 1u << K;
            ns++;
        }
        if (m > o->last) return 0xFFFFFFFFu; /* the definition never gets here */
        zr = fma(nwr, Sinv, o->x[2 * m]);
        zi = fma(nwi, Sinv, o->x[2 * m + 1]);
        wr = nwr;
        wi = nwi;
        ur = nur; /* escape returns nu; otherwise u = nu */
        ui = nui;
        /* 3. the tests, SCALED PT's; a rebase never touches u */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) {
            result = i - 1; /* i counts the steps taken here: the plain loop's index i and the table form's i - 1 are this one */
            break;
        }
        int rebase;
        if (is_big(wr, wi)) {
            const double dr = wr * Sinv, di = wi * Sinv;
            rebase = dist < dr * dr + di * di;
        } else {
            const double ar = zr * S, ai = zi * S;
            rebase = ar * ar + ai * ai < wr * wr + wi * wi;
        }
        if (rebase || m == o->last) {
            wr = zr * S;
            wi = zi * S;
            m = 0;
            o = ok;
        }
    }
    out[0] = zr, out[1] = zi, out[2] = ur, out[3] = ui;
    *passes = np;
    *skips = ns;
    return result;
}

/* rows [y0, y1): z[2p], z[2p+1]; iters[p]; der[2p], der[2p+1] = u; passes[p], skips[p]; p = (y - y0) * width + x.  escape == 0
 * (an algorithm without orbits): zeros in all of them.  range[0], range[1]: the smallest and the largest nonzero finite magnitude
 * of the u chain over these rows (+inf and 0 when it produced none).  Returns 1 if the chain held a subnormal, else 0; -1 if a
 * step went past the end of an orbit. */
int desm_rows(const desm_view *v, int escape, const double *x, uint32_t x_last, const double *x_table, const uint32_t *x_n,
              uint32_t x_levels, const double *k, uint32_t k_last, const double *k_table, const uint32_t *k_n, uint32_t k_levels,
              uint32_t y0, uint32_t y1, double *z, uint32_t *iters, double *der, uint32_t *passes, uint32_t *skips, double *range) {
    desm_orbit ox, ok;
    desm_range rg = {INFINITY, 0.0, 0};
    int good = 1;
    if (escape) {
        orbit_init(&ox, x, x_last, x_table, x_n, x_levels);
        orbit_init(&ok, k, k_last, k_table, k_n, k_levels);
    }
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t xx = 0; xx < v->width; xx++) {
            const uint64_t p = (uint64_t)(y - y0) * v->width + xx;
            double o[4] = {0.0, 0.0, 0.0, 0.0};
            passes[p] = skips[p] = 0;
            iters[p] = escape ? pixel(v, &ox, &ok, xx, y, o, &passes[p], &skips[p], &rg) : 0u;
            if (escape && iters[p] == 0xFFFFFFFFu) good = 0;
            z[2 * p] = o[0], z[2 * p + 1] = o[1], der[2 * p] = o[2], der[2 * p + 1] = o[3];
        }
    range[0] = rg.lo;
    range[1] = rg.hi;
    return good ? rg.sub : -1;
}
