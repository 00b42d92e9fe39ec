/*
 * bla_model.c — host restatement of BLA-PT (include/fractal_hip.h, fr_precision: "BLA-PT"), written from the definition
 * alone: the checker the device kernel (fractal-renderer_amd/csrc/fr_bla.hip) and the library's host table are compared
 * with bit for bit.  Orbits are passed in as arrays of stored f64 entries, so the dd road (tests/pt_model.py) and the wide
 * road (tests/pt_wide_model.py) both go through it.
 *
 * Compiled by tests/bla_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused multiply-add but
 * the explicit fma() calls), into a temporary directory.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    uint32_t width, height, iterations;
    int julia;
    double limit, scale_re, scale_im;
} blam_view;

typedef struct {
    double are, aim, bre, bim, r2;
} blam_entry;

/* the table of one orbit: level k at e[off[k]], n[k] entries; levels == 0: empty */
typedef struct {
    uint32_t levels;
    uint32_t n[33];
    uint64_t off[33];
    blam_entry *e;
} blam_table;

static double off_re(const blam_view *v, uint64_t x) {
    const double w = (double)v->width, h = (double)v->height;
    return (((double)x / h) - ((w / h) / 2.0)) / v->scale_re;
}

static double off_im(const blam_view *v, uint64_t y) {
    const double h = (double)v->height;
    return (((double)y / h) - 0.5) / v->scale_im;
}

/* D: the bound of |dc| over the whole image */
double blam_D(const blam_view *v) {
    const double a = fabs(off_re(v, 0)), b = fabs(off_re(v, v->width ? v->width - 1u : 0u));
    const double c = fabs(off_im(v, 0)), d = fabs(off_im(v, v->height ? v->height - 1u : 0u));
    const double mr = a > b ? a : b, mi = c > d ? c : d;
    return sqrt(mr * mr + mi * mi);
}

/* entries of all levels of the table of an orbit with last index `last` */
uint64_t blam_table_entries(uint32_t last) {
    if (last < 2) return 0;
    uint64_t total = 0;
    uint32_t n = last - 1;
    for (;;) {
        total += n;
        if (n < 2) break;
        n /= 2;
    }
    return total;
}

static void build(const double *X, uint32_t last, double D, double b0, int bits, blam_table *t, blam_entry *store) {
    t->levels = 0;
    t->e = store;
    if (last < 2) return;
    const double eps = ldexp(1.0, -bits);
    uint32_t n = last - 1;
    uint64_t off = 0;
    t->n[0] = n;
    t->off[0] = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t m = j + 1;
        blam_entry *e = &store[j];
        e->are = X[2 * m] + X[2 * m];
        e->aim = X[2 * m + 1] + X[2 * m + 1];
        e->bre = b0;
        e->bim = 0.0;
        const double r = eps * sqrt(e->are * e->are + e->aim * e->aim);
        e->r2 = r * r;
    }
    /* r itself is needed to merge: keep it beside the entries, level by level */
    double *r_prev = malloc((size_t)n * sizeof(double));
    for (uint32_t j = 0; j < n; j++) {
        const blam_entry *e = &store[j];
        r_prev[j] = eps * sqrt(e->are * e->are + e->aim * e->aim);
    }
    uint32_t k = 0;
    while (n >= 2) {
        const uint32_t nn = n / 2;
        const blam_entry *lo = store + off;
        off += n;
        blam_entry *hi = store + off;
        for (uint32_t j = 0; j < nn; j++) {
            const blam_entry *x = &lo[2 * j], *y = &lo[2 * j + 1];
            const double rx = r_prev[2 * j], ry = r_prev[2 * j + 1];
            blam_entry *e = &hi[j];
            e->are = fma(y->are, x->are, -(y->aim * x->aim));
            e->aim = fma(y->are, x->aim, y->aim * x->are);
            e->bre = fma(y->are, x->bre, -(y->aim * x->bim)) + y->bre;
            e->bim = fma(y->are, x->bim, y->aim * x->bre) + y->bim;
            double q = (ry - sqrt(x->bre * x->bre + x->bim * x->bim) * D) / sqrt(x->are * x->are + x->aim * x->aim);
            if (!(q > 0.0)) q = 0.0;
            const double r = rx < q ? rx : q;
            e->r2 = r * r;
            r_prev[j] = r; /* j <= 2j: entry j of the new level overwrites a slot already consumed */
        }
        k++;
        n = nn;
        t->n[k] = n;
        t->off[k] = off;
    }
    t->levels = k + 1;
    free(r_prev);
}

/* The table of orbit X (re, im pairs, entries 0 .. last) into out, 5 doubles per entry (A.re, A.im, B.re, B.im, r2), level
 * after level; n_out[k] = entries of level k for k < the returned number of levels.  out has room for
 * blam_table_entries(last) entries, n_out for 33 levels. */
uint32_t blam_build_table(const double *X, uint32_t last, double D, double b0, int bits, double *out, uint32_t *n_out) {
    blam_table t;
    build(X, last, D, b0, bits, &t, (blam_entry *)out);
    for (uint32_t k = 0; k < t.levels; k++) n_out[k] = t.n[k];
    return t.levels;
}

typedef struct {
    const double *x;
    uint32_t last;
    const blam_table *t;
} followed;

static uint32_t pixel(const blam_view *v, const followed *ox, const followed *ok, uint64_t x, uint64_t y, double *out_re,
                      double *out_im, uint32_t *passes) {
    const double ore = off_re(v, x), oim = off_im(v, y);
    const double squared = v->limit * v->limit;
    const uint32_t iterations = v->iterations;
    const followed *o = ox;
    uint32_t m = v->julia ? 0u : 1u;
    double dzr = ore, dzi = oim;
    const double dcr = v->julia ? 0.0 : ore, dci = v->julia ? 0.0 : oim;
    double zr = o->x[2 * m] + dzr, zi = o->x[2 * m + 1] + dzi;
    uint32_t i = 0, np = 0;
    while (i < iterations) {
        np++;
        /* 1. pick the level */
        const double d2 = dzr * dzr + dzi * dzi;
        uint32_t K = 0;
        if (m >= 1) {
            const uint32_t j = m - 1;
            for (uint32_t k = 1; k < o->t->levels; k++) {
                if (j % (1u << k) != 0) break;
                if ((j >> k) >= o->t->n[k]) break;
                if ((uint64_t)i + (1u << k) > iterations) break;
                if (!(d2 < o->t->e[o->t->off[k] + (j >> k)].r2)) break;
                K = k;
            }
        }
        /* 2. step */
        double ndr, ndi;
        if (K == 0) {
            const double tr = o->x[2 * m] + zr, ti = o->x[2 * m + 1] + zi;
            ndr = fma(tr, dzr, fma(-ti, dzi, dcr));
            ndi = fma(tr, dzi, fma(ti, dzr, dci));
            m += 1;
            i += 1;
        } else {
            const blam_entry *e = &o->t->e[o->t->off[K] + ((m - 1) >> K)];
            ndr = fma(e->are, dzr, fma(-e->aim, dzi, fma(e->bre, dcr, -(e->bim * dci))));
            ndi = fma(e->are, dzi, fma(e->aim, dzr, fma(e->bre, dci, e->bim * dcr)));
            m += 1u << K;
            i += 1u << K;
        }
        zr = o->x[2 * m] + ndr;
        zi = o->x[2 * m + 1] + ndi;
        dzr = ndr;
        dzi = ndi;
        /* 3. test */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) {
            *out_re = zr;
            *out_im = zi;
            *passes = np;
            return i - 1;
        }
        if (dist < dzr * dzr + dzi * dzi || m == o->last) {
            dzr = zr;
            dzi = zi;
            m = 0;
            o = ok;
        }
    }
    *out_re = zr;
    *out_im = zi;
    *passes = np;
    return iterations;
}

/* rows [y0, y1): z2[2k], z2[2k+1] = re, im; iters[k]; passes[k] = passes through the loop; k = (y - y0) * width + x.
 * x: the orbit a pixel starts on (R or V), k: the one it rebases onto (R again, or K).  Returns 0 on allocation failure. */
int blam_rows(const blam_view *v, const double *x, uint32_t x_last, const double *k, uint32_t k_last, int bits, uint32_t y0,
              uint32_t y1, double *z2, uint32_t *iters, uint32_t *passes) {
    const double D = blam_D(v), b0 = v->julia ? 0.0 : 1.0;
    blam_table tx, tk;
    blam_entry *sx = malloc((size_t)(blam_table_entries(x_last) + 1) * sizeof(blam_entry)), *sk = NULL;
    if (!sx) return 0;
    build(x, x_last, D, b0, bits, &tx, sx);
    followed ox = {x, x_last, &tx}, ok = ox;
    if (v->julia) {
        sk = malloc((size_t)(blam_table_entries(k_last) + 1) * sizeof(blam_entry));
        if (!sk) {
            free(sx);
            return 0;
        }
        build(k, k_last, D, b0, bits, &tk, sk);
        ok.x = k, ok.last = k_last, ok.t = &tk;
    }
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t xx = 0; xx < v->width; xx++) {
            const uint64_t p = (uint64_t)(y - y0) * v->width + xx;
            iters[p] = pixel(v, &ox, &ok, xx, y, &z2[2 * p], &z2[2 * p + 1], &passes[p]);
        }
    free(sx);
    free(sk);
    return 1;
}
