/*
 * pt_scaled_model.c — host restatement of SCALED PT (include/fractal_hip.h, fr_precision: "SCALED PT"), written from the
 * definition alone: the checker the device kernels (fractal-renderer_amd/csrc/fr_scaled.hip) and the library's host table
 * are compared with bit for bit.  Orbits are passed in as arrays of stored f64 entries; tests/pt_wide_model.py computes
 * them on Python integers.
 *
 * Compiled by tests/pt_scaled_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused multiply-add
 * but the explicit fma() calls), into a temporary directory.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    uint32_t width, height, iterations;
    int julia;
    double limit, scale_re, scale_im;
} ptsm_view;

/* the constants of a view */
typedef struct {
    int e;
    double S, Sinv, sre, sim;
} ptsm_consts;

typedef struct {
    double are, aim, bre, bim, R;
} ptsm_entry;

/* the table of one orbit: level k at e[off[k]], n[k] entries; levels == 0: empty, or no table (bits = -1) */
typedef struct {
    uint32_t levels;
    uint32_t n[33];
    uint64_t off[33];
    ptsm_entry *e;
} ptsm_table;

#define BIG 0x1p500
#define R_MIN 0x1p-53

static ptsm_consts consts(const ptsm_view *v) {
    ptsm_consts c;
    const double a = fabs(v->scale_re), b = fabs(v->scale_im);
    (void)frexp(a > b ? a : b, &c.e);
    c.S = ldexp(1.0, c.e);
    c.Sinv = ldexp(1.0, -c.e);
    c.sre = v->scale_re * c.Sinv;
    c.sim = v->scale_im * c.Sinv;
    return c;
}

int ptsm_e(const ptsm_view *v) { return consts(v).e; }

static double woff_re(const ptsm_view *v, const ptsm_consts *c, uint64_t x) {
    const double w = (double)v->width, h = (double)v->height;
    return (((double)x / h) - ((w / h) / 2.0)) / c->sre;
}

static double woff_im(const ptsm_view *v, const ptsm_consts *c, uint64_t y) {
    const double h = (double)v->height;
    return (((double)y / h) - 0.5) / c->sim;
}

/* Dw: the bound of |wc| over the whole image */
double ptsm_Dw(const ptsm_view *v) {
    const ptsm_consts k = consts(v);
    const double a = fabs(woff_re(v, &k, 0)), b = fabs(woff_re(v, &k, v->width ? v->width - 1u : 0u));
    const double c = fabs(woff_im(v, &k, 0)), d = fabs(woff_im(v, &k, v->height ? v->height - 1u : 0u));
    const double mrw = a > b ? a : b, miw = c > d ? c : d;
    return sqrt(mrw * mrw + miw * miw);
}

/* entries of all levels of the table of an orbit with last index `last` */
uint64_t ptsm_table_entries(uint32_t last) {
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

static double stored_R(double R) { return R < R_MIN ? 0.0 : R; }

static void build(const double *X, uint32_t last, double Dw, double S, double b0, int bits, ptsm_table *t, ptsm_entry *store) {
    t->levels = 0;
    t->e = store;
    if (last < 2) return;
    const double epsS = ldexp(1.0, -bits) * S;
    uint32_t n = last - 1;
    uint64_t off = 0;
    t->n[0] = n;
    t->off[0] = 0;
    /* the radius before the 2^-53 rule is what a merge reads: keep it beside the entries, level by level */
    double *r_prev = malloc((size_t)n * sizeof(double));
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t m = j + 1;
        ptsm_entry *e = &store[j];
        e->are = X[2 * m] + X[2 * m];
        e->aim = X[2 * m + 1] + X[2 * m + 1];
        e->bre = b0;
        e->bim = 0.0;
        r_prev[j] = epsS * sqrt(e->are * e->are + e->aim * e->aim);
        e->R = stored_R(r_prev[j]);
    }
    uint32_t k = 0;
    while (n >= 2) {
        const uint32_t nn = n / 2;
        const ptsm_entry *lo = store + off;
        off += n;
        ptsm_entry *hi = store + off;
        for (uint32_t j = 0; j < nn; j++) {
            const ptsm_entry *x = &lo[2 * j], *y = &lo[2 * j + 1];
            const double Rx = r_prev[2 * j], Ry = r_prev[2 * j + 1];
            ptsm_entry *e = &hi[j];
            e->are = fma(y->are, x->are, -(y->aim * x->aim));
            e->aim = fma(y->are, x->aim, y->aim * x->are);
            e->bre = fma(y->are, x->bre, -(y->aim * x->bim)) + y->bre;
            e->bim = fma(y->are, x->bim, y->aim * x->bre) + y->bim;
            double Q = (Ry - sqrt(x->bre * x->bre + x->bim * x->bim) * Dw) / sqrt(x->are * x->are + x->aim * x->aim);
            if (!(Q > 0.0)) Q = 0.0;
            const double R = Rx < Q ? Rx : Q;
            e->R = stored_R(R);
            r_prev[j] = R; /* j <= 2j: entry j of the new level overwrites a slot already consumed */
        }
        k++;
        n = nn;
        t->n[k] = n;
        t->off[k] = off;
    }
    t->levels = k + 1;
    free(r_prev);
}

/* The table of orbit X (re, im pairs, entries 0 .. last) into out, 5 doubles per entry (A.re, A.im, B.re, B.im, R), level
 * after level; n_out[k] = entries of level k for k < the returned number of levels.  out has room for
 * ptsm_table_entries(last) entries, n_out for 33 levels. */
uint32_t ptsm_build_table(const ptsm_view *v, const double *X, uint32_t last, int bits, double *out, uint32_t *n_out) {
    ptsm_table t;
    build(X, last, ptsm_Dw(v), consts(v).S, v->julia ? 0.0 : 1.0, bits, &t, (ptsm_entry *)out);
    for (uint32_t k = 0; k < t.levels; k++) n_out[k] = t.n[k];
    return t.levels;
}

typedef struct {
    const double *x;
    uint32_t last;
    const ptsm_table *t;
} followed;

static int is_big(double wr, double wi) {
    const double a = fabs(wr), b = fabs(wi);
    return (a > b ? a : b) >= BIG;
}

static uint32_t pixel(const ptsm_view *v, const ptsm_consts *c, const followed *ox, const followed *ok, uint64_t x, uint64_t y,
                      double *out_re, double *out_im, uint32_t *passes, uint32_t *rebases) {
    const double S = c->S, Sinv = c->Sinv;
    const double ore = woff_re(v, c, x), oim = woff_im(v, c, y);
    const double squared = v->limit * v->limit;
    const uint32_t iterations = v->iterations;
    const followed *o = ox;
    uint32_t m = v->julia ? 0u : 1u;
    double wr = ore, wi = oim;
    const double wcr = v->julia ? 0.0 : ore, wci = v->julia ? 0.0 : oim;
    double zr = fma(wr, Sinv, o->x[2 * m]), zi = fma(wi, Sinv, o->x[2 * m + 1]);
    uint32_t i = 0, np = 0, nreb = 0;
    *passes = *rebases = 0;
    while (i < iterations) {
        np++;
        /* 1. pick the level */
        uint32_t K = 0;
        if (m >= 1 && o->t->levels) {
            const uint32_t j = m - 1;
            const double f = is_big(wr, wi) ? Sinv : 1.0;
            const double ar = wr * f, ai = wi * f;
            const double d2 = ar * ar + ai * ai;
            for (uint32_t k = 1; k < o->t->levels; k++) {
                if (j % (1u << k) != 0) break;
                if ((j >> k) >= o->t->n[k]) break;
                if ((uint64_t)i + (1u << k) > iterations) break;
                const double Rf = o->t->e[o->t->off[k] + (j >> k)].R * f;
                if (!(d2 < Rf * Rf)) break;
                K = k;
            }
        }
        /* 2. step */
        double nwr, nwi;
        if (K == 0) {
            const double tr = o->x[2 * m] + zr, ti = o->x[2 * m + 1] + zi;
            nwr = fma(tr, wr, fma(-ti, wi, wcr));
            nwi = fma(tr, wi, fma(ti, wr, wci));
            m += 1;
            i += 1;
        } else {
            const ptsm_entry *e = &o->t->e[o->t->off[K] + ((m - 1) >> K)];
            nwr = fma(e->are, wr, fma(-e->aim, wi, fma(e->bre, wcr, -(e->bim * wci))));
            nwi = fma(e->are, wi, fma(e->aim, wr, fma(e->bre, wci, e->bim * wcr)));
            m += 1u << K;
            i += 1u << K;
        }
        if (m > o->last) return 0xFFFFFFFFu; /* the definition never gets here */
        zr = fma(nwr, Sinv, o->x[2 * m]);
        zi = fma(nwi, Sinv, o->x[2 * m + 1]);
        wr = nwr;
        wi = nwi;
        /* 3. test */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) {
            *out_re = zr;
            *out_im = zi;
            *passes = np;
            *rebases = nreb;
            return i - 1;
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
            nreb++;
        }
    }
    *out_re = zr;
    *out_im = zi;
    *passes = np;
    *rebases = nreb;
    return iterations;
}

/* rows [y0, y1): z2[2k], z2[2k+1] = re, im; iters[k]; passes[k] = passes through the loop; rebases[k]; k = (y - y0) * width
 * + x.  x: the orbit a pixel starts on (R or V), k: the one it rebases onto (R again, or K).  bits = -1: no table, the plain
 * scaled loop.  Returns 0 on allocation failure or if a step went past the end of an orbit. */
int ptsm_rows(const ptsm_view *v, const double *x, uint32_t x_last, const double *k, uint32_t k_last, int bits, uint32_t y0,
              uint32_t y1, double *z2, uint32_t *iters, uint32_t *passes, uint32_t *rebases) {
    const ptsm_consts c = consts(v);
    const double Dw = ptsm_Dw(v), b0 = v->julia ? 0.0 : 1.0;
    ptsm_table tx, tk;
    tx.levels = tk.levels = 0;
    ptsm_entry *sx = NULL, *sk = NULL;
    if (bits >= 0) {
        sx = malloc((size_t)(ptsm_table_entries(x_last) + 1) * sizeof(ptsm_entry));
        if (!sx) return 0;
        build(x, x_last, Dw, c.S, b0, bits, &tx, sx);
    }
    followed ox = {x, x_last, &tx}, ok = ox;
    if (v->julia) {
        if (bits >= 0) {
            sk = malloc((size_t)(ptsm_table_entries(k_last) + 1) * sizeof(ptsm_entry));
            if (!sk) {
                free(sx);
                return 0;
            }
            build(k, k_last, Dw, c.S, b0, bits, &tk, sk);
        }
        ok.x = k, ok.last = k_last, ok.t = &tk;
    }
    int good = 1;
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t xx = 0; xx < v->width; xx++) {
            const uint64_t p = (uint64_t)(y - y0) * v->width + xx;
            iters[p] = pixel(v, &c, &ox, &ok, xx, y, &z2[2 * p], &z2[2 * p + 1], &passes[p], &rebases[p]);
            if (iters[p] == 0xFFFFFFFFu) good = 0;
        }
    free(sx);
    free(sk);
    return good;
}

/* ptsm_rows with a FOREIGN table: the tables are built with tv's Dw and S, everything else — the pixel loop's constants, the
 * offsets, the cap, the limit, the orbits — is v's.  What a kernel computes that is handed the tables of another view on the
 * same orbits (tests/test_table_cache_cpu.py).  tv = v: ptsm_rows, bit for bit.  bits >= 0. */
int ptsm_rows_table_of(const ptsm_view *v, const ptsm_view *tv, const double *x, uint32_t x_last, const double *k, uint32_t k_last,
                       int bits, uint32_t y0, uint32_t y1, double *z2, uint32_t *iters, uint32_t *passes, uint32_t *rebases) {
    const ptsm_consts c = consts(v);
    const double Dw = ptsm_Dw(tv), S = consts(tv).S, b0 = v->julia ? 0.0 : 1.0;
    ptsm_table tx, tk;
    tx.levels = tk.levels = 0;
    ptsm_entry *sx = NULL, *sk = NULL;
    if (bits < 0) return 0;
    sx = malloc((size_t)(ptsm_table_entries(x_last) + 1) * sizeof(ptsm_entry));
    if (!sx) return 0;
    build(x, x_last, Dw, S, b0, bits, &tx, sx);
    followed ox = {x, x_last, &tx}, ok = ox;
    if (v->julia) {
        sk = malloc((size_t)(ptsm_table_entries(k_last) + 1) * sizeof(ptsm_entry));
        if (!sk) {
            free(sx);
            return 0;
        }
        build(k, k_last, Dw, S, b0, bits, &tk, sk);
        ok.x = k, ok.last = k_last, ok.t = &tk;
    }
    int good = 1;
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t xx = 0; xx < v->width; xx++) {
            const uint64_t p = (uint64_t)(y - y0) * v->width + xx;
            iters[p] = pixel(v, &c, &ox, &ok, xx, y, &z2[2 * p], &z2[2 * p + 1], &passes[p], &rebases[p]);
            if (iters[p] == 0xFFFFFFFFu) good = 0;
        }
    free(sx);
    free(sk);
    return good;
}
