/*
 * de_scaled_state_model.c — host restatement of RESUMABLE SCALED DE (include/fractal_hip.h, fr_precision: "RESUMABLE SCALED
 * DE"), written from the definition alone: SCALED PT's plain loop (bits = -1) on w = dz 2^e with the state rule — a pixel
 * rebases on the scaled rebase test, or at m == last of X only when X is ENDED BY ESCAPE — and beside it the scaled derivative
 * u = d 2^-e of DE ON SCALED PT's plain step, from the z the loop holds before the step.  A rebase never touches u.  Orbits are
 * passed in as arrays of stored f64 entries with their ended flags; tests/pt_wide_model.py computes them on Python integers.
 *
 * Compiled by tests/de_scaled_state_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused
 * multiply-add but the explicit fma() calls), into a temporary directory.
 */
#include <math.h>
#include <stdint.h>

typedef struct {
    uint32_t width, height, iterations;
    int julia;
    double limit, scale_re, scale_im;
} view;

typedef struct {
    const double *v; /* re, im pairs, entries 0 .. last */
    uint32_t last;
    int ended; /* ended by escape (else cut by the cap) */
} orbit;

typedef struct {
    double zr, zi, wr, wi, ur, ui;
    uint32_t m;
    int on_k;
} state;

#define ON_K 0x80000000u
#define BIG 0x1p500

/* the constants of a view: max |scale| = f 2^e with 0.5 <= f < 1 */
typedef struct {
    double S, Sinv, sre, sim;
} consts;

static consts view_consts(const view *v) {
    consts c;
    int e;
    const double a = fabs(v->scale_re), b = fabs(v->scale_im);
    (void)frexp(a > b ? a : b, &e);
    c.S = ldexp(1.0, e);
    c.Sinv = ldexp(1.0, -e);
    c.sre = v->scale_re * c.Sinv;
    c.sim = v->scale_im * c.Sinv;
    return c;
}

static int big(double wr, double wi) {
    const double a = fabs(wr), b = fabs(wi);
    return (a > b ? a : b) >= BIG;
}

/* steps from .. to - 1 on a running pixel.  Returns the escape index, or `to`.  *violations counts the steps that began with
 * m >= last of the orbit followed (the definition needs X_{m+1}). */
static uint32_t run(const view *v, const consts *c, const orbit *x, const orbit *k, double woff_re, double woff_im, uint32_t from,
                    uint32_t to, state *s, uint64_t *violations) {
    const double S = c->S, Sinv = c->Sinv;
    const double squared = v->limit * v->limit;
    const double wcr = v->julia ? 0.0 : woff_re, wci = v->julia ? 0.0 : woff_im;
    const double bs0 = v->julia ? 0.0 : Sinv;
    const orbit *X = s->on_k ? k : x;
    for (uint32_t i = from; i < to; i++) {
        if (s->m >= X->last) {
            (*violations)++;
            return to;
        }
        /* the derivative: from the z before the step */
        const double gr = s->zr + s->zr, gi = s->zi + s->zi;
        const double nur = fma(gr, s->ur, fma(-gi, s->ui, bs0));
        const double nui = fma(gr, s->ui, gi * s->ur);
        /* SCALED PT's step */
        const double tr = X->v[2 * s->m] + s->zr, ti = X->v[2 * s->m + 1] + s->zi;
        const double nwr = fma(tr, s->wr, fma(-ti, s->wi, wcr));
        const double nwi = fma(tr, s->wi, fma(ti, s->wr, wci));
        s->m++;
        s->zr = fma(nwr, Sinv, X->v[2 * s->m]);
        s->zi = fma(nwi, Sinv, X->v[2 * s->m + 1]);
        s->wr = nwr;
        s->wi = nwi;
        s->ur = nur; /* escape stores nu; otherwise u = nu */
        s->ui = nui;
        const double dist = s->zr * s->zr + s->zi * s->zi;
        if (dist > squared) {
            s->wr = s->wi = 0.0;
            s->m = 0;
            s->on_k = 0;
            return i;
        }
        int test;
        if (big(s->wr, s->wi)) {
            const double dr = s->wr * Sinv, di = s->wi * Sinv;
            test = dist < dr * dr + di * di;
        } else {
            const double ar = s->zr * S, ai = s->zi * S;
            test = ar * ar + ai * ai < s->wr * s->wr + s->wi * s->wi;
        }
        if (test || (s->m == X->last && X->ended)) { /* a rebase never touches u */
            s->wr = s->zr * S;
            s->wi = s->zi * S;
            s->m = 0;
            if (v->julia) {
                X = k;
                s->on_k = 1;
            }
        }
    }
    return to;
}

/* Rows [y0, y1) from cap `from` to v->iterations.  fresh != 0: from the initial state (`from` is 0 then), every pixel
 * written.  Otherwise the arrays hold the state at `from` and are continued in place: a pixel with iters != from is not
 * touched.  z, w, der: re, im per pixel; m: bit 31 = on K.  Mandelbrot: pass the same orbit for x and k.  orbits == 0: an
 * algorithm without orbits, zeros in all five arrays. */
void dessm_rows(const view *v, int orbits, const double *x, uint32_t x_last, int x_ended, const double *k, uint32_t k_last, int k_ended,
                uint32_t y0, uint32_t y1, uint32_t from, int fresh, double *z, uint32_t *iters, double *w, uint32_t *m, double *der,
                uint64_t *violations) {
    const orbit ox = {x, x_last, x_ended}, ok = {k, k_last, k_ended};
    const consts c = view_consts(v);
    const double wd = (double)v->width, h = (double)v->height;
    uint64_t viol = 0;
    for (uint32_t y = y0; y < y1; y++) {
        for (uint32_t px = 0; px < v->width; px++) {
            const uint64_t i = (uint64_t)(y - y0) * v->width + px;
            if (!orbits) {
                z[2 * i] = z[2 * i + 1] = w[2 * i] = w[2 * i + 1] = der[2 * i] = der[2 * i + 1] = 0.0;
                iters[i] = m[i] = 0;
                continue;
            }
            const double woff_re = (((double)px / h) - ((wd / h) / 2.0)) / c.sre;
            const double woff_im = (((double)y / h) - 0.5) / c.sim;
            state s;
            if (fresh) {
                s.m = v->julia ? 0u : 1u;
                s.on_k = 0;
                s.wr = woff_re;
                s.wi = woff_im;
                s.zr = fma(s.wr, c.Sinv, x[2 * s.m]);
                s.zi = fma(s.wi, c.Sinv, x[2 * s.m + 1]);
                s.ur = c.Sinv; /* u0 = (Sinv, 0) */
                s.ui = 0.0;
            } else {
                if (iters[i] != from) continue;
                s.zr = z[2 * i], s.zi = z[2 * i + 1], s.wr = w[2 * i], s.wi = w[2 * i + 1];
                s.ur = der[2 * i], s.ui = der[2 * i + 1];
                s.m = m[i] & ~ON_K;
                s.on_k = (m[i] & ON_K) != 0;
            }
            iters[i] = run(v, &c, &ox, &ok, woff_re, woff_im, from, v->iterations, &s, &viol);
            z[2 * i] = s.zr, z[2 * i + 1] = s.zi, w[2 * i] = s.wr, w[2 * i + 1] = s.wi;
            der[2 * i] = s.ur, der[2 * i + 1] = s.ui;
            m[i] = s.m | (s.on_k ? ON_K : 0u);
        }
    }
    *violations = viol;
}
