/*
 * pt_wide_model.c — the pixel loop of WIDE PT (include/fractal_hip.h, fr_precision: "WIDE PT"), which is PT's and RESUMABLE
 * PT's step sequence over reference orbits that are PASSED IN: tests/pt_wide_model.py computes them on Python integers.
 * Written from the definition alone; Python 3.10 has no fma, hence C.
 *
 * `rule` 0 is the state rule (a pixel rebases at m == last of X only when X is ended by escape); `rule` 1 is PT's own rule
 * (rebase at m == last of X whatever ended X): z and iters of a fresh run under either are PT's.
 *
 * Compiled by tests/pt_wide_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared, into a temporary
 * directory.
 */
#include <math.h>
#include <stdint.h>

typedef struct {
    const double *v; /* re, im pairs, entries 0 .. last */
    uint32_t last;
    int ended; /* ended by escape (else cut by the cap) */
} orbit;

typedef struct {
    uint32_t width, height, iterations;
    int julia;
    double limit, scale_re, scale_im;
} view;

typedef struct {
    double zr, zi, dzr, dzi;
    uint32_t m;
    int on_k;
} state;

#define ON_K 0x80000000u

/* steps from .. to - 1 on a running pixel.  Returns the escape index, or `to`.  *violations counts the steps that began with
 * m >= last of the orbit followed (the definition needs X_{m+1}); *rebases the rebases of this pixel. */
static uint32_t run(const view *v, const orbit *x, const orbit *k, double off_re, double off_im, uint32_t from, uint32_t to, int rule,
                    state *s, uint32_t *rebases, uint64_t *violations) {
    const double squared = v->limit * v->limit;
    const double dcr = v->julia ? 0.0 : off_re, dci = v->julia ? 0.0 : off_im;
    const orbit *X = s->on_k ? k : x;
    for (uint32_t i = from; i < to; i++) {
        if (s->m >= X->last) {
            (*violations)++;
            return to;
        }
        const double tr = X->v[2 * s->m] + s->zr, ti = X->v[2 * s->m + 1] + s->zi;
        const double ndr = fma(tr, s->dzr, fma(-ti, s->dzi, dcr));
        const double ndi = fma(tr, s->dzi, fma(ti, s->dzr, dci));
        s->m++;
        s->zr = X->v[2 * s->m] + ndr;
        s->zi = X->v[2 * s->m + 1] + ndi;
        s->dzr = ndr;
        s->dzi = ndi;
        const double dist = s->zr * s->zr + s->zi * s->zi;
        if (dist > squared) {
            s->dzr = s->dzi = 0.0;
            s->m = 0;
            s->on_k = 0;
            return i;
        }
        if (dist < s->dzr * s->dzr + s->dzi * s->dzi || (s->m == X->last && (X->ended || rule == 1))) {
            s->dzr = s->zr;
            s->dzi = s->zi;
            s->m = 0;
            (*rebases)++;
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
 * touched.  z, dz: re, im per pixel; m: bit 31 = on K; rebases (may be NULL): per pixel, the rebases of this call.
 * Mandelbrot: pass the same orbit for x and k. */
void ptwm_rows(const view *v, const double *x, uint32_t x_last, int x_ended, const double *k, uint32_t k_last, int k_ended,
               uint32_t y0, uint32_t y1, uint32_t from, int fresh, int rule, double *z, uint32_t *iters, double *dz, uint32_t *m,
               uint32_t *rebases, uint64_t *violations) {
    const orbit ox = {x, x_last, x_ended}, ok = {k, k_last, k_ended};
    const double w = (double)v->width, h = (double)v->height;
    uint64_t viol = 0;
    for (uint32_t y = y0; y < y1; y++) {
        for (uint32_t px = 0; px < v->width; px++) {
            const uint64_t i = (uint64_t)(y - y0) * v->width + px;
            const double off_re = (((double)px / h) - ((w / h) / 2.0)) / v->scale_re;
            const double off_im = (((double)y / h) - 0.5) / v->scale_im;
            state s;
            uint32_t nreb = 0;
            if (fresh) {
                s.m = v->julia ? 0u : 1u;
                s.on_k = 0;
                s.dzr = off_re;
                s.dzi = off_im;
                s.zr = x[2 * s.m] + s.dzr;
                s.zi = x[2 * s.m + 1] + s.dzi;
            } else {
                if (rebases) rebases[i] = 0;
                if (iters[i] != from) continue;
                s.zr = z[2 * i], s.zi = z[2 * i + 1], s.dzr = dz[2 * i], s.dzi = dz[2 * i + 1];
                s.m = m[i] & ~ON_K;
                s.on_k = (m[i] & ON_K) != 0;
            }
            iters[i] = run(v, &ox, &ok, off_re, off_im, from, v->iterations, rule, &s, &nreb, &viol);
            z[2 * i] = s.zr, z[2 * i + 1] = s.zi, dz[2 * i] = s.dzr, dz[2 * i + 1] = s.dzi;
            m[i] = s.m | (s.on_k ? ON_K : 0u);
            if (rebases) rebases[i] = nreb;
        }
    }
    if (violations) *violations = viol;
}
