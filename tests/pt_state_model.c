/*
 * pt_state_model.c — host restatement of the resumable PT state (include/fractal_hip.h, fr_precision: "RESUMABLE PT"),
 * written from the definition alone: the checker escape_pt_state_kernel and escape_extend_pt_kernel
 * (fractal-renderer_amd/csrc/fr_pt.hip) are compared with bit for bit, and itself compared with tests/pt_model.c, the
 * restatement of PT, in tests/test_pt_state_cpu.py.
 *
 * `rule` 0 is the definition: a pixel rebases at m == last of X only when X is ended by escape.  `rule` 1 is PT's own rule
 * (rebase at m == last of X whatever ended X), i.e. the state one would get by storing PT's registers: kept to show that
 * such a state does NOT continue to the higher cap.
 *
 * Compiled by tests/pt_state_model.py at run time: gcc -O2 -ffp-contract=off -fopenmp -shared (no fused multiply-add but
 * the explicit fma() calls, no fast-math), into a temporary directory.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    double re, im;
} sm_imaginary;

typedef struct {
    uint8_t r, g, b;
} sm_rgb;

/* fr_config, field for field (104 bytes) */
typedef struct {
    uint32_t algo, width, height, iterations;
    double limit, stable_limit;
    sm_imaginary pos, scale;
    double exposure;
    uint8_t inside, smooth;
    sm_rgb primary_color, secondary_color;
    double color_weight;
    sm_imaginary julia_set;
} sm_config;

typedef struct {
    double hi, lo;
} ddv;

/* ---- DD's operations (include/fractal_hip.h) ---- */

static ddv two_sum(double a, double b) {
    ddv r;
    double s = a + b;
    double bb = s - a;
    r.hi = s;
    r.lo = (a - (s - bb)) + (b - bb);
    return r;
}

static ddv fast_two_sum(double a, double b) {
    ddv r;
    double s = a + b;
    r.hi = s;
    r.lo = b - (s - a);
    return r;
}

static ddv add_dd(ddv a, ddv b) {
    ddv s = two_sum(a.hi, b.hi);
    ddv t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return fast_two_sum(s.hi, s.lo);
}

static ddv add_d(ddv a, double d) {
    ddv s = two_sum(a.hi, d);
    s.lo = s.lo + a.lo;
    return fast_two_sum(s.hi, s.lo);
}

static ddv sqr(ddv x) {
    double p = x.hi * x.hi;
    double e = fma(x.hi, x.hi, -p);
    e = fma(x.hi + x.hi, x.lo, e);
    return fast_two_sum(p, e);
}

static ddv twice_mul(ddv x, ddv y) {
    double p = x.hi * y.hi;
    double e = fma(x.hi, y.hi, -p);
    e = fma(x.hi, y.lo, e);
    e = fma(x.lo, y.hi, e);
    ddv h = fast_two_sum(p, e);
    ddv r;
    r.hi = h.hi + h.hi;
    r.lo = h.lo + h.lo;
    return r;
}

static ddv neg(ddv x) {
    ddv r;
    r.hi = -x.hi;
    r.lo = -x.lo;
    return r;
}

/* ---- reference orbits: entries 0 .. last, and whether the last one ended the orbit by the escape test ---- */

typedef struct {
    double *v; /* re, im pairs */
    uint32_t last;
    int ended;
} orbit;

/* which 0: R (Mandelbrot) or V (Julia); 1: K (Julia).  Returns 0 on allocation failure. */
static int make_orbit(const sm_config *cfg, double lo_re, double lo_im, int which, orbit *o) {
    const int julia = cfg->algo == 2;
    const uint32_t kmin = julia ? 1u : 2u;
    const uint32_t kmax = julia ? (cfg->iterations > 1 ? cfg->iterations : 1u) : cfg->iterations + 1u;
    const ddv cre = {cfg->pos.re, lo_re}, cim = {cfg->pos.im, lo_im};
    ddv zr = {0.0, 0.0}, zi = {0.0, 0.0};
    if (julia && which == 0) zr = cre, zi = cim;
    o->v = malloc(((size_t)kmax + 1) * 2 * sizeof(double));
    if (!o->v) return 0;
    uint32_t k = 0;
    for (;;) {
        o->v[2 * k] = zr.hi;
        o->v[2 * k + 1] = zi.hi;
        o->ended = k >= kmin && zr.hi * zr.hi + zi.hi * zi.hi > 4.0;
        if (o->ended) break;
        if (k == kmax) break;
        if (!julia && k == 0) {
            zr = cre, zi = cim; /* R_1 = C */
        } else {
            ddv a = add_dd(sqr(zr), neg(sqr(zi)));
            ddv b = twice_mul(zr, zi);
            if (julia) {
                zr = add_d(a, cfg->julia_set.re);
                zi = add_d(b, cfg->julia_set.im);
            } else {
                zr = add_dd(a, cre);
                zi = add_dd(b, cim);
            }
        }
        k++;
    }
    o->last = k;
    return 1;
}

typedef struct {
    orbit x, k; /* Mandelbrot: k is x */
    int julia;
} orbits;

static int make_orbits(const sm_config *cfg, double lo_re, double lo_im, orbits *o) {
    o->julia = cfg->algo == 2;
    if (!make_orbit(cfg, lo_re, lo_im, 0, &o->x)) return 0;
    if (o->julia) {
        if (!make_orbit(cfg, lo_re, lo_im, 1, &o->k)) {
            free(o->x.v);
            return 0;
        }
    } else {
        o->k = o->x;
    }
    return 1;
}

static void free_orbits(orbits *o) {
    if (o->julia) free(o->k.v);
    free(o->x.v);
}

/* out[0] = last, out[1] = ended by escape, of orbit `which` at cfg's cap.  Returns 0 on allocation failure. */
int ptsm_orbit_info(const sm_config *cfg, double lo_re, double lo_im, int which, uint32_t out[2]) {
    orbit o;
    if (!make_orbit(cfg, lo_re, lo_im, which, &o)) return 0;
    out[0] = o.last;
    out[1] = (uint32_t)o.ended;
    free(o.v);
    return 1;
}

/* ---- pixels ---- */

typedef struct {
    double zr, zi, dzr, dzi;
    uint32_t m;
    int on_k;
} state;

static void offsets(const sm_config *cfg, uint64_t x, uint64_t y, double *off_re, double *off_im) {
    const double w = (double)cfg->width, h = (double)cfg->height;
    *off_re = (((double)x / h) - ((w / h) / 2.0)) / cfg->scale.re;
    *off_im = (((double)y / h) - 0.5) / cfg->scale.im;
}

/* the state after 0 steps */
static void initial(const sm_config *cfg, const orbits *o, double off_re, double off_im, state *s) {
    s->m = o->julia ? 0u : 1u;
    s->on_k = 0;
    s->dzr = off_re;
    s->dzi = off_im;
    s->zr = o->x.v[2 * s->m] + s->dzr;
    s->zi = o->x.v[2 * s->m + 1] + s->dzi;
}

/* steps from .. to - 1 on a running pixel.  Returns the escape index, or `to`.  *violations counts the steps that began
 * with m >= last of the orbit followed (the definition needs X_{m+1}); such a pixel is left where it is. */
static uint32_t run(const sm_config *cfg, const orbits *o, double off_re, double off_im, uint32_t from, uint32_t to, int rule,
                    state *s, uint64_t *violations) {
    const double squared = cfg->limit * cfg->limit;
    const double dcr = o->julia ? 0.0 : off_re, dci = o->julia ? 0.0 : off_im;
    const orbit *X = s->on_k ? &o->k : &o->x;
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
            if (o->julia) {
                X = &o->k;
                s->on_k = 1;
            }
        }
    }
    return to;
}

static int escape_algo(const sm_config *cfg) { return cfg->algo == 0 || cfg->algo == 2; }

#define ON_K 0x80000000u

/* Rows [y0, y1) from cap `from` to cfg->iterations, on the orbits of cfg's cap.  fresh != 0: from the initial state (`from`
 * is 0 then), every pixel written.  Otherwise the arrays hold the state at `from` and are continued in place: a pixel with
 * iters != from is not touched.  z, dz: re, im per pixel; m: bit 31 = on K.  Returns 0 on allocation failure. */
int ptsm_rows(const sm_config *cfg, double lo_re, double lo_im, uint32_t y0, uint32_t y1, uint32_t from, int fresh, int rule,
              double *z, uint32_t *iters, double *dz, uint32_t *m, uint64_t *violations, int threads) {
    orbits o;
    const int esc = escape_algo(cfg);
    uint64_t viol = 0;
    if (esc && !make_orbits(cfg, lo_re, lo_im, &o)) return 0;
    const int64_t rows = (int64_t)y1 - (int64_t)y0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(+ : viol)
    for (int64_t r = 0; r < rows; r++) {
        for (uint32_t x = 0; x < cfg->width; x++) {
            const uint64_t k = (uint64_t)r * cfg->width + x;
            if (!esc) {
                if (fresh) z[2 * k] = z[2 * k + 1] = dz[2 * k] = dz[2 * k + 1] = 0.0, iters[k] = m[k] = 0;
                continue;
            }
            double off_re, off_im;
            offsets(cfg, x, (uint64_t)y0 + (uint64_t)r, &off_re, &off_im);
            state s;
            if (fresh) {
                initial(cfg, &o, off_re, off_im, &s);
            } else {
                if (iters[k] != from) continue;
                s.zr = z[2 * k], s.zi = z[2 * k + 1], s.dzr = dz[2 * k], s.dzi = dz[2 * k + 1];
                s.m = m[k] & ~ON_K;
                s.on_k = (m[k] & ON_K) != 0;
            }
            iters[k] = run(cfg, &o, off_re, off_im, from, cfg->iterations, rule, &s, &viol);
            z[2 * k] = s.zr, z[2 * k + 1] = s.zi, dz[2 * k] = s.dzr, dz[2 * k + 1] = s.dzi;
            m[k] = s.m | (s.on_k ? ON_K : 0u);
        }
    }
    if (esc) free_orbits(&o);
    if (violations) *violations = viol;
    return 1;
}
