/*
 * dd_model.c — host restatement of FR_PRECISION_DD (include/fractal_hip.h, fr_precision), written from the definition
 * alone: the checker the device kernel (fractal-renderer_amd/csrc/fr_dd.hip) is compared with bit for bit.
 *
 * Compiled by tests/test_dd_model_cpu.py at run time: gcc -O2 -ffp-contract=off -fopenmp -shared (no fused
 * multiply-add but the explicit fma() calls, no fast-math), into a temporary directory.
 */
#include <math.h>
#include <stdint.h>

typedef struct {
    double re, im;
} ddm_imaginary;

typedef struct {
    uint8_t r, g, b;
} ddm_rgb;

/* fr_config, field for field (104 bytes) */
typedef struct {
    uint32_t algo, width, height, iterations;
    double limit, stable_limit;
    ddm_imaginary pos, scale;
    double exposure;
    uint8_t inside, smooth;
    ddm_rgb primary_color, secondary_color;
    double color_weight;
    ddm_imaginary julia_set;
} ddm_config;

typedef struct {
    double hi, lo;
} ddv;

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

/* the start of pixel (x, y): coord_to_space without `+ pos`, then add_d onto (pos, pos_lo) */
static void start_of(const ddm_config *cfg, double lo_re, double lo_im, uint64_t x, uint64_t y, ddv *re, ddv *im) {
    const double w = (double)cfg->width, h = (double)cfg->height;
    const double off_re = (((double)x / h) - ((w / h) / 2.0)) / cfg->scale.re;
    const double off_im = (((double)y / h) - 0.5) / cfg->scale.im;
    ddv pr = {cfg->pos.re, lo_re}, pi = {cfg->pos.im, lo_im};
    *re = add_d(pr, off_re);
    *im = add_d(pi, off_im);
}

/* recursive() in dd: (re, im) in, the result position out; returns the escape index */
static uint32_t orbit(const ddm_config *cfg, ddv *re, ddv *im) {
    const double squared = cfg->limit * cfg->limit;
    const int julia = cfg->algo == 2;
    const ddv cre = *re, cim = *im;
    ddv zr = *re, zi = *im;
    for (uint32_t i = 0; i < cfg->iterations; i++) {
        ddv a = add_dd(sqr(zr), neg(sqr(zi)));
        ddv b = twice_mul(zr, zi);
        ddv nr, ni;
        if (julia) {
            nr = add_d(a, cfg->julia_set.re);
            ni = add_d(b, cfg->julia_set.im);
        } else {
            nr = add_dd(a, cre);
            ni = add_dd(b, cim);
        }
        double dist = nr.hi * nr.hi + ni.hi * ni.hi;
        if (dist > squared) {
            *re = nr;
            *im = ni;
            return i;
        }
        zr = nr;
        zi = ni;
    }
    *re = zr;
    *im = zi;
    return cfg->iterations;
}

static int escape_algo(const ddm_config *cfg) { return cfg->algo == 0 || cfg->algo == 2; }

/* rows [y0, y1): z4[4k .. 4k+3] = re.hi, re.lo, im.hi, im.lo; iters[k]; k = (y - y0) * width + x */
void ddm_escape_rows(const ddm_config *cfg, double lo_re, double lo_im, uint32_t y0, uint32_t y1, double *z4,
                     uint32_t *iters, int threads) {
    const int64_t rows = (int64_t)y1 - (int64_t)y0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int64_t r = 0; r < rows; r++) {
        for (uint32_t x = 0; x < cfg->width; x++) {
            const uint64_t k = (uint64_t)r * cfg->width + x;
            ddv re = {0.0, 0.0}, im = {0.0, 0.0};
            uint32_t it = 0;
            if (escape_algo(cfg)) {
                start_of(cfg, lo_re, lo_im, x, (uint64_t)y0 + (uint64_t)r, &re, &im);
                it = orbit(cfg, &re, &im);
            }
            z4[4 * k] = re.hi;
            z4[4 * k + 1] = re.lo;
            z4[4 * k + 2] = im.hi;
            z4[4 * k + 3] = im.lo;
            iters[k] = it;
        }
    }
}

/* one pixel at any (x, y), inside the image or not (get_recursive_pixel does not clamp x, y to the image, and off_re
 * depends on the width, so no row range stands in for it): z4 = re.hi, re.lo, im.hi, im.lo; returns the escape index */
uint32_t ddm_pixel(const ddm_config *cfg, double lo_re, double lo_im, uint32_t x, uint32_t y, double z4[4]) {
    ddv re = {0.0, 0.0}, im = {0.0, 0.0};
    uint32_t it = 0;
    if (escape_algo(cfg)) {
        start_of(cfg, lo_re, lo_im, x, y, &re, &im);
        it = orbit(cfg, &re, &im);
    }
    z4[0] = re.hi;
    z4[1] = re.lo;
    z4[2] = im.hi;
    z4[3] = im.lo;
    return it;
}

/* the start coordinates alone (iterations = 0 gives the same through ddm_escape_rows) */
void ddm_start(const ddm_config *cfg, double lo_re, double lo_im, uint32_t x, uint32_t y, double out4[4]) {
    ddv re, im;
    start_of(cfg, lo_re, lo_im, x, y, &re, &im);
    out4[0] = re.hi;
    out4[1] = re.lo;
    out4[2] = im.hi;
    out4[3] = im.lo;
}

/* executed iterations over rows [y0, y1): escape at index i -> i + 1, exhaustion -> iterations */
uint64_t ddm_count_iterations(const ddm_config *cfg, uint32_t y0, uint32_t y1, int threads) {
    uint64_t total = 0;
    if (!escape_algo(cfg)) return 0;
    const int64_t rows = (int64_t)y1 - (int64_t)y0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(+ : total)
    for (int64_t r = 0; r < rows; r++) {
        for (uint32_t x = 0; x < cfg->width; x++) {
            ddv re, im;
            start_of(cfg, 0.0, 0.0, x, (uint64_t)y0 + (uint64_t)r, &re, &im);
            const uint32_t it = orbit(cfg, &re, &im);
            total += it < cfg->iterations ? (uint64_t)it + 1 : cfg->iterations;
        }
    }
    return total;
}
