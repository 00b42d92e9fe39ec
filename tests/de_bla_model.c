/*
 * de_bla_model.c — host restatement of DE ON BLA-PT (include/fractal_hip.h, "DE ON BLA-PT"), written from the definition
 * alone: BLA-PT's pixel loop (tests/bla_model.c restates it; the lines are repeated here so that z, iters and the passes can
 * be compared with that model bit for bit) with the derivative d carried beside it.  The checker escape_bla_de_kernel
 * (fractal-renderer_amd/csrc/fr_de_bla.hip) is compared with bit for bit.
 *
 * Nothing is built here: the orbits are PASSED IN (tests/pt_model.py gives a dd centre's, tests/pt_wide_model.py a wide
 * centre's) and so are their tables, as tests/bla_model.c's blam_build_table lays them out — 5 doubles per entry (A.re, A.im,
 * B.re, B.im, r2), level after level from level 0.
 *
 * Compiled by tests/de_bla_model.py at run time: gcc -O2 -ffp-contract=off -fno-fast-math -shared (no fused multiply-add but
 * the explicit fma() calls), into a temporary directory.
 */
#include <math.h>
#include <stdint.h>

typedef struct {
    uint32_t width, height, iterations;
    int julia;
    double limit, scale_re, scale_im;
} debm_view;

typedef struct {
    double are, aim, bre, bim, r2;
} debm_entry;

/* one followed orbit with its table: level k has n[k] entries from e[off[k]]; levels == 0: the table is empty */
typedef struct {
    const double *x;
    uint32_t last;
    uint32_t levels;
    uint32_t n[33];
    uint64_t off[33];
    const debm_entry *e;
} debm_orbit;

static void orbit_init(debm_orbit *o, const double *x, uint32_t last, const double *table, const uint32_t *n, uint32_t levels) {
    o->x = x;
    o->last = last;
    o->levels = levels;
    o->e = (const debm_entry *)table;
    uint64_t off = 0;
    for (uint32_t k = 0; k < levels; k++) {
        o->n[k] = n[k];
        o->off[k] = off;
        off += n[k];
    }
}

/* out: z.re, z.im, d.re, d.im */
static uint32_t pixel(const debm_view *v, const debm_orbit *ox, const debm_orbit *ok, uint64_t x, uint64_t y, double out[4],
                      uint32_t *passes, uint32_t *skips) {
    const double w = (double)v->width, h = (double)v->height;
    const double ore = (((double)x / h) - ((w / h) / 2.0)) / v->scale_re;
    const double oim = (((double)y / h) - 0.5) / v->scale_im;
    const double squared = v->limit * v->limit;
    const double b0 = v->julia ? 0.0 : 1.0;
    const uint32_t iterations = v->iterations;
    const debm_orbit *o = ox;
    uint32_t m = v->julia ? 0u : 1u;
    double dzr = ore, dzi = oim;
    const double dcr = v->julia ? 0.0 : ore, dci = v->julia ? 0.0 : oim;
    double zr = o->x[2 * m] + dzr, zi = o->x[2 * m + 1] + dzi;
    double dr = 1.0, di = 0.0; /* d0 = (1, 0) */
    uint32_t i = 0, np = 0, ns = 0, result = iterations;
    while (i < iterations) {
        np++;
        /* 1. the level: BLA-PT's four conditions */
        const double d2 = dzr * dzr + dzi * dzi;
        uint32_t K = 0;
        if (m >= 1) {
            const uint32_t j = m - 1;
            for (uint32_t k = 1; k < o->levels; k++) {
                if (j % (1u << k) != 0) break;
                if ((j >> k) >= o->n[k]) break;
                if ((uint64_t)i + (1u << k) > iterations) break;
                if (!(d2 < o->e[o->off[k] + (j >> k)].r2)) break;
                K = k;
            }
        }
        /* 2. the step, and the derivative's beside it */
        double ndr, ndi, ner, nei;
        if (K == 0) {
            const double tr = o->x[2 * m] + zr, ti = o->x[2 * m + 1] + zi;
            ndr = fma(tr, dzr, fma(-ti, dzi, dcr));
            ndi = fma(tr, dzi, fma(ti, dzr, dci));
            const double ur = zr + zr, ui = zi + zi; /* DE's step, from the z before the step */
            ner = fma(ur, dr, fma(-ui, di, b0));
            nei = fma(ur, di, ui * dr);
            m += 1;
            i += 1;
        } else {
            const debm_entry *e = &o->e[o->off[K] + ((m - 1) >> K)];
            ndr = fma(e->are, dzr, fma(-e->aim, dzi, fma(e->bre, dcr, -(e->bim * dci))));
            ndi = fma(e->are, dzi, fma(e->aim, dzr, fma(e->bre, dci, e->bim * dcr)));
            const double br = v->julia ? 0.0 : e->bre, bi = v->julia ? 0.0 : e->bim; /* Julia: b = (+0, +0) */
            ner = fma(e->are, dr, fma(-e->aim, di, br));
            nei = fma(e->are, di, fma(e->aim, dr, bi));
            m += 1u << K;
            i += 1u << K;
            ns++;
        }
        zr = o->x[2 * m] + ndr;
        zi = o->x[2 * m + 1] + ndi;
        dzr = ndr;
        dzi = ndi;
        dr = ner; /* escape returns nd; otherwise d = nd */
        di = nei;
        /* 3. the tests, BLA-PT's */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) {
            result = i - 1;
            break;
        }
        if (dist < dzr * dzr + dzi * dzi || m == o->last) { /* a rebase never touches d */
            dzr = zr;
            dzi = zi;
            m = 0;
            o = ok;
        }
    }
    out[0] = zr, out[1] = zi, out[2] = dr, out[3] = di;
    *passes = np;
    *skips = ns;
    return result;
}

/* rows [y0, y1): z[2p], z[2p+1]; iters[p]; der[2p], der[2p+1]; passes[p] = passes through the loop and skips[p] = those that
 * skipped; p = (y - y0) * width + x.  escape == 0 (an algorithm without orbits): zeros in all of them.
 * x: the orbit a pixel starts on (R or V), k: the one it rebases onto (R again, or K), each with its table. */
void debm_rows(const debm_view *v, int escape, const double *x, uint32_t x_last, const double *x_table, const uint32_t *x_n,
               uint32_t x_levels, const double *k, uint32_t k_last, const double *k_table, const uint32_t *k_n, uint32_t k_levels,
               uint32_t y0, uint32_t y1, double *z, uint32_t *iters, double *der, uint32_t *passes, uint32_t *skips) {
    debm_orbit ox, ok;
    if (escape) {
        orbit_init(&ox, x, x_last, x_table, x_n, x_levels);
        orbit_init(&ok, k, k_last, k_table, k_n, k_levels);
    }
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t xx = 0; xx < v->width; xx++) {
            const uint64_t p = (uint64_t)(y - y0) * v->width + xx;
            double o[4] = {0.0, 0.0, 0.0, 0.0};
            passes[p] = skips[p] = 0;
            iters[p] = escape ? pixel(v, &ox, &ok, xx, y, o, &passes[p], &skips[p]) : 0u;
            z[2 * p] = o[0], z[2 * p + 1] = o[1], der[2 * p] = o[2], der[2 * p + 1] = o[3];
        }
}
