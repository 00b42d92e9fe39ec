/*
 * fr_de_bla.hip — DE ON BLA-PT (include/fractal_hip.h, "DE ON BLA-PT"): BLA-PT's pixel loop (fr_bla.hip: orbit_bla) with the
 * orbit's derivative d carried beside it, through the plain steps as DE carries it (fr_de.hip) and through the table's skips:
 * a skip over 2^K steps is d' = A d + B with the entry's own coefficients, since the table's merge A = Ay Ax, B = Ay Bx + By is
 * the recurrence of d' = 2 X d + b0 over the block.  tests/de_bla_model.c restates the definition; tests/test_gpu_de_bla.py
 * compares the two bit for bit.
 *
 * Nothing is added to the table and none is rebuilt: orbits and tables are the context's (fr_bla.h: bla_table_for), so a BLA-PT
 * call and a DE call of the same view and bits share one table.
 *
 * escape_bla_de_kernel<JULIA>: escape_bla_kernel's escape mode — a workgroup of 4 waves renders 16 x 16 pixels, each wave one
 * 8 x 8 tile, `off` staged in LDS, the level search by bisection over r2, 64-bit output offsets — writing z, iters and der.
 * One pass:
 *   - the search, the load of (A, B) behind the branch and the step of dz are orbit_bla's, operation for operation: the
 *     derivative only reads, so z and iters are fr_escape_rows_pt_bla's bit for bit;
 *   - ONE arithmetic path for the derivative of both kinds of lanes: nd = (fma(g.re, d.re, fma(-g.im, d.im, b.re)),
 *     fma(g.re, d.im, fma(g.im, d.re, b.im))), where a lane that skips takes g = A and b = B (Julia: b = (+0, +0), its table
 *     stores no B) and a lane that steps takes g = z + z and b = (b0, -0).  fma(x, y, -0) is x * y in every bit — the sum of a
 *     product and -0 is the product, and -0 + -0 = -0 keeps a zero product's sign — so the plain lane's imaginary part is the
 *     definition's fma(t.re, d.im, t.im * d.re), and on a view where no pass skips all three arrays are fr_escape_rows_de's (PT).
 * The registers, the occupancy and the inner loop: profiles/de_bla_inner_loop_isa.txt.
 *
 * ss_refine_de_bla_kernel<JULIA>: ADAPTIVE SUPERSAMPLED DE's refine pass on this road (fr_ss_adaptive_de.hip; fr_ss_list.h: the
 * claim loop) — orbit_bla_de on the s x s samples of the listed edge pixels, each coloured and shaded through fr_ss_de_sample.h.
 *
 * The host half, at the end of the file, is the three things fr_de.h asks of a road — bla_de_domain (BLA-PT's domain check,
 * fr_bla.h: bla_check, then DE's limit), bla_de_launch (the kernel on given parameters, on the context's orbits and tables) and
 * bla_de_ss_refine — and the two calls, each the domain and fr_de.h's device or host form of a three-array row call.
 */
#include <cmath>
#include <memory>

#include "fr_bla.h"
#include "fr_ctx.h"
#include "fr_de.h"
#include "fr_math.h"
#include "fr_ss_list.h"
#include "fr_wide.h"

namespace {

#include "fr_colour.h"
#include "fr_de_shade.h"
#include "fr_ss_de_sample.h" /* ss_de_sample_colour */

/* the orbits and their tables as the kernel sees them (fr_bla.hip's BlaDev); Mandelbrot: the k fields repeat the x fields */
struct DeBlaDev {
    const double2 *x_orbit, *k_orbit;
    const double *x_r2, *k_r2;     /* r2 of the levels >= 1 */
    const double *x_coef, *k_coef; /* Mandelbrot: A.re, A.im, B.re, B.im per entry; Julia: A.re, A.im */
    uint32_t x_last, k_last;
    uint32_t x_n0, k_n0; /* entries of level 0: last - 1, or 0 for an empty table */
};

/* The pixel loop of "DE ON BLA-PT": orbit_bla (fr_bla.hip) with d = (er, ei) beside it.  Returns the escape index (or
 * `iterations`), the final z in (out_re, out_im) and the derivative in (out_dr, out_di): the returned step's on escape, the
 * last one's on exhaustion, (1, 0) for a cap of 0. */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_bla_de(uint32_t iterations, double off_re, double off_im, const DeBlaDev &t, double squared,
                                                 double &out_re, double &out_im, double &out_dr, double &out_di) {
    const double2 *X = t.x_orbit;
    const double *R2 = t.x_r2, *CF = t.x_coef;
    uint32_t last = t.x_last, n0 = t.x_n0;
    uint32_t m = JULIA ? 0u : 1u;
    double dzr = off_re, dzi = off_im;
    const double dcr = JULIA ? 0.0 : off_re, dci = JULIA ? 0.0 : off_im;
    const double b0 = JULIA ? 0.0 : 1.0;
    double2 Z = X[m]; /* X_m of the orbit followed */
    double zr = Z.x + dzr, zi = Z.y + dzi;
    double er = 1.0, ei = 0.0; /* d0 = (1, 0) */
    uint32_t i = 0, result = iterations;
    while (i < iterations) {
        /* 1. the level: the largest k in 1 .. kc whose radius holds dz (orbit_bla's search) */
        const double d2 = dzr * dzr + dzi * dzi;
        const uint32_t j = m - 1u;
        uint32_t K = 0;
        if (m >= 1u && j < n0) {
            uint32_t kc = j ? (uint32_t)__builtin_ctz(j) : 31u;          /* j % 2^k == 0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(n0 - j));         /* (j >> k) < n_k, that is j + 2^k <= n0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(iterations - i)); /* i + 2^k <= iterations */
            uint32_t lo = 0, hi = kc;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                if (d2 < R2[bla_level_offset(n0, mid) + (j >> mid)])
                    lo = mid;
                else
                    hi = mid - 1u;
            }
            K = lo;
        }
        /* 2. the step dz' = A dz + c and the derivative's d' = g d + b */
        double ar, ai, cr = dcr, ci = dci;
        double gr, gi, br = b0, bi = -0.0; /* a plain step: fma(g.im, d.re, -0) is g.im * d.re, the definition's product */
        uint32_t step = 1u;
        if (K) {
            const uint32_t e = bla_level_offset(n0, K) + (j >> K);
            if (JULIA) { /* B dc is +0 = dc for every finite B; the derivative's b is (+0, +0) by definition */
                const double2 A = reinterpret_cast<const double2 *>(CF)[e];
                ar = A.x, ai = A.y;
                br = 0.0, bi = 0.0;
            } else {
                const double4 AB = reinterpret_cast<const double4 *>(CF)[e];
                ar = AB.x, ai = AB.y;
                cr = __builtin_fma(AB.z, dcr, -(AB.w * dci));
                ci = __builtin_fma(AB.z, dci, AB.w * dcr);
                br = AB.z, bi = AB.w;
            }
            gr = ar, gi = ai;
            step = 1u << K;
        } else {
            ar = Z.x + zr, ai = Z.y + zi; /* t = X_m + z */
            gr = zr + zr, gi = zi + zi;   /* the derivative's t: from the z before the step */
        }
        const double ndr = __builtin_fma(ar, dzr, __builtin_fma(-ai, dzi, cr));
        const double ndi = __builtin_fma(ar, dzi, __builtin_fma(ai, dzr, ci));
        const double ner = __builtin_fma(gr, er, __builtin_fma(-gi, ei, br));
        const double nei = __builtin_fma(gr, ei, __builtin_fma(gi, er, bi));
        m += step;
        i += step;
        const double2 N = X[min(m, last)]; /* m <= last: 1 + ((j >> K) + 1) 2^K <= 1 + n0 */
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
        er = ner; /* escape returns nd; otherwise d = nd */
        ei = nei;
        /* 3. the tests, PT's; a rebase never touches d */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) { /* this lane leaves EXEC; the wave goes on while any lane is left */
            result = i - 1u;
            break;
        }
        if (dist < dzr * dzr + dzi * dzi || m == last) {
            dzr = zr;
            dzi = zi;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                R2 = t.k_r2;
                CF = t.k_coef;
                last = t.k_last;
                n0 = t.k_n0;
            }
            Z = make_double2(0.0, 0.0); /* K_0 = R_0 = 0 */
        } else {
            Z = N;
        }
    }
    out_re = zr;
    out_im = zi;
    out_dr = er;
    out_di = ei;
    return result;
}

template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_bla_de_kernel(const fr_kparams p, double *__restrict__ z,
                                                                        uint32_t *__restrict__ iters, double *__restrict__ der,
                                                                        const DeBlaDev t) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;

    if (tid < kDeepBlockW + kDeepBlockH) {
        /* off: coord_to_space (calc/src/lib.rs:181-197) without the final `+ pos`, PT's off */
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kDeepBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            s_re[tid] = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        } else {
            const uint32_t r = row0 + (tid - kDeepBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            s_im[tid - kDeepBlockW] = (((double)y / height) - 0.5) / p.scale_im;
        }
    }
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    if (!(cx < p.ncols && r < p.nrows)) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    double zr = 0.0, zi = 0.0, dr = 0.0, di = 0.0; /* an algorithm without orbits writes zeros */
    uint32_t it = 0;
    if (escape_algo) {
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        it = orbit_bla_de<JULIA>(p.iterations, s_re[lx], s_im[ly], t, squared, zr, zi, dr, di);
    }
    const uint64_t k = (uint64_t)r * p.ncols + cx;
    z[2 * k] = zr;
    z[2 * k + 1] = zi;
    iters[k] = it;
    der[2 * k] = dr;
    der[2 * k + 1] = di;
}

/* ADAPTIVE SUPERSAMPLED DE's refine pass (include/fractal_hip.h; fr_ss_list.h: the claim loop; fr_de.hip: ss_refine_de_pt_kernel)
 * with orbit_bla_de: `off` by escape_bla_de_kernel's formula on cfg_s (`p`), the table `t` built with D over the whole image of
 * cfg_s */
template <bool JULIA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_de_bla_kernel(const fr_kparams p, const fr_ss_refine a, const fr_ss_de_shade sh,
                                                                            const DeBlaDev t) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kSsRefineThreads) s_tab[k] = gt[k];
    const uint16_t *const s_lt = ss_refine_tables<LINEAR>(); /* LINEAR-LIGHT SUPERSAMPLING: staged with the log2 table */
    __syncthreads();
    const double width = (double)p.width, height = (double)p.height;
    const double squared = p.limit * p.limit;
    ss_refine_loop<LINEAR>(a, s_lt, [&](uint64_t x, uint64_t y) {
        const double off_re = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        const double off_im = (((double)y / height) - 0.5) / p.scale_im;
        double zr, zi, dr, di;
        const uint32_t it = orbit_bla_de<JULIA>(p.iterations, off_re, off_im, t, squared, zr, zi, dr, di);
        return ss_de_sample_colour(p, zr, zi, dr, di, it, sh.pixels, sh.thickness, s_tab);
    });
}

}  // namespace

using namespace fr;

namespace {

/* the orbits and the table of an escape-time view as the kernels take them, from the context's caches */
int de_bla_dev_fill(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, std::shared_ptr<PtOrbit> &orbit,
                    std::shared_ptr<BlaTable> &table, DeBlaDev &t) {
    PtOrbitView v;
    const int rc = bla_table_for(ctx, cfg, c, bits, false, orbit, v, table);
    if (rc != FR_OK) return rc;
    const BlaTableDev &d = table->view;
    t = DeBlaDev{};
    t.x_r2 = d.x_rad, t.k_r2 = d.k_rad;
    t.x_coef = d.x_coef, t.k_coef = d.k_coef;
    t.x_n0 = d.x_n0, t.k_n0 = d.k_n0;
    t.x_orbit = v.x;
    t.k_orbit = v.k;
    t.x_last = v.x_last;
    t.k_last = v.k_last;
    return FR_OK;
}

}  // namespace

/* fr_de.h: the road's domain and its launch; fr_ss_list.h: its refine launch */
namespace fr {

/* BLA-PT's domain (bits resolved in place), then DE's limit */
int bla_de_domain(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1) {
    const int rc = bla_check(cfg, c, bits, y0, y1);
    return rc != FR_OK ? rc : check_de_limit(cfg);
}

/* on the context's orbits and tables */
int bla_de_launch(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_kparams &p, double *d_z, uint32_t *d_iters,
                  double *d_der, hipStream_t stream, const char *&kname) {
    kname = "escape_bla_de_kernel";
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    dim3 grid, block;
    HIP_TRY(fr_deep_grid(p, grid, block));
    const bool julia = cfg->algo == FR_ALGO_JULIA;
    if (cfg->algo != FR_ALGO_MANDELBROT && !julia) { /* no escape-time algorithm: zeros, and no orbit is asked for */
        escape_bla_de_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, DeBlaDev{});
        HIP_TRY(hipGetLastError());
        return FR_OK;
    }
    std::shared_ptr<PtOrbit> orbit; /* alive until the launch is enqueued, like the table */
    std::shared_ptr<BlaTable> table;
    DeBlaDev t;
    const int rc = de_bla_dev_fill(ctx, cfg, c, bits, orbit, table, t);
    if (rc != FR_OK) return rc;
    if (julia)
        escape_bla_de_kernel<true><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, t);
    else
        escape_bla_de_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, t);
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

int bla_de_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, const fr_ss_de_shade &sh,
                     uint32_t groups, hipStream_t stream) {
    std::shared_ptr<PtOrbit> orbit; /* alive until the launch is enqueued, like the table */
    std::shared_ptr<BlaTable> table;
    DeBlaDev t;
    const int rc = de_bla_dev_fill(ctx, cfg, c, bits, orbit, table, t);
    if (rc != FR_OK) return rc;
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    ss_refine_instance(cfg->algo == FR_ALGO_JULIA, a.linear, [&](auto J, auto L) {
        ss_refine_de_bla_kernel<J(), L()><<<dim3(groups), dim3(kSsRefineThreads), 0, stream>>>(p, a, sh, t);
    });
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

}  // namespace fr

extern "C" {

int fr_escape_rows_de_pt_bla_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                                    uint32_t y1, void *d_z, void *d_iters, void *d_der, void *hip_stream) {
    const Centre c{pos_lo, centre};
    const int rc = bla_de_domain(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_device(cfg, y0, y1, d_z, d_iters, d_der, hip_stream, de_rows(cfg, y0, y1, de_road(bla_de_launch, cfg, c, bits)));
}

int fr_escape_rows_de_pt_bla(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                             uint32_t y1, double *z, uint32_t *iters, double *der) {
    const Centre c{pos_lo, centre};
    const int rc = bla_de_domain(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_host(cfg, y0, y1, z, iters, der, de_rows(cfg, y0, y1, de_road(bla_de_launch, cfg, c, bits)));
}

} /* extern "C" */
