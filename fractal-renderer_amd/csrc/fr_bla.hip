/*
 * fr_bla.hip — BLA-PT: perturbation with bilinear-approximation skips (include/fractal_hip.h, fr_precision: "BLA-PT";
 * tests/bla_model.c restates it; tests/test_gpu_bla.py compares the two bit for bit).  While a pixel's offset dz from the
 * reference orbit is far below the orbit itself, the PT step dz' = (2X + dz) dz + dc is linear in (dz, dc) to below f64
 * rounding, and 2^k composed steps are one tabulated dz' = A dz + B dc.
 *
 * Host part: the table of an orbit, built from its stored f64 entries alone (the orbit comes from fr_pt.hip's cache, dd or
 * wide), with -ffp-contract=off and std::fma exactly where the definition has fma; uploaded once and kept per context
 * (Ctx::bla_table, under Ctx::pt_mu), keyed by the orbit's identity, D, S and bits.  SCALED PT's table (fr_scaled.hip) is the
 * same build with eps S for eps, Dw for D and the scaled radius R stored where BLA-PT stores r2; it shares the slot, with its
 * kind in the key (fr_bla.h).  S = 2^e is a key field of its own (BLA-PT: 1): two views whose scales differ by a power of two
 * share the orbit, (sre, sim) and with them Dw bit for bit, and every R of one is 2^k times the other's.
 *
 * Device layout of one orbit's table: the levels k >= 1 one after another (level 0 only builds the levels above it and never
 * leaves the host); level k starts at entry bla_level_offset(n0, k), a closed form, so the kernel needs no offset array.  r2
 * lives in an array of its own (8 B per entry: the level search reads nothing else), the coefficients in another: A and B
 * for Mandelbrot (32 B), A alone for Julia (16 B: dc = 0 there, and B dc is exactly +0).  n0 - popcount(n0) entries in all,
 * so at most 40 B (Mandelbrot) or 24 B (Julia, per orbit, two orbits) per orbit entry.
 *
 * Device part, escape_bla_kernel<MODE, JULIA>: PT's shape (cdna_hip_programming: one lane per pixel, LDS for what a
 * workgroup shares) — a workgroup of 4 waves renders 16 x 16 pixels, each wave one 8 x 8 tile, `off` and the log2 table
 * staged in LDS, 64-bit output offsets, plain vector loads and stores.  One pass of the loop:
 *   - the level search: conditions 1 to 3 of the definition are arithmetic (count of trailing zeros of j, the entries left
 *     in the orbit, the iterations left under the cap) and give a cap kc; condition 4 is monotone, so the largest level is
 *     found by bisection over 1 .. kc, one 8-byte gather of r2 per probe.  kc is above 2 or 3 only where j has many trailing
 *     zeros: at j = 0 (the start, and one step after every rebase), which is where the long skips are;
 *   - ONE arithmetic path for both kinds of lanes: a lane that skips loads (A, B) and forms c = B dc; a lane that steps takes
 *     A = X_m + z and c = dc; then dz' = fma(A.re, dz.re, fma(-A.im, dz.im, c.re)) etc. is the definition's sequence for
 *     either, bit for bit (the plain step IS that expression with A = t and c = dc).  Only the loads sit behind the branch;
 *   - one 16-byte gather of X at the new m, which is also the next plain step's X_m.  After the first skip the lanes of a
 *     wave no longer share m, so PT's one-step-ahead load of X_{m+2} has nothing to aim at and is not carried over: the
 *     latency is covered by the other waves of the CU (the kernel runs at 8 waves per SIMD).
 *
 * ADAPTIVE SUPERSAMPLING (include/fractal_hip.h; fr_ss_adaptive.hip): ss_refine_bla_kernel<JULIA>, persistent waves that run
 * orbit_bla on the s x s samples of the listed edge pixels (fr_ss_list.h: the claim loop); bla_render_map, the RGB launch over
 * the probe's strided map, and bla_ss_refine, the refine launch.
 *
 * The calls, at the end of the file: each builds its Centre, runs check_bla and hands bla_rows — the profiled launch of its
 * rows — to the row-call body of its form in fr_ctx.h (rgb_rows_device, rgb_rows_host, raw_rows_device, raw_rows_host,
 * count_rows).  The workgroup's geometry and the launch's grid are the deep kernels' (fr_kernels.h: kDeep*, fr_deep_grid).
 */
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fr_bla.h"
#include "fr_ctx.h"
#include "fr_math.h"
#include "fr_ss_list.h"
#include "fr_wide.h"

namespace {

#include "fr_colour.h"

/* the orbits and their tables as the kernel sees them; Mandelbrot: the k fields repeat the x fields */
struct BlaDev {
    const double2 *x_orbit, *k_orbit;
    const double *x_r2, *k_r2;     /* r2 of the levels >= 1 */
    const double *x_coef, *k_coef; /* Mandelbrot: A.re, A.im, B.re, B.im per entry; Julia: A.re, A.im */
    uint32_t x_last, k_last;
    uint32_t x_n0, k_n0; /* entries of level 0: last - 1, or 0 for an empty table */
};

/* ---- device: the pixel loop (include/fractal_hip.h, "BLA-PT"), operation for operation ----------------------------- */

/* Returns the escape index (or `iterations`), the final z in (out_re, out_im), the passes through the loop in `passes`. */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_bla(uint32_t iterations, double off_re, double off_im, const BlaDev &t, double squared,
                                              double &out_re, double &out_im, uint32_t &passes) {
    const double2 *X = t.x_orbit;
    const double *R2 = t.x_r2, *CF = t.x_coef;
    uint32_t last = t.x_last, n0 = t.x_n0;
    uint32_t m = JULIA ? 0u : 1u;
    double dzr = off_re, dzi = off_im;
    const double dcr = JULIA ? 0.0 : off_re, dci = JULIA ? 0.0 : off_im;
    double2 Z = X[m]; /* X_m of the orbit followed */
    double zr = Z.x + dzr, zi = Z.y + dzi;
    uint32_t i = 0, np = 0, result = iterations;
    while (i < iterations) {
        np++;
        /* 1. the level: the largest k in 1 .. kc whose radius holds dz (r2 is non-increasing in k for a fixed first step) */
        const double d2 = dzr * dzr + dzi * dzi;
        const uint32_t j = m - 1u;
        uint32_t K = 0;
        if (m >= 1u && j < n0) {
            uint32_t kc = j ? (uint32_t)__builtin_ctz(j) : 31u;      /* j % 2^k == 0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(n0 - j));     /* (j >> k) < n_k, that is j + 2^k <= n0 */
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
        /* 2. the step: A and the constant term c of dz' = A dz + c */
        double ar, ai, cr = dcr, ci = dci;
        uint32_t step = 1u;
        if (K) {
            const uint32_t e = bla_level_offset(n0, K) + (j >> K);
            if (JULIA) { /* B dc: fma(B.re, 0, -(B.im * 0)) and fma(B.re, 0, B.im * 0) are +0 = dc for every finite B */
                const double2 A = reinterpret_cast<const double2 *>(CF)[e];
                ar = A.x, ai = A.y;
            } else {
                const double4 AB = reinterpret_cast<const double4 *>(CF)[e];
                ar = AB.x, ai = AB.y;
                cr = __builtin_fma(AB.z, dcr, -(AB.w * dci));
                ci = __builtin_fma(AB.z, dci, AB.w * dcr);
            }
            step = 1u << K;
        } else {
            ar = Z.x + zr, ai = Z.y + zi; /* t = X_m + z */
        }
        const double ndr = __builtin_fma(ar, dzr, __builtin_fma(-ai, dzi, cr));
        const double ndi = __builtin_fma(ar, dzi, __builtin_fma(ai, dzr, ci));
        m += step;
        i += step;
        const double2 N = X[min(m, last)]; /* m <= last: 1 + ((j >> K) + 1) 2^K <= 1 + n0 */
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
        /* 3. the tests, PT's */
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
    passes = np;
    return result;
}

template <int MODE, bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_bla_kernel(const fr_kparams p, const fr_kout out, const BlaDev t) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;

    if (MODE == FR_OUT_RGB) {
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += 64 * kDeepWaves) s_tab[k] = gt[k];
    }
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
    const bool valid = cx < p.ncols && r < p.nrows;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    double zr = 0.0, zi = 0.0;
    uint32_t iters = 0, passes = 0;
    if (valid && escape_algo) {
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        iters = orbit_bla<JULIA>(p.iterations, s_re[lx], s_im[ly], t, squared, zr, zi, passes);
    }

    if constexpr (MODE == FR_OUT_RGB) {
        if (valid) {
            uint8_t rgb[3] = {0, 0, 0};
            if (escape_algo) {
                const ColourConsts cc = make_colour_consts(p);
                const double r2 = zr * zr, i2 = zi * zi;
                colour_pixel<double>(cc, zr, zi, r2, i2, iters, s_tab, nullptr, rgb); /* :214-234 on the f64 z */
            }
            const uint64_t k = (uint64_t)r * p.ncols + cx;
            if (p.out_rgba) {
                reinterpret_cast<uint32_t *>(out.rgb)[k] =
                    (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16) | 0xFF000000u;
            } else {
                uint8_t *o = out.rgb + 3ull * k;
                o[0] = rgb[0];
                o[1] = rgb[1];
                o[2] = rgb[2];
            }
        }
    } else if constexpr (MODE == FR_OUT_ESCAPE) {
        if (valid) {
            const uint64_t k = (uint64_t)r * p.ncols + cx;
            if (out.z) {
                out.z[2 * k] = zr;
                out.z[2 * k + 1] = zi;
            }
            if (out.iters) out.iters[k] = iters;
        }
    } else { /* COUNT: the passes into count[0 .. SLOTS), the nominal iterations into count[SLOTS .. 2 SLOTS) */
        unsigned long long np = 0, n = 0;
        if (valid && escape_algo) {
            np = passes;
            n = iters < p.iterations ? (unsigned long long)iters + 1ull : p.iterations;
        }
        for (int off = 32; off > 0; off >>= 1) {
            np += __shfl_down(np, off, 64);
            n += __shfl_down(n, off, 64);
        }
        if (lane == 0 && n) {
            const uint32_t slot = (blockIdx.x + 131u * wave) % FR_COUNT_SLOTS;
            atomicAdd(out.count + slot, np);
            atomicAdd(out.count + FR_COUNT_SLOTS + slot, n);
        }
    }
}

template <bool JULIA>
hipError_t launch(const fr_kparams &p, int mode, const fr_kout &out, const BlaDev &t, hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    if (mode == FR_OUT_RGB)
        escape_bla_kernel<FR_OUT_RGB, JULIA><<<grid, block, 0, stream>>>(p, out, t);
    else if (mode == FR_OUT_ESCAPE)
        escape_bla_kernel<FR_OUT_ESCAPE, JULIA><<<grid, block, 0, stream>>>(p, out, t);
    else
        escape_bla_kernel<FR_OUT_COUNT, JULIA><<<grid, block, 0, stream>>>(p, out, t);
    return hipGetLastError();
}

/* ---- device: ADAPTIVE SUPERSAMPLING's refine pass (include/fractal_hip.h; fr_ss_list.h: the claim loop) ---------------- */

/* ss_refine_pt_kernel (fr_pt.hip) with orbit_bla: `off` by escape_bla_kernel's formula on cfg_s (`p`), the table `t` built with
 * D over the whole image of cfg_s */
template <bool JULIA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_bla_kernel(const fr_kparams p, const fr_ss_refine a, const BlaDev t) {
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
        double zr, zi;
        uint32_t passes;
        const uint32_t iters = orbit_bla<JULIA>(p.iterations, off_re, off_im, t, squared, zr, zi, passes);
        uint8_t rgb[3] = {0, 0, 0};
        const ColourConsts cc = make_colour_consts(p);
        colour_pixel<double>(cc, zr, zi, zr * zr, zi * zi, iters, s_tab, nullptr, rgb);
        return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
    });
}

/* ---- host: the table of one orbit (include/fractal_hip.h, "BLA-PT": table) ------------------------------------------ */

/* levels >= 1 in the device layout; level 0 is a function of one orbit entry and is recomputed where it is asked for */
struct HostTable {
    uint32_t n0 = 0;          /* entries of level 0; 0: the table is empty */
    std::vector<double> coef; /* A.re, A.im, B.re, B.im per entry */
    std::vector<double> rad;  /* what an entry stores for the level search: r2, or SCALED PT's R */
    uint32_t levels() const { /* level 0 included */
        uint32_t k = 0;
        for (uint32_t n = n0; n; n >>= 1) k++;
        return k;
    }
    uint64_t entries() const { return n0 ? (uint64_t)n0 + (n0 - (uint32_t)__builtin_popcount(n0)) : 0; }
};

struct Entry {
    double are, aim, bre, bim, r;
};

Entry level0(const double *X, uint32_t j, double b0, double eps) {
    const uint32_t m = j + 1;
    Entry e;
    e.are = X[2 * m] + X[2 * m];
    e.aim = X[2 * m + 1] + X[2 * m + 1];
    e.bre = b0;
    e.bim = 0.0;
    e.r = eps * std::sqrt(e.are * e.are + e.aim * e.aim);
    return e;
}

Entry merge(const Entry &x, const Entry &y, double D) {
    Entry e;
    e.are = std::fma(y.are, x.are, -(y.aim * x.aim));
    e.aim = std::fma(y.are, x.aim, y.aim * x.are);
    e.bre = std::fma(y.are, x.bre, -(y.aim * x.bim)) + y.bre;
    e.bim = std::fma(y.are, x.bim, y.aim * x.bre) + y.bim;
    double q = (y.r - std::sqrt(x.bre * x.bre + x.bim * x.bim) * D) / std::sqrt(x.are * x.are + x.aim * x.aim);
    if (!(q > 0.0)) q = 0.0;
    e.r = x.r < q ? x.r : q;
    return e;
}

/* what an entry with radius r stores: BLA-PT r2 = r*r; SCALED PT (include/fractal_hip.h) R itself, or 0 below 2^-53 */
double stored_radius(double r, bool scaled) {
    if (!scaled) return r * r;
    return r < 0x1p-53 ? 0.0 : r;
}

/* X: re, im pairs of the entries 0 .. last.  BLA-PT: S = 1 and D of the image; SCALED PT: S = 2^e and Dw (eps S is exact) */
void build_table(const double *X, uint32_t last, double D, double b0, int bits, double S, bool scaled, HostTable &t) {
    t = HostTable();
    if (last < 2) return;
    const double eps = std::ldexp(1.0, -bits) * S;
    uint32_t n = last - 1;
    t.n0 = n;
    const size_t total = n - (uint32_t)__builtin_popcount(n);
    t.coef.resize(4 * total);
    t.rad.resize(total);
    std::vector<Entry> cur(n);
    for (uint32_t j = 0; j < n; j++) cur[j] = level0(X, j, b0, eps);
    size_t at = 0;
    while (n >= 2) {
        n /= 2;
        for (uint32_t j = 0; j < n; j++) { /* in place: slot j <= 2j has been consumed */
            const Entry e = merge(cur[2 * j], cur[2 * j + 1], D);
            cur[j] = e;
            double *c = &t.coef[4 * (at + j)];
            c[0] = e.are, c[1] = e.aim, c[2] = e.bre, c[3] = e.bim;
            t.rad[at + j] = stored_radius(e.r, scaled);
        }
        at += n;
    }
}

/* D of the definition: the bound of |dc| over the whole image */
double image_D(const fr_config *cfg) {
    const double width = (double)cfg->width, height = (double)cfg->height;
    const auto off_re = [&](uint64_t x) { return (((double)x / height) - ((width / height) / 2.0)) / cfg->scale.re; };
    const auto off_im = [&](uint64_t y) { return (((double)y / height) - 0.5) / cfg->scale.im; };
    const double a = std::fabs(off_re(0)), b = std::fabs(off_re(cfg->width ? cfg->width - 1u : 0u));
    const double c = std::fabs(off_im(0)), d = std::fabs(off_im(cfg->height ? cfg->height - 1u : 0u));
    const double mr = a > b ? a : b, mi = c > d ? c : d;
    return std::sqrt(mr * mr + mi * mi);
}

}  // namespace

namespace fr {

/* fr_bla.h: one slot per context for both kinds of table, keyed by the orbit, D (or Dw), S (1 for BLA-PT), bits and the kind:
 * everything build_table reads */
int bla_table_for(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, bool scaled, std::shared_ptr<PtOrbit> &orbit,
                  PtOrbitView &v, std::shared_ptr<BlaTable> &out) {
    const int rc = pt_orbit_view(ctx, cfg, c, orbit, v);
    if (rc != FR_OK) return rc;
    const bool julia = cfg->algo == 2;
    fr_config image = *cfg; /* Dw is D of the image with the scaled divisors (sre, sim) */
    double S = 1.0;
    if (scaled) {
        const ScaledConsts k = scaled_consts(cfg);
        image.scale.re = k.sre, image.scale.im = k.sim, S = k.S;
    }
    const double D = image_D(&image);
    std::lock_guard<std::mutex> lk(ctx.pt_mu);
    const std::shared_ptr<BlaTable> cached = ctx.bla_table;
    if (cached && cached->orbit.lock() == orbit && memcmp(&cached->D, &D, sizeof D) == 0 && memcmp(&cached->S, &S, sizeof S) == 0 &&
        cached->bits == bits && cached->scaled == scaled) {
        cached->built = false;
        out = cached;
        return FR_OK;
    }
    /* the stored entries come back from the device: the table is a function of them alone, and the cache keeps no host copy */
    const size_t x_n = (size_t)v.x_last + 1, k_n = julia ? (size_t)v.k_last + 1 : 0;
    std::vector<double> host(2 * (x_n + k_n));
    HIP_TRY(hipMemcpy(host.data(), v.x, x_n * sizeof(double2), hipMemcpyDeviceToHost));
    if (k_n) HIP_TRY(hipMemcpy(host.data() + 2 * x_n, v.k, k_n * sizeof(double2), hipMemcpyDeviceToHost));
    const double b0 = julia ? 0.0 : 1.0;
    HostTable tx, tk;
    build_table(host.data(), v.x_last, D, b0, bits, S, scaled, tx);
    if (julia) build_table(host.data() + 2 * x_n, v.k_last, D, b0, bits, S, scaled, tk);
    const size_t xe = tx.rad.size(), ke = tk.rad.size(), cw = julia ? 2 : 4; /* doubles per coefficient entry */
    std::vector<double> up(cw * (xe + ke) + xe + ke);
    const auto pack = [&](const HostTable &t, double *coef, double *rad) {
        for (size_t e = 0; e < t.rad.size(); e++)
            for (size_t w = 0; w < cw; w++) coef[cw * e + w] = t.coef[4 * e + w];
        if (!t.rad.empty()) memcpy(rad, t.rad.data(), t.rad.size() * sizeof(double));
    };
    double *h_xc = up.data(), *h_kc = h_xc + cw * xe, *h_xr = h_kc + cw * ke, *h_kr = h_xr + xe;
    pack(tx, h_xc, h_xr);
    pack(tk, h_kc, h_kr);
    auto t = std::make_shared<BlaTable>();
    t->orbit = orbit;
    t->D = D;
    t->S = S;
    t->bits = bits;
    t->scaled = scaled;
    t->x_levels = tx.levels();
    t->entries = (uint32_t)(tx.entries() + tk.entries());
    t->built = true;
    ctx.bla_table.reset(); /* the previous view's tables go first: their memory is free for these */
    if (!up.empty()) {
        HIP_TRY(hipMalloc(&t->dev, up.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(t->dev, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const double *d = static_cast<const double *>(t->dev);
    BlaTableDev &b = t->view;
    b.x_coef = d;
    b.k_coef = julia ? d + cw * xe : d;
    b.x_rad = d + cw * (xe + ke);
    b.k_rad = julia ? b.x_rad + xe : b.x_rad;
    b.x_n0 = tx.n0;
    b.k_n0 = julia ? tk.n0 : tx.n0;
    ctx.bla_table = t;
    out = std::move(t);
    return FR_OK;
}

namespace {

/* the view's orbits and tables from the context's caches as the kernels take them; the caller keeps `orbit` and `table` alive
 * until its launch has been enqueued */
int bla_dev_fill(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, std::shared_ptr<PtOrbit> &orbit, std::shared_ptr<BlaTable> &table,
                 BlaDev &t) {
    PtOrbitView v;
    const int rc = bla_table_for(ctx, cfg, c, bits, false, orbit, v, table);
    if (rc != FR_OK) return rc;
    const BlaTableDev &d = table->view;
    t = BlaDev{};
    t.x_r2 = d.x_rad, t.k_r2 = d.k_rad;
    t.x_coef = d.x_coef, t.k_coef = d.k_coef;
    t.x_n0 = d.x_n0, t.k_n0 = d.k_n0;
    t.x_orbit = v.x;
    t.k_orbit = v.k;
    t.x_last = v.x_last;
    t.k_last = v.k_last;
    return FR_OK;
}

int launch_bla(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_kparams &p, int mode, const fr_kout &out,
               hipStream_t stream) {
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    const bool julia = cfg->algo == 2;
    if (cfg->algo != 0 && !julia) { /* no escape-time algorithm: every pixel is black / zero, as PT's kernel gives */
        HIP_TRY(launch<false>(p, mode, out, BlaDev{}, stream));
        return FR_OK;
    }
    std::shared_ptr<PtOrbit> orbit;
    std::shared_ptr<BlaTable> table;
    BlaDev t;
    const int rc = bla_dev_fill(ctx, cfg, c, bits, orbit, table, t);
    if (rc != FR_OK) return rc;
    HIP_TRY(julia ? launch<true>(p, mode, out, t, stream) : launch<false>(p, mode, out, t, stream));
    return FR_OK;
}

/* ---- the calls ------------------------------------------------------------------------------------------------------ */

int check_bla(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1) {
    int rc = check_rows(cfg, y0, y1);
    if (rc != FR_OK) return rc;
    if (c.wide && c.pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "BLA-PT: pos_lo must be NULL when a wide centre is given");
    rc = c.check(cfg, FR_PRECISION_PT);
    if (rc != FR_OK) return rc;
    if (bits == 0) bits = FR_BLA_DEFAULT_BITS;
    if (bits < 24 || bits > 53) return fail(FR_ERR_INVALID_ARGUMENT, "BLA-PT: bits must be 0 (FR_BLA_DEFAULT_BITS) or 24 .. 53");
    return FR_OK;
}

/* The launch every row call below hands to its helper (fr_ctx.h): rows [y0, y1) in `mode` on `stream` between the profiling
 * events; the colour constants alone: no loop plan, no kernel choice, no view sample */
auto bla_rows(const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, unsigned channels, int mode) {
    return [=](Ctx &ctx, const fr_kout &out, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, channels, stream, [&](fr_kparams &p, const char *&kname) {
            kname = "escape_bla_kernel";
            return launch_bla(ctx, cfg, c, bits, p, mode, out, stream);
        });
    };
}

}  // namespace

/* the road's check and RGB row launch for the supersampled form (fr_ss.hip), which bands the rows itself */
int bla_check(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1) { return check_bla(cfg, c, bits, y0, y1); }
int bla_render_rows(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, unsigned channels,
                    const fr_kout &out, hipStream_t stream) {
    return bla_rows(cfg, c, bits, y0, y1, channels, FR_OUT_RGB)(ctx, out, stream);
}

/* fr_ss_list.h: ADAPTIVE SUPERSAMPLING on BLA-PT — the probe (the road's RGB kernel over the strided map) and the refine pass */
int bla_render_map(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_map &map, const fr_kout &out, hipStream_t stream) {
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    map.apply(p);
    return launch_bla(ctx, cfg, c, bits, p, FR_OUT_RGB, out, stream);
}

int bla_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, uint32_t groups, hipStream_t stream) {
    std::shared_ptr<PtOrbit> orbit;
    std::shared_ptr<BlaTable> table;
    BlaDev t;
    const int rc = bla_dev_fill(ctx, cfg, c, bits, orbit, table, t);
    if (rc != FR_OK) return rc;
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    ss_refine_instance(cfg->algo == 2, a.linear, [&](auto J, auto L) {
        ss_refine_bla_kernel<J(), L()><<<dim3(groups), dim3(kSsRefineThreads), 0, stream>>>(p, a, t);
    });
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

}  // namespace fr

using namespace fr;

int fr_render_rows_pt_bla_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                                 uint32_t y1, int channels, void *d_out, size_t out_len, void *hip_stream) {
    const Centre c{pos_lo, centre};
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = check_bla(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return rgb_rows_device(cfg, y0, y1, channels, d_out, out_len, hip_stream, bla_rows(cfg, c, bits, y0, y1, (unsigned)channels, FR_OUT_RGB));
}

int fr_render_rows_pt_bla(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                          uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    const Centre c{pos_lo, centre};
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = check_bla(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return rgb_rows_host(cfg, y0, y1, channels, out, out_len, bla_rows(cfg, c, bits, y0, y1, (unsigned)channels, FR_OUT_RGB));
}

int fr_escape_rows_pt_bla_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                                 uint32_t y1, void *d_z, void *d_iters, void *hip_stream) {
    const Centre c{pos_lo, centre};
    const int rc = check_bla(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return raw_rows_device(cfg, y0, y1, d_z, d_iters, hip_stream, bla_rows(cfg, c, bits, y0, y1, 0, FR_OUT_ESCAPE));
}

int fr_escape_rows_pt_bla(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                          uint32_t y1, double *z, uint32_t *iters) {
    const Centre c{pos_lo, centre};
    const int rc = check_bla(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return raw_rows_host(cfg, y0, y1, z, iters, 2, bla_rows(cfg, c, bits, y0, y1, 0, FR_OUT_ESCAPE));
}

int fr_debug_bla_count(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                       uint32_t y1, uint64_t *passes, uint64_t *steps) {
    const Centre c{pos_lo, centre};
    const int rc = check_bla(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    if (!passes || !steps) return fail(FR_ERR_INVALID_ARGUMENT, "passes or steps is NULL");
    *passes = *steps = 0;
    if ((size_t)cfg->width * (size_t)(y1 - y0) == 0) return FR_OK;
    uint64_t *const sums[2] = {passes, steps};
    return count_rows(sums, bla_rows(cfg, c, bits, y0, y1, 0, FR_OUT_COUNT));
}

int fr_debug_bla_table(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, int which,
                       uint32_t level, double *out, size_t cap, uint32_t *len) {
    const Centre c{pos_lo, centre};
    const int rc = check_bla(cfg, c, bits, 0, 0);
    if (rc != FR_OK) return rc;
    return bla_debug_table(cfg, c, bits, false, which, level, out, cap, len);
}

int fr::bla_debug_table(const fr_config *cfg, const Centre &c, int bits, bool scaled, int which, uint32_t level, double *out,
                        size_t cap, uint32_t *len) {
    if (cfg->algo != 0 && cfg->algo != 2) return fail(FR_ERR_INVALID_ARGUMENT, "BLA-PT: tables exist for Mandelbrot and Julia");
    if (which != 0 && !(which == 1 && cfg->algo == 2))
        return fail(FR_ERR_INVALID_ARGUMENT, "which must be 0 (the table of R or V) or, for Julia, 1 (K's)");
    if (!len) return fail(FR_ERR_INVALID_ARGUMENT, "len is NULL");
    if (cap && !out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    std::vector<double> X;
    pt_host_orbit(cfg, c, which, X);
    const uint32_t last = (uint32_t)(X.size() / 2 - 1);
    const double b0 = cfg->algo == 2 ? 0.0 : 1.0;
    fr_config image = *cfg;
    double S = 1.0;
    if (scaled) {
        const ScaledConsts k = scaled_consts(cfg);
        image.scale.re = k.sre, image.scale.im = k.sim, S = k.S;
    }
    HostTable t;
    build_table(X.data(), last, image_D(&image), b0, bits, S, scaled, t);
    const uint32_t n = level < 32 ? t.n0 >> level : 0;
    *len = n;
    const size_t w = std::min<size_t>(cap, n);
    if (level == 0) {
        const double eps = std::ldexp(1.0, -bits) * S;
        for (size_t j = 0; j < w; j++) {
            const Entry e = level0(X.data(), (uint32_t)j, b0, eps);
            double *o = out + 5 * j;
            o[0] = e.are, o[1] = e.aim, o[2] = e.bre, o[3] = e.bim, o[4] = stored_radius(e.r, scaled);
        }
        return FR_OK;
    }
    const size_t at = n ? bla_level_offset(t.n0, level) : 0;
    for (size_t j = 0; j < w; j++) {
        double *o = out + 5 * j;
        memcpy(o, &t.coef[4 * (at + j)], 4 * sizeof(double));
        o[4] = t.rad[at + j];
    }
    return FR_OK;
}

int fr_debug_bla_cache(uint32_t out[4]) {
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    out[0] = out[1] = out[2] = out[3] = 0;
    LifeShared ls;
    Ctx *ctx = primary_if_created();
    if (!ctx) return FR_OK;
    std::lock_guard<std::mutex> lk(ctx->pt_mu);
    const BlaTable *t = ctx->bla_table.get();
    if (!t) return FR_OK;
    out[0] = (uint32_t)t->bits;
    out[1] = t->x_levels;
    out[2] = t->entries;
    out[3] = t->built ? 1u : 0u;
    return FR_OK;
}
