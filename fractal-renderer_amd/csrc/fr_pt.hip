/*
 * fr_pt.hip — FR_PRECISION_PT: deep zooms by perturbation.  The view's reference orbit is iterated once on the host in
 * double-double arithmetic (DD's operations) and stored as its f64 hi parts; every pixel then iterates in f64 only its
 * offset dz from that orbit, dz' = (2Z + dz) dz + dc, and rebases (dz = z, back to the orbit's start) when |z| < |dz|
 * or the orbit runs out, so one orbit serves the whole view (include/fractal_hip.h, fr_precision, states the sequence;
 * tests/pt_model.c restates it; tests/test_gpu_pt.py compares the two bit for bit).
 *
 * Host part: the orbits (R for Mandelbrot; V and K for Julia), computed with -ffp-contract=off and std::fma exactly where
 * the definition has fma, uploaded into device memory owned by the context and kept there for the next call of the same
 * view (Ctx::pt_orbit, guarded by Ctx::pt_mu).
 *
 * Device part, escape_pt_kernel<MODE, JULIA> (cdna_hip_programming: one lane per pixel, LDS for what a workgroup
 * shares):
 *   - a workgroup of 4 waves renders 16 x 16 pixels, each wave one 8 x 8 tile (DD's shape);
 *   - the 16 column and 16 row offsets `off` are computed once per workgroup by 32 lanes and staged in LDS, as is the
 *     log2 table for RGB;
 *   - one step is 4 fma + 4 add for dz' and z', 3 + 3 for the escape and rebase tests: ~14 f64 VALU operations against
 *     DD's ~89.  Each step needs the orbit entries X_m and X_{m+1}; the next index is m + 1 or, after a rebase, 0, so
 *     X_0 = 0 and X_1 (of the orbit rebased onto) stay in registers and the load of X_{m+2} is issued one step ahead,
 *     its latency hidden behind the step's arithmetic.  While no lane of a wave has rebased, the lanes share m and the
 *     16-byte load of an interleaved (re, im) entry is one cache line for the whole wave; afterwards it gathers, from
 *     an orbit that the L2 holds (16 B per entry);
 *   - outputs as escape_dd_kernel's: RGB / RGBA, ESCAPE (z, index), COUNT; 64-bit output offsets.
 */
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fr_ctx.h"
#include "fr_math.h"

namespace {

#include "fr_colour.h"

constexpr int kPtWaves = 4;               /* 256-thread workgroups */
constexpr int kPtTileW = 8, kPtTileH = 8; /* one wave = 8 x 8 pixels */
constexpr int kPtWavesX = 2, kPtWavesY = 2;
constexpr int kPtBlockW = kPtTileW * kPtWavesX, kPtBlockH = kPtTileH * kPtWavesY; /* 16 x 16 pixels per workgroup */

/* ---- device: the pixel loop (include/fractal_hip.h, fr_precision: PT), operation for operation ------------------- */

/* X: the orbit the pixel starts on (R or V), K: the one it rebases onto (R or K); *_last: index of the last entry.
 * Returns the escape index (or `iterations`), the final z in (out_re, out_im). */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt(uint32_t iterations, double off_re, double off_im, const double2 *x_orbit,
                                             const double2 *k_orbit, uint32_t x_last, uint32_t k_last, double squared,
                                             double &out_re, double &out_im) {
    const double2 *X = x_orbit;
    uint32_t last = x_last;
    uint32_t m = JULIA ? 0u : 1u;
    double dzr = off_re, dzi = off_im;
    const double dcr = JULIA ? 0.0 : off_re, dci = JULIA ? 0.0 : off_im;
    double2 Z = X[m], N = X[m + 1]; /* m <= last - 1 at the top of every step: X_{m+1} exists */
    const double2 K1 = k_orbit[1];  /* the entry after a rebase; K_0 = R_0 = 0 */
    double zr = Z.x + dzr, zi = Z.y + dzi;
    uint32_t i = 0;
    for (; i < iterations; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double ndr = __builtin_fma(tr, dzr, __builtin_fma(-ti, dzi, dcr));
        const double ndi = __builtin_fma(tr, dzi, __builtin_fma(ti, dzr, dci));
        m++;
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
        if (dist < dzr * dzr + dzi * dzi || m == last) {
            dzr = zr;
            dzi = zi;
            m = 0;
            if (JULIA) {
                X = k_orbit;
                last = k_last;
            }
            Z = make_double2(0.0, 0.0);
            N = K1;
        } else {
            Z = N;
            N = P;
        }
    }
    out_re = zr;
    out_im = zi;
    return i;
}

template <int MODE, bool JULIA>
__global__ __launch_bounds__(64 * kPtWaves) void escape_pt_kernel(const fr_kparams p, const fr_kout out,
                                                                 const double2 *__restrict__ x_orbit,
                                                                 const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                 const uint32_t k_last) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    __shared__ double s_re[kPtBlockW];
    __shared__ double s_im[kPtBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kPtBlockW - 1) / kPtBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kPtBlockW, row0 = by * kPtBlockH;

    if (MODE == FR_OUT_RGB) {
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += 64 * kPtWaves) s_tab[k] = gt[k];
    }
    if (tid < kPtBlockW + kPtBlockH) {
        /* off: coord_to_space (calc/src/lib.rs:181-197) without the final `+ pos`, DD's off */
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kPtBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            s_re[tid] = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        } else {
            const uint32_t r = row0 + (tid - kPtBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            s_im[tid - kPtBlockW] = (((double)y / height) - 0.5) / p.scale_im;
        }
    }
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kPtWavesX) * kPtTileW + lane % kPtTileW;
    const uint32_t ly = (wave / kPtWavesX) * kPtTileH + lane / kPtTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    const bool valid = cx < p.ncols && r < p.nrows;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    double zr = 0.0, zi = 0.0;
    uint32_t iters = 0;
    if (valid && escape_algo) {
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        iters = orbit_pt<JULIA>(p.iterations, s_re[lx], s_im[ly], x_orbit, k_orbit, x_last, k_last, squared, zr, zi);
    }

    if constexpr (MODE == FR_OUT_RGB) {
        if (valid) {
            uint8_t rgb[3] = {0, 0, 0};
            if (escape_algo) {
                const ColourConsts cc = make_colour_consts(p);
                const double r2 = zr * zr, i2 = zi * zi;
                colour_pixel<double>(cc, zr, zi, r2, i2, iters, s_tab, nullptr, rgb); /* :214-234 on the f64 z */
            }
            uint64_t row_out = r;
            if (p.out_in_place) row_out = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            const uint64_t k = row_out * p.ncols + cx;
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
    } else {
        unsigned long long n = 0;
        if (valid && escape_algo) n = iters < p.iterations ? (unsigned long long)iters + 1ull : p.iterations;
        for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
        if (lane == 0 && n) atomicAdd(out.count + ((blockIdx.x + 131u * wave) % FR_COUNT_SLOTS), n);
    }
}

template <bool JULIA>
hipError_t launch(const fr_kparams &p, int mode, const fr_kout &out, const double2 *x_orbit, const double2 *k_orbit,
                  uint32_t x_last, uint32_t k_last, hipStream_t stream) {
    const uint64_t tiles = (((uint64_t)p.ncols + kPtBlockW - 1) / kPtBlockW) * (((uint64_t)p.nrows + kPtBlockH - 1) / kPtBlockH);
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)tiles), block(64 * kPtWaves);
    if (mode == FR_OUT_RGB)
        escape_pt_kernel<FR_OUT_RGB, JULIA><<<grid, block, 0, stream>>>(p, out, x_orbit, k_orbit, x_last, k_last);
    else if (mode == FR_OUT_ESCAPE)
        escape_pt_kernel<FR_OUT_ESCAPE, JULIA><<<grid, block, 0, stream>>>(p, out, x_orbit, k_orbit, x_last, k_last);
    else
        escape_pt_kernel<FR_OUT_COUNT, JULIA><<<grid, block, 0, stream>>>(p, out, x_orbit, k_orbit, x_last, k_last);
    return hipGetLastError();
}

/* ---- host: the reference orbits, DD's operations (include/fractal_hip.h) with std::fma where the definition has fma -- */

struct ddh {
    double hi, lo;
};

ddh two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

ddh fast_two_sum(double a, double b) {
    const double s = a + b;
    return {s, b - (s - a)};
}

ddh add_dd(ddh a, ddh b) {
    ddh s = two_sum(a.hi, b.hi);
    const ddh t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return fast_two_sum(s.hi, s.lo);
}

ddh add_d(ddh a, double d) {
    ddh s = two_sum(a.hi, d);
    s.lo = s.lo + a.lo;
    return fast_two_sum(s.hi, s.lo);
}

ddh sqr(ddh x) {
    const double p = x.hi * x.hi;
    double e = std::fma(x.hi, x.hi, -p);
    e = std::fma(x.hi + x.hi, x.lo, e);
    return fast_two_sum(p, e);
}

ddh twice_mul(ddh x, ddh y) {
    const double p = x.hi * y.hi;
    double e = std::fma(x.hi, y.hi, -p);
    e = std::fma(x.hi, y.lo, e);
    e = std::fma(x.lo, y.hi, e);
    const ddh h = fast_two_sum(p, e);
    return {h.hi + h.hi, h.lo + h.lo};
}

ddh neg(ddh x) { return {-x.hi, -x.lo}; }

/* orbit `which` (0: R or V, 1: K) of the view as re, im pairs of the hi parts; at most iterations + 2 entries */
void reference_orbit(const fr_config *cfg, double lo_re, double lo_im, int which, std::vector<double> &out) {
    const bool julia = cfg->algo == 2;
    const uint32_t kmin = julia ? 1u : 2u;
    const uint32_t kmax = julia ? (cfg->iterations > 1 ? cfg->iterations : 1u) : cfg->iterations + 1u;
    const ddh cre{cfg->pos.re, lo_re}, cim{cfg->pos.im, lo_im};
    ddh zr{0.0, 0.0}, zi{0.0, 0.0};
    if (julia && which == 0) zr = cre, zi = cim;
    out.clear();
    out.reserve(2 * ((size_t)kmax + 1));
    for (uint32_t k = 0;; k++) {
        out.push_back(zr.hi);
        out.push_back(zi.hi);
        if (k >= kmin && zr.hi * zr.hi + zi.hi * zi.hi > 4.0) break;
        if (k == kmax) break;
        if (!julia && k == 0) {
            zr = cre, zi = cim; /* R_1 = C */
        } else {
            const ddh a = add_dd(sqr(zr), neg(sqr(zi)));
            const ddh b = twice_mul(zr, zi);
            if (julia) {
                zr = add_d(a, cfg->julia_set.re);
                zi = add_d(b, cfg->julia_set.im);
            } else {
                zr = add_dd(a, cre);
                zi = add_dd(b, cim);
            }
        }
    }
}

}  // namespace

namespace fr {

/* the orbits of one view in device memory: X (R or V) at dev[0 ..], K (Julia) after it */
struct PtOrbit {
    uint32_t algo = 0, iterations = 0;
    double key[6] = {}; /* pos.re, pos.im, pos_lo.re, pos_lo.im, julia_set.re, julia_set.im, compared bit for bit */
    double2 *dev = nullptr;
    uint32_t x_last = 0, k_last = 0;
    size_t k_offset = 0; /* entries */
    ~PtOrbit() {
        if (dev) (void)hipFree(dev); /* hipFree waits for the device: no kernel still reads the orbit */
    }
};

namespace {

void view_key(const fr_config *cfg, const fr_imaginary *pos_lo, double key[6]) {
    key[0] = cfg->pos.re;
    key[1] = cfg->pos.im;
    key[2] = pos_lo ? pos_lo->re : 0.0;
    key[3] = pos_lo ? pos_lo->im : 0.0;
    key[4] = cfg->algo == 2 ? cfg->julia_set.re : 0.0;
    key[5] = cfg->algo == 2 ? cfg->julia_set.im : 0.0;
}

/* the view's orbits, from the context's cache or computed and uploaded; the caller keeps `out` alive until its launch
 * has been enqueued (a later view may replace the cache entry meanwhile; the last reference frees it) */
int orbit_for(Ctx &ctx, const fr_config *cfg, const fr_imaginary *pos_lo, std::shared_ptr<PtOrbit> &out) {
    double key[6];
    view_key(cfg, pos_lo, key);
    std::lock_guard<std::mutex> lk(ctx.pt_mu);
    const std::shared_ptr<PtOrbit> &c = ctx.pt_orbit;
    if (c && c->algo == cfg->algo && c->iterations == cfg->iterations && memcmp(c->key, key, sizeof key) == 0) {
        out = c;
        return FR_OK;
    }
    std::vector<double> x, k;
    reference_orbit(cfg, key[2], key[3], 0, x);
    if (cfg->algo == 2) reference_orbit(cfg, key[2], key[3], 1, k);
    auto o = std::make_shared<PtOrbit>();
    o->algo = cfg->algo;
    o->iterations = cfg->iterations;
    memcpy(o->key, key, sizeof key);
    o->x_last = (uint32_t)(x.size() / 2 - 1);
    o->k_offset = x.size() / 2;
    o->k_last = k.empty() ? o->x_last : (uint32_t)(k.size() / 2 - 1);
    const size_t bytes = (x.size() + k.size()) * sizeof(double);
    ctx.pt_orbit.reset(); /* the previous view's orbit goes first: its memory is free for this one */
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&o->dev), bytes));
    HIP_TRY(hipMemcpy(o->dev, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!k.empty()) HIP_TRY(hipMemcpy(o->dev + o->k_offset, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx.pt_orbit = o;
    out = std::move(o);
    return FR_OK;
}

}  // namespace

int launch_pt(Ctx &ctx, const fr_config *cfg, const fr_imaginary *pos_lo, const fr_kparams &p, int mode, const fr_kout &out,
              hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "escape_pt_kernel";
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    const bool julia = cfg->algo == 2;
    if (cfg->algo != 0 && !julia) { /* no escape-time algorithm: every pixel is black / zero, as DD's kernel gives */
        HIP_TRY(launch<false>(p, mode, out, nullptr, nullptr, 0, 0, stream));
        return FR_OK;
    }
    std::shared_ptr<PtOrbit> o;
    const int rc = orbit_for(ctx, cfg, pos_lo, o);
    if (rc != FR_OK) return rc;
    if (julia) {
        HIP_TRY(launch<true>(p, mode, out, o->dev, o->dev + o->k_offset, o->x_last, o->k_last, stream));
    } else {
        HIP_TRY(launch<false>(p, mode, out, o->dev, o->dev, o->x_last, o->x_last, stream));
    }
    return FR_OK;
}

}  // namespace fr

int fr_debug_reference_orbit(const fr_config *cfg, const fr_imaginary *pos_lo, int which, double *out, size_t cap,
                             uint32_t *len) {
    using namespace fr;
    int rc = check_pt(cfg, pos_lo);
    if (rc != FR_OK) return rc;
    if (cfg->algo != 0 && cfg->algo != 2) return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_PT: orbits exist for Mandelbrot and Julia");
    if (which != 0 && !(which == 1 && cfg->algo == 2))
        return fail(FR_ERR_INVALID_ARGUMENT, "which must be 0 (R or V) or, for Julia, 1 (K)");
    if (!len) return fail(FR_ERR_INVALID_ARGUMENT, "len is NULL");
    if (cap && !out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    std::vector<double> v;
    reference_orbit(cfg, pos_lo ? pos_lo->re : 0.0, pos_lo ? pos_lo->im : 0.0, which, v);
    *len = (uint32_t)(v.size() / 2);
    const size_t n = std::min(cap, v.size() / 2);
    if (n) memcpy(out, v.data(), n * 2 * sizeof(double));
    return FR_OK;
}
