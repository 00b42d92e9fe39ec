/*
 * fr_dd.hip — gfx950 kernel of FR_PRECISION_DD: the z = z^2 + c loop in double-double arithmetic (a value is an
 * unevaluated pair hi + lo of f64 values, about 106 significant bits), for zooms past the f64 limit (a pixel narrower
 * than one f64 ulp of pos: scale >~ 10^13 near |pos| ~ 0.75 at 1080 rows).
 *
 * The precision is DEFINED by the operation sequence in include/fractal_hip.h (fr_precision); every function below is
 * that sequence written out, with each fma spelt __builtin_fma (the library is built with -ffp-contract=off, so the
 * compiler fuses nothing by itself and reassociates nothing).  tests/dd_model.c restates the same definition in C on the
 * host; tests/test_gpu_dd.py compares the two bit for bit.  The only liberty taken is common-subexpression reuse the
 * compiler finds by itself (re'.hi * re'.hi of the escape test is the next iteration's sqr(re).p): the same IEEE
 * operation on the same operands, so the same bits.
 *
 * Shape (cdna_hip_programming: one lane per pixel, LDS for what a workgroup shares):
 *   - a workgroup of 4 waves renders 16 x 16 pixels, each wave one 8 x 8 tile;
 *   - the 16 column and 16 row start coordinates (dd) are computed once per workgroup by 32 lanes and staged in LDS
 *     (re depends on x only, im on y only), as escape_kernel does in f64;
 *   - each lane leaves the loop when its orbit escapes (the lane drops out of EXEC); the wave leaves when EXEC is
 *     empty or the wave-uniform counter reaches the cap.  No speculative blocks, no scaled loop, no two passes, no
 *     view sample: a Mandelbrot iteration costs ~83 f64 VALU operations here against ~6 in f64, so the loop itself is
 *     the only thing worth the registers;
 *   - outputs as fr_launch_escape's: RGB / RGBA (packed or in place), ESCAPE (hi parts, optionally lo parts, and the
 *     index), COUNT (executed iterations into FR_COUNT_SLOTS partial sums); 64-bit output offsets.
 */
#include "fr_kernels.h"

#include "fr_math.h"

namespace {

#include "fr_colour.h"

struct dd {
    double hi, lo;
};

/* ---- the definition (include/fractal_hip.h, fr_precision), operation for operation ---------------------------- */

__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    const double e = (a - (s - bb)) + (b - bb);
    return {s, e};
}

__device__ __forceinline__ dd fast_two_sum(double a, double b) {
    const double s = a + b;
    const double e = b - (s - a);
    return {s, e};
}

__device__ __forceinline__ dd add_dd(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return fast_two_sum(s.hi, s.lo);
}

__device__ __forceinline__ dd add_d(dd a, double d) {
    dd s = two_sum(a.hi, d);
    s.lo = s.lo + a.lo;
    return fast_two_sum(s.hi, s.lo);
}

__device__ __forceinline__ dd sqr(dd x) {
    const double p = x.hi * x.hi;
    double e = __builtin_fma(x.hi, x.hi, -p);
    e = __builtin_fma(x.hi + x.hi, x.lo, e);
    return fast_two_sum(p, e);
}

__device__ __forceinline__ dd twice_mul(dd x, dd y) {
    const double p = x.hi * y.hi;
    double e = __builtin_fma(x.hi, y.hi, -p);
    e = __builtin_fma(x.hi, y.lo, e);
    e = __builtin_fma(x.lo, y.hi, e);
    const dd h = fast_two_sum(p, e);
    return {h.hi + h.hi, h.lo + h.lo};
}

__device__ __forceinline__ dd neg(dd x) { return {-x.hi, -x.lo}; }

/* recursive() (calc/src/lib.rs:245-257) in dd: `next` with its index on escape, `previous` with `iterations` on
 * exhaustion.  JULIA: c is julia_set (f64) and the two outer additions are add_d. */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_dd(uint32_t iterations, dd &re, dd &im, dd cre, dd cim, double squared) {
    uint32_t i = 0;
    for (; i < iterations; i++) {
        const dd s = add_dd(sqr(re), neg(sqr(im)));
        const dd t = twice_mul(re, im);
        const dd nre = JULIA ? add_d(s, cre.hi) : add_dd(s, cre);
        const dd nim = JULIA ? add_d(t, cim.hi) : add_dd(t, cim);
        const double dist = nre.hi * nre.hi + nim.hi * nim.hi;
        re = nre;
        im = nim;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
    }
    return i;
}

/* start coordinate: coord_to_space (calc/src/lib.rs:181-197) without the final `+ pos`, then add_d onto (pos, pos_lo) */
__device__ __forceinline__ dd start_dd(double coord, double max, double offset, double pos, double pos_lo, double scale) {
    const double off = ((coord / max) - offset) / scale;
    return add_d(dd{pos, pos_lo}, off);
}

template <int MODE>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_dd_kernel(const fr_kparams p, const fr_kout out, const double lo_re,
                                                                    const double lo_im, const uint32_t with_lo) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    __shared__ dd s_re[kDeepBlockW];
    __shared__ dd s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;

    if (MODE == FR_OUT_RGB) {
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += 64 * kDeepWaves) s_tab[k] = gt[k];
    }
    if (tid < kDeepBlockW + kDeepBlockH) {
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kDeepBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            s_re[tid] = start_dd((double)x, height, (width / height) / 2.0, p.pos_re, lo_re, p.scale_re);
        } else {
            const uint32_t r = row0 + (tid - kDeepBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            s_im[tid - kDeepBlockW] = start_dd((double)y, height, 0.5, p.pos_im, lo_im, p.scale_im);
        }
    }
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    const bool valid = cx < p.ncols && r < p.nrows;
    const bool escape_algo = p.algo == 0 /* Mandelbrot */ || p.algo == 2 /* Julia */;

    dd re{0.0, 0.0}, im{0.0, 0.0};
    uint32_t iters = 0;
    if (valid && escape_algo) {
        re = s_re[lx];
        im = s_im[ly];
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        if (p.algo == 2)
            iters = orbit_dd<true>(p.iterations, re, im, dd{p.julia_re, 0.0}, dd{p.julia_im, 0.0}, squared);
        else
            iters = orbit_dd<false>(p.iterations, re, im, re, im, squared);
    }

    if constexpr (MODE == FR_OUT_RGB) {
        if (valid) {
            uint8_t rgb[3] = {0, 0, 0};
            if (escape_algo) {
                const ColourConsts cc = make_colour_consts(p);
                const double r2 = re.hi * re.hi, i2 = im.hi * im.hi;
                colour_pixel<double>(cc, re.hi, im.hi, r2, i2, iters, s_tab, nullptr, rgb); /* :214-234 on the hi parts */
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
                if (with_lo) {
                    out.z[4 * k] = re.hi;
                    out.z[4 * k + 1] = re.lo;
                    out.z[4 * k + 2] = im.hi;
                    out.z[4 * k + 3] = im.lo;
                } else {
                    out.z[2 * k] = re.hi;
                    out.z[2 * k + 1] = im.hi;
                }
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

/* Raise the cap of stored DD results in place (include/fractal_hip.h, fr_escape_extend_device): a stored (re, im, iters ==
 * N) — all four doubles, the low parts are state — is recursive()'s `previous` after N unescaped steps, and orbit_dd takes
 * it on for M - N more with the c the render uses (start_dd of the pixel, or julia_set).  escape_dd_kernel's shape: 4
 * waves, 16 x 16 pixels.  `iters` is read first; a workgroup with no pixel at N ends there, having written nothing, and a
 * finished pixel's z is neither loaded nor stored. */
__global__ __launch_bounds__(64 * kDeepWaves) void escape_extend_dd_kernel(const fr_kparams p, double *z, uint32_t *iters,
                                                                           const uint32_t from, const double lo_re, const double lo_im) {
    __shared__ dd s_re[kDeepBlockW];
    __shared__ dd s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    const bool valid = cx < p.ncols && r < p.nrows;
    const uint64_t k = (uint64_t)r * p.ncols + cx;
    uint32_t done = 0;
    if (valid) done = iters[k];
    const bool running = valid && done == from;
    if (!__syncthreads_or(running ? 1 : 0)) return; /* whole workgroup (uniform) */

    const bool julia = p.algo == 2;
    if (!julia) { /* uniform: c = the pixel's start, staged as escape_dd_kernel stages it */
        if (tid < kDeepBlockW + kDeepBlockH) {
            const double width = (double)p.width, height = (double)p.height;
            if (tid < kDeepBlockW) {
                const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
                s_re[tid] = start_dd((double)x, height, (width / height) / 2.0, p.pos_re, lo_re, p.scale_re);
            } else {
                const uint32_t rr = row0 + (tid - kDeepBlockW);
                const uint64_t y = (uint64_t)p.y_first + (uint64_t)(rr / p.block_rows) * p.y_stride + rr % p.block_rows;
                s_im[tid - kDeepBlockW] = start_dd((double)y, height, 0.5, p.pos_im, lo_im, p.scale_im);
            }
        }
        __syncthreads();
    }
    if (running) {
        dd re{z[4 * k], z[4 * k + 1]}, im{z[4 * k + 2], z[4 * k + 3]};
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        const uint32_t n = p.iterations - from;
        uint32_t it;
        if (julia)
            it = orbit_dd<true>(n, re, im, dd{p.julia_re, 0.0}, dd{p.julia_im, 0.0}, squared);
        else
            it = orbit_dd<false>(n, re, im, s_re[lx], s_im[ly], squared);
        z[4 * k] = re.hi;
        z[4 * k + 1] = re.lo;
        z[4 * k + 2] = im.hi;
        z[4 * k + 3] = im.lo;
        iters[k] = from + it; /* it == n on exhaustion: the new cap */
    }
}

}  // namespace

hipError_t fr_launch_escape_extend_dd(const fr_kparams &p, double pos_lo_re, double pos_lo_im, uint32_t from_iterations,
                                      double *z, uint32_t *iters, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "escape_extend_dd_kernel";
    if (p.ncols == 0 || p.nrows == 0) return hipSuccess;
    if (p.iterations < from_iterations || (p.algo != 0 && p.algo != 2)) return hipErrorInvalidValue;
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    escape_extend_dd_kernel<<<grid, block, 0, stream>>>(p, z, iters, from_iterations, pos_lo_re, pos_lo_im);
    return hipGetLastError();
}

hipError_t fr_launch_escape_dd(const fr_kparams &p, double pos_lo_re, double pos_lo_im, int mode, const fr_kout &out,
                               bool with_lo, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "escape_dd_kernel";
    if (p.ncols == 0 || p.nrows == 0) return hipSuccess;
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    const uint32_t wl = with_lo ? 1u : 0u;
    if (mode == FR_OUT_RGB)
        escape_dd_kernel<FR_OUT_RGB><<<grid, block, 0, stream>>>(p, out, pos_lo_re, pos_lo_im, wl);
    else if (mode == FR_OUT_ESCAPE)
        escape_dd_kernel<FR_OUT_ESCAPE><<<grid, block, 0, stream>>>(p, out, pos_lo_re, pos_lo_im, wl);
    else
        escape_dd_kernel<FR_OUT_COUNT><<<grid, block, 0, stream>>>(p, out, pos_lo_re, pos_lo_im, wl);
    return hipGetLastError();
}
