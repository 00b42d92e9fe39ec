/*
 * fr_scaled.hip — SCALED PT: WIDE PT and BLA-PT past a scale of 2^440 (include/fractal_hip.h, fr_precision: "SCALED PT";
 * tests/pt_scaled_model.c restates it; tests/test_gpu_pt_scaled.py compares the two bit for bit).  The pixel's offset from
 * the reference orbit is carried as w = dz 2^e, e the exponent of the view's scale, so that neither it nor the squares the
 * loop compares leave f64's normal range; multiplying by a power of two commutes with every rounding, so inside WIDE PT's
 * domain the kernels here give escape_pt_kernel's and escape_bla_kernel's results bit for bit.
 *
 * Host part: nothing of its own.  The orbits are WIDE PT's (fr_pt.hip's cache, shared with the wide calls), the table is
 * fr_bla.hip's build in its scaled form (R in place of r2), cached in the context's one table slot.
 *
 * Device part: escape_pt_scaled_kernel<MODE, JULIA> (bits = -1, no table) and escape_bla_scaled_kernel<MODE, JULIA>, in the
 * shape of the kernels they extend (cdna_hip_programming: one lane per pixel, LDS for what a workgroup shares) — a workgroup
 * of 4 waves renders 16 x 16 pixels, each wave one 8 x 8 tile, woff and the log2 table staged in LDS, 64-bit output offsets,
 * plain vector loads and stores.  woff is PT's off with the divisor scale 2^-e, so the staging code is PT's on a copy of the
 * parameters that holds (sre, sim).  What a scaled step adds to its unscaled counterpart:
 *   - z = fma(w', Sinv, X_m) where PT has an addition;
 *   - the two-sided comparisons.  Both forms of the rebase test are  (z fl)^2 < (w fr)^2  with (fl, fr) = (1, Sinv) for a big
 *     w and (S, 1) otherwise: the factors are SELECTED (two v_cndmask pairs) and the four multiplies, two squares-and-sums
 *     and one compare run on one path for every lane; a multiplication by 1 is exact, so each lane computes exactly the
 *     expression of its form.  The level search does the same with f = Sinv or 1 on w and on each R it probes.
 *
 * Resumable SCALED PT (include/fractal_hip.h, "RESUMABLE SCALED PT"; tests/pt_scaled_state_model.c restates it;
 * tests/test_gpu_pt_scaled_state.py compares the two bit for bit): escape_pt_scaled_state_kernel<JULIA> is the plain loop's
 * ESCAPE render with the state rule — no rebase at the end of an orbit that the cap cut — and stores the whole state
 * (z, iters, w, m); escape_extend_pt_scaled_kernel<JULIA> continues such a state to a higher cap in place, on orbits that
 * fr_pt.hip's cache continued from their integer tails.  They are to orbit_pt_scaled what fr_pt.hip's escape_pt_state_kernel
 * and escape_extend_pt_kernel are to orbit_pt, in their shape; escape_pt_scaled_kernel and orbit_pt_scaled are SCALED PT's and
 * stay as they are.  The table form has no state (BLA-PT's reason: i + 2^k <= iterations).
 *
 * ADAPTIVE SUPERSAMPLING (include/fractal_hip.h; fr_ss_adaptive.hip): ss_refine_scaled_kernel<JULIA, BLA>, persistent waves that
 * run orbit_pt_scaled / orbit_bla_scaled on the s x s samples of the listed edge pixels (fr_ss_list.h: the claim loop);
 * scaled_render_map, the RGB launch over the probe's strided map, and scaled_ss_refine, the refine launch.
 *
 * What the kernels here share with those of DE ON SCALED PT (fr_de_scaled.hip) lives in fr_scaled.h, one copy: ScaledDev and its
 * fill from the context's caches, kBig, kOnK, is_big, rebase_test and stage_woff.
 *
 * The calls, at the end of the file: each builds its Centre (scaled: the wide centre is required), runs check_scaled and hands
 * scaled_rows — the profiled launch of its rows — to the row-call body of its form in fr_ctx.h, as fr_bla.hip's do; the state
 * calls hand scaled_state_rows to fr_ctx.h's state road (state_device, state_host), as fr_pt.hip's do.  The workgroup's
 * geometry and the launches' grid are the deep kernels' (fr_kernels.h: kDeep*, fr_deep_grid).
 */
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fr_bla.h"
#include "fr_ctx.h"
#include "fr_math.h"
#include "fr_scaled.h"
#include "fr_ss_list.h"
#include "fr_wide.h"

namespace {

#include "fr_colour.h"

/* ---- device: the plain scaled loop (include/fractal_hip.h, "SCALED PT", bits = -1), operation for operation -------------- */

/* orbit_pt (fr_pt.hip) with w for dz: X_0 = 0 and X_1 of the orbit rebased onto stay in registers, X_{m+2} is loaded one
 * step ahead.  Returns the escape index (or `iterations`), the final z in (out_re, out_im). */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_scaled(uint32_t iterations, double woff_re, double woff_im, const ScaledDev &t,
                                                    double squared, double &out_re, double &out_im) {
    const double S = t.S, Sinv = t.Sinv;
    const double2 *X = t.x_orbit;
    uint32_t last = t.x_last;
    uint32_t m = JULIA ? 0u : 1u;
    double wr = woff_re, wi = woff_im;
    const double wcr = JULIA ? 0.0 : woff_re, wci = JULIA ? 0.0 : woff_im;
    double2 Z = X[m], N = X[min(m + 1u, last)]; /* m <= last - 1 at the top of every step (a cap of 0 takes none) */
    const double2 K1 = t.k_orbit[1]; /* the entry after a rebase; K_0 = R_0 = 0 */
    double zr = __builtin_fma(wr, Sinv, Z.x), zi = __builtin_fma(wi, Sinv, Z.y);
    uint32_t i = 0;
    for (; i < iterations; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double nwr = __builtin_fma(tr, wr, __builtin_fma(-ti, wi, wcr));
        const double nwi = __builtin_fma(tr, wi, __builtin_fma(ti, wr, wci));
        m++;
        zr = __builtin_fma(nwr, Sinv, N.x);
        zi = __builtin_fma(nwi, Sinv, N.y);
        wr = nwr;
        wi = nwi;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
        if (rebase_test(zr, zi, wr, wi, S, Sinv) || m == last) {
            wr = zr * S;
            wi = zi * S;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                last = t.k_last;
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

/* ---- device: the resumable state of the plain scaled loop (include/fractal_hip.h, "RESUMABLE SCALED PT") ----------------- */

/* A pixel's state between steps: z, w, the index m into the orbit it follows and whether that orbit is K (Julia after a
 * rebase).  orbit_pt_scaled_state is orbit_pt_state (fr_pt.hip) with w for dz: it runs `steps` steps of the plain scaled loop
 * from the state with the state rule's rebase condition — the scaled rebase test, or m == last of an orbit that is ENDED BY
 * ESCAPE (x_end / k_end: that last index, or ~0 for an orbit cut by the cap, which m never equals) — and leaves the state
 * after the last step in `s`; on escape the state is (z, 0, 0).  Returns the steps completed before the escape (`steps`:
 * none).  t.x_last / t.k_last only clamp the loads. */
struct ScaledState {
    double zr, zi, wr, wi;
    uint32_t m;
    bool on_k;
};

template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_scaled_state(uint32_t steps, double wcr, double wci, const ScaledDev &t, uint32_t x_end,
                                                          uint32_t k_end, double squared, ScaledState &s) {
    const double S = t.S, Sinv = t.Sinv;
    const bool on_k = JULIA && s.on_k;
    const double2 *X = on_k ? t.k_orbit : t.x_orbit;
    uint32_t last = on_k ? t.k_last : t.x_last, end = on_k ? k_end : x_end;
    uint32_t m = s.m;
    bool k_now = on_k;
    double wr = s.wr, wi = s.wi, zr = s.zr, zi = s.zi;
    double2 Z = X[min(m, last)], N = X[min(m + 1u, last)]; /* m < last at the top of every step */
    const double2 K1 = t.k_orbit[1];                       /* the entry after a rebase; K_0 = R_0 = 0 */
    uint32_t i = 0;
    for (; i < steps; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double nwr = __builtin_fma(tr, wr, __builtin_fma(-ti, wi, wcr));
        const double nwi = __builtin_fma(tr, wi, __builtin_fma(ti, wr, wci));
        m++;
        zr = __builtin_fma(nwr, Sinv, N.x);
        zi = __builtin_fma(nwi, Sinv, N.y);
        wr = nwr;
        wi = nwi;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
        if (rebase_test(zr, zi, wr, wi, S, Sinv) || m == end) {
            wr = zr * S;
            wi = zi * S;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                last = t.k_last;
                end = k_end;
                k_now = true;
            }
            Z = make_double2(0.0, 0.0);
            N = K1;
        } else {
            Z = N;
            N = P;
        }
    }
    const bool escaped = i < steps; /* (z, 0, 0) for an escaped lane */
    s.zr = zr;
    s.zi = zi;
    s.wr = escaped ? 0.0 : wr;
    s.wi = escaped ? 0.0 : wi;
    s.m = escaped ? 0u : m;
    s.on_k = !escaped && k_now;
    return i;
}

/* escape_pt_scaled_kernel<FR_OUT_ESCAPE>'s shape with the state rule, storing the whole state: z and w as re, im per pixel,
 * iters, m (bit 31: on K).  `ended`: bit 0 = X, bit 1 = K is ended by escape.  An algorithm without orbits writes zeros. */
template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_pt_scaled_state_kernel(const fr_kparams p, double *__restrict__ z,
                                                                                 uint32_t *__restrict__ iters, double *__restrict__ w,
                                                                                 uint32_t *__restrict__ mm, const ScaledDev t,
                                                                                 const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;
    stage_woff(p, tid, col0, row0, s_re, s_im);
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    if (cx >= p.ncols || r >= p.nrows) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    ScaledState s{0.0, 0.0, 0.0, 0.0, 0u, false};
    uint32_t it = 0;
    if (escape_algo) {
        const double woff_re = s_re[lx], woff_im = s_im[ly];
        s.m = JULIA ? 0u : 1u;
        s.wr = woff_re;
        s.wi = woff_im;
        const double2 X0 = t.x_orbit[min(s.m, t.x_last)];
        s.zr = __builtin_fma(s.wr, t.Sinv, X0.x);
        s.zi = __builtin_fma(s.wi, t.Sinv, X0.y);
        it = orbit_pt_scaled_state<JULIA>(p.iterations, JULIA ? 0.0 : woff_re, JULIA ? 0.0 : woff_im, t, (ended & 1u) ? t.x_last : ~0u,
                                          (ended & 2u) ? t.k_last : ~0u, p.limit * p.limit, s);
    }
    const uint64_t k = (uint64_t)r * p.ncols + cx;
    z[2 * k] = s.zr;
    z[2 * k + 1] = s.zi;
    iters[k] = it;
    w[2 * k] = s.wr;
    w[2 * k + 1] = s.wi;
    mm[k] = s.m | (s.on_k ? kOnK : 0u);
}

/* Continue a stored state from cap `from` to p.iterations in place (escape_extend_pt_kernel's early-out): `iters` is read
 * first and a workgroup with no pixel at `from` ends there, having written nothing; a finished pixel's z, w and m are
 * neither loaded nor stored.  The orbits are those of the new cap. */
template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_extend_pt_scaled_kernel(const fr_kparams p, double *z, uint32_t *iters, double *w,
                                                                                  uint32_t *mm, const uint32_t from, const ScaledDev t,
                                                                                  const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

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

    if (!JULIA) { /* wc = the pixel's woff, staged as the render stages it; Julia's wc is 0 */
        stage_woff(p, tid, col0, row0, s_re, s_im);
        __syncthreads();
    }
    if (running) {
        const uint32_t word = mm[k];
        ScaledState s;
        s.zr = z[2 * k];
        s.zi = z[2 * k + 1];
        s.wr = w[2 * k];
        s.wi = w[2 * k + 1];
        s.on_k = JULIA && (word & kOnK) != 0;
        /* m < last of the orbit followed in every state this view produces; the clamp keeps foreign data inside the orbit */
        s.m = min(word & ~kOnK, (s.on_k ? t.k_last : t.x_last) - 1u);
        const uint32_t it = orbit_pt_scaled_state<JULIA>(p.iterations - from, JULIA ? 0.0 : s_re[lx], JULIA ? 0.0 : s_im[ly], t,
                                                         (ended & 1u) ? t.x_last : ~0u, (ended & 2u) ? t.k_last : ~0u,
                                                         p.limit * p.limit, s);
        z[2 * k] = s.zr;
        z[2 * k + 1] = s.zi;
        w[2 * k] = s.wr;
        w[2 * k + 1] = s.wi;
        mm[k] = s.m | (s.on_k ? kOnK : 0u);
        iters[k] = from + it; /* it == M - N on exhaustion: the new cap */
    }
}

/* ---- device: the scaled loop with table skips (bits >= 0) ------------------------------------------------------------- */

/* orbit_bla (fr_bla.hip) with w for dz and R for r2.  Returns the escape index (or `iterations`), the final z in (out_re,
 * out_im), the passes through the loop in `passes`. */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_bla_scaled(uint32_t iterations, double woff_re, double woff_im, const ScaledDev &t,
                                                     double squared, double &out_re, double &out_im, uint32_t &passes) {
    const double S = t.S, Sinv = t.Sinv;
    const double2 *X = t.x_orbit;
    const double *R = t.x_R, *CF = t.x_coef;
    uint32_t last = t.x_last, n0 = t.x_n0;
    uint32_t m = JULIA ? 0u : 1u;
    double wr = woff_re, wi = woff_im;
    const double wcr = JULIA ? 0.0 : woff_re, wci = JULIA ? 0.0 : woff_im;
    double2 Z = X[m]; /* X_m of the orbit followed */
    double zr = __builtin_fma(wr, Sinv, Z.x), zi = __builtin_fma(wi, Sinv, Z.y);
    uint32_t i = 0, np = 0, result = iterations;
    while (i < iterations) {
        np++;
        /* 1. the level: the largest k in 1 .. kc with (w f)^2 < (R f)^2 (R is non-increasing in k for a fixed first step) */
        const uint32_t j = m - 1u;
        uint32_t K = 0;
        if (m >= 1u && j < n0) {
            const double f = is_big(wr, wi) ? Sinv : 1.0;
            const double ar = wr * f, ai = wi * f;
            const double d2 = ar * ar + ai * ai;
            uint32_t kc = j ? (uint32_t)__builtin_ctz(j) : 31u;          /* j % 2^k == 0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(n0 - j));         /* (j >> k) < n_k, that is j + 2^k <= n0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(iterations - i)); /* i + 2^k <= iterations */
            uint32_t lo = 0, hi = kc;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                const double Rf = R[bla_level_offset(n0, mid) + (j >> mid)] * f;
                if (d2 < Rf * Rf)
                    lo = mid;
                else
                    hi = mid - 1u;
            }
            K = lo;
        }
        /* 2. the step: A and the constant term c of w' = A w + c — one arithmetic path, only the loads behind the branch */
        double ar, ai, cr = wcr, ci = wci;
        uint32_t step = 1u;
        if (K) {
            const uint32_t e = bla_level_offset(n0, K) + (j >> K);
            if (JULIA) { /* B wc: fma(B.re, 0, -(B.im * 0)) and fma(B.re, 0, B.im * 0) are +0 = wc for every finite B */
                const double2 A = reinterpret_cast<const double2 *>(CF)[e];
                ar = A.x, ai = A.y;
            } else {
                const double4 AB = reinterpret_cast<const double4 *>(CF)[e];
                ar = AB.x, ai = AB.y;
                cr = __builtin_fma(AB.z, wcr, -(AB.w * wci));
                ci = __builtin_fma(AB.z, wci, AB.w * wcr);
            }
            step = 1u << K;
        } else {
            ar = Z.x + zr, ai = Z.y + zi; /* t = X_m + z */
        }
        const double nwr = __builtin_fma(ar, wr, __builtin_fma(-ai, wi, cr));
        const double nwi = __builtin_fma(ar, wi, __builtin_fma(ai, wr, ci));
        m += step;
        i += step;
        const double2 N = X[min(m, last)]; /* m <= last: 1 + ((j >> K) + 1) 2^K <= 1 + n0 */
        zr = __builtin_fma(nwr, Sinv, N.x);
        zi = __builtin_fma(nwi, Sinv, N.y);
        wr = nwr;
        wi = nwi;
        /* 3. the tests, the plain scaled loop's */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) { /* this lane leaves EXEC; the wave goes on while any lane is left */
            result = i - 1u;
            break;
        }
        if (rebase_test(zr, zi, wr, wi, S, Sinv) || m == last) {
            wr = zr * S;
            wi = zi * S;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                R = t.k_R;
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

/* ---- device: the kernels: one body, the loop chosen by BLA ------------------------------------------------------------- */

template <int MODE, bool JULIA, bool BLA>
__device__ __forceinline__ void scaled_body(const fr_kparams &p, const fr_kout &out, const ScaledDev &t) {
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
        /* woff: PT's off with the scaled divisors — p.scale_re and p.scale_im hold sre and sim */
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
        if constexpr (BLA) {
            iters = orbit_bla_scaled<JULIA>(p.iterations, s_re[lx], s_im[ly], t, squared, zr, zi, passes);
        } else {
            iters = orbit_pt_scaled<JULIA>(p.iterations, s_re[lx], s_im[ly], t, squared, zr, zi);
            passes = iters < p.iterations ? iters + 1u : p.iterations; /* every pass is one step */
        }
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

template <int MODE, bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_pt_scaled_kernel(const fr_kparams p, const fr_kout out, const ScaledDev t) {
    scaled_body<MODE, JULIA, false>(p, out, t);
}

template <int MODE, bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_bla_scaled_kernel(const fr_kparams p, const fr_kout out, const ScaledDev t) {
    scaled_body<MODE, JULIA, true>(p, out, t);
}

template <bool JULIA, bool BLA>
hipError_t launch(const fr_kparams &p, int mode, const fr_kout &out, const ScaledDev &t, hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    if constexpr (BLA) {
        if (mode == FR_OUT_RGB)
            escape_bla_scaled_kernel<FR_OUT_RGB, JULIA><<<grid, block, 0, stream>>>(p, out, t);
        else if (mode == FR_OUT_ESCAPE)
            escape_bla_scaled_kernel<FR_OUT_ESCAPE, JULIA><<<grid, block, 0, stream>>>(p, out, t);
        else
            escape_bla_scaled_kernel<FR_OUT_COUNT, JULIA><<<grid, block, 0, stream>>>(p, out, t);
    } else {
        if (mode == FR_OUT_RGB)
            escape_pt_scaled_kernel<FR_OUT_RGB, JULIA><<<grid, block, 0, stream>>>(p, out, t);
        else if (mode == FR_OUT_ESCAPE)
            escape_pt_scaled_kernel<FR_OUT_ESCAPE, JULIA><<<grid, block, 0, stream>>>(p, out, t);
        else
            escape_pt_scaled_kernel<FR_OUT_COUNT, JULIA><<<grid, block, 0, stream>>>(p, out, t);
    }
    return hipGetLastError();
}

hipError_t launch(bool julia, bool bla, const fr_kparams &p, int mode, const fr_kout &out, const ScaledDev &t, hipStream_t stream) {
    if (bla) return julia ? launch<true, true>(p, mode, out, t, stream) : launch<false, true>(p, mode, out, t, stream);
    return julia ? launch<true, false>(p, mode, out, t, stream) : launch<false, false>(p, mode, out, t, stream);
}

/* ---- device: ADAPTIVE SUPERSAMPLING's refine pass (include/fractal_hip.h; fr_ss_list.h: the claim loop) ---------------- */

/* ss_refine_pt_kernel (fr_pt.hip) with the scaled loops: `woff` by scaled_body's formula on cfg_s (`p` holds cfg_s with the
 * scaled divisors sre, sim), the loop chosen by BLA, the table built with Dw over the whole image of cfg_s */
template <bool JULIA, bool BLA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_scaled_kernel(const fr_kparams p, const fr_ss_refine a, const ScaledDev t) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kSsRefineThreads) s_tab[k] = gt[k];
    const uint16_t *const s_lt = ss_refine_tables<LINEAR>(); /* LINEAR-LIGHT SUPERSAMPLING: staged with the log2 table */
    __syncthreads();
    const double width = (double)p.width, height = (double)p.height;
    const double squared = p.limit * p.limit;
    ss_refine_loop<LINEAR>(a, s_lt, [&](uint64_t x, uint64_t y) {
        const double woff_re = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        const double woff_im = (((double)y / height) - 0.5) / p.scale_im;
        double zr, zi;
        uint32_t iters;
        if constexpr (BLA) {
            uint32_t passes;
            iters = orbit_bla_scaled<JULIA>(p.iterations, woff_re, woff_im, t, squared, zr, zi, passes);
        } else {
            iters = orbit_pt_scaled<JULIA>(p.iterations, woff_re, woff_im, t, squared, zr, zi);
        }
        uint8_t rgb[3] = {0, 0, 0};
        const ColourConsts cc = make_colour_consts(p);
        colour_pixel<double>(cc, zr, zi, zr * zr, zi * zi, iters, s_tab, nullptr, rgb);
        return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
    });
}

/* the state render, or — extend — the extension from `from` */
template <bool JULIA>
hipError_t launch_state(const fr_kparams &p, uint32_t from, bool extend, double *z, uint32_t *iters, double *w, uint32_t *m,
                        const ScaledDev &t, uint32_t ended, hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    if (extend)
        escape_extend_pt_scaled_kernel<JULIA><<<grid, block, 0, stream>>>(p, z, iters, w, m, from, t, ended);
    else
        escape_pt_scaled_state_kernel<JULIA><<<grid, block, 0, stream>>>(p, z, iters, w, m, t, ended);
    return hipGetLastError();
}

}  // namespace

namespace fr {
namespace {

/* `p` holds the view's scale; the kernels get a copy with the scaled divisors.  bits < 0: no table. */
int launch_scaled(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_kparams &p, int mode, const fr_kout &out,
                  hipStream_t stream) {
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    const bool julia = cfg->algo == 2, bla = bits >= 0;
    if (cfg->algo != 0 && !julia) { /* no escape-time algorithm: every pixel is black / zero, as PT's kernel gives */
        HIP_TRY(launch(false, bla, p, mode, out, ScaledDev{}, stream));
        return FR_OK;
    }
    const ScaledConsts k = scaled_consts(cfg);
    fr_kparams ps = p;
    ps.scale_re = k.sre;
    ps.scale_im = k.sim;
    std::shared_ptr<PtOrbit> orbit;
    std::shared_ptr<BlaTable> table;
    ScaledDev t;
    const int rc = scaled_dev_fill(ctx, cfg, c, bits, k, orbit, table, t);
    if (rc != FR_OK) return rc;
    HIP_TRY(launch(julia, bla, ps, mode, out, t, stream));
    return FR_OK;
}

/* ---- the calls ------------------------------------------------------------------------------------------------------ */

/* SCALED PT's domain (include/fractal_hip.h); table: the call is about a table, so bits = -1 is no answer */
int check_scaled(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1, bool table = false) {
    int rc = check_rows(cfg, y0, y1);
    if (rc == FR_OK) rc = c.check(cfg, FR_PRECISION_PT);
    if (rc != FR_OK) return rc;
    if (bits == 0) bits = FR_BLA_DEFAULT_BITS;
    if (table && (bits < 24 || bits > 53))
        return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: the bits of a table are 0 (FR_BLA_DEFAULT_BITS) or 24 .. 53");
    if (bits != -1 && (bits < 24 || bits > 53))
        return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: bits must be -1 (no table), 0 (FR_BLA_DEFAULT_BITS) or 24 .. 53");
    return FR_OK;
}

/* The launch every row call below hands to its helper (fr_ctx.h): rows [y0, y1) in `mode` on `stream` between the profiling
 * events; the colour constants alone: no loop plan, no kernel choice, no view sample */
auto scaled_rows(const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, unsigned channels, int mode) {
    return [=](Ctx &ctx, const fr_kout &out, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, channels, stream, [&](fr_kparams &p, const char *&kname) {
            kname = bits < 0 ? "escape_pt_scaled_kernel" : "escape_bla_scaled_kernel";
            return launch_scaled(ctx, cfg, c, bits, p, mode, out, stream);
        });
    };
}

/* ---- RESUMABLE SCALED PT: the plain loop's rows with their state, and that state continued to a higher cap -------------- */

/* The launch of the state road (fr_ctx.h: state_device, state_host).  from == nullptr: the state render; else the extension
 * from *from, on the orbits of cfg's cap, which pt_orbit_view's cache continues from those of the old one.  Into the arrays it
 * is given, between the profiling events. */
auto scaled_state_rows(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from) {
    return [=](Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_w, uint32_t *d_m, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, 0, stream, [&](fr_kparams &p, const char *&kname) -> int {
            kname = from ? "escape_extend_pt_scaled_kernel" : "escape_pt_scaled_state_kernel";
            const bool julia = cfg->algo == 2, extend = from != nullptr;
            if (cfg->algo != 0 && !julia) { /* no escape-time algorithm: zeros in all four arrays (the extension never gets here) */
                HIP_TRY(launch_state<false>(p, 0, false, d_z, d_iters, d_w, d_m, ScaledDev{}, 0, stream));
                return FR_OK;
            }
            const ScaledConsts k = scaled_consts(cfg);
            p.scale_re = k.sre;
            p.scale_im = k.sim;
            std::shared_ptr<PtOrbit> orbit;
            PtOrbitView v;
            const int rc = pt_orbit_view(ctx, cfg, c, orbit, v);
            if (rc != FR_OK) return rc;
            ScaledDev t{};
            t.x_orbit = v.x;
            t.k_orbit = v.k;
            t.x_last = v.x_last;
            t.k_last = v.k_last;
            t.S = k.S;
            t.Sinv = k.Sinv;
            const uint32_t n = extend ? *from : 0u;
            HIP_TRY(julia ? launch_state<true>(p, n, extend, d_z, d_iters, d_w, d_m, t, v.ended, stream)
                          : launch_state<false>(p, n, extend, d_z, d_iters, d_w, d_m, t, v.ended, stream));
            return FR_OK;
        });
    };
}

/* the state calls are the plain loop's: SCALED PT's domain with bits = -1 */
int check_scaled_plain(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1) {
    int bits = -1;
    return check_scaled(cfg, c, bits, y0, y1);
}

int scaled_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z,
                        void *d_iters, void *d_w, void *d_m, void *hip_stream) {
    const Centre c{nullptr, centre, true};
    const int rc = check_scaled_plain(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return state_device(cfg, y0, y1, from, d_z, d_iters, d_w, d_m, hip_stream, "SCALED PT", "w", scaled_state_rows(cfg, c, y0, y1, from));
}

int scaled_state_host(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, const uint32_t *from, double *z,
                      uint32_t *iters, double *w, uint32_t *m) {
    const Centre c{nullptr, centre, true};
    const int rc = check_scaled_plain(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return state_host(cfg, y0, y1, from, z, iters, w, m, "SCALED PT", "w", scaled_state_rows(cfg, c, y0, y1, from));
}

}  // namespace

/* the road's check and RGB row launch for the supersampled form (fr_ss.hip), which bands the rows itself */
int scaled_check(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1) { return check_scaled(cfg, c, bits, y0, y1); }
int scaled_render_rows(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, unsigned channels,
                       const fr_kout &out, hipStream_t stream) {
    return scaled_rows(cfg, c, bits, y0, y1, channels, FR_OUT_RGB)(ctx, out, stream);
}

/* fr_ss_list.h: ADAPTIVE SUPERSAMPLING on SCALED PT — the probe (the road's RGB kernel over the strided map) and the refine pass */
int scaled_render_map(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_map &map, const fr_kout &out, hipStream_t stream) {
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    map.apply(p);
    return launch_scaled(ctx, cfg, c, bits, p, FR_OUT_RGB, out, stream);
}

int scaled_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, uint32_t groups, hipStream_t stream) {
    const ScaledConsts k = scaled_consts(cfg);
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    p.scale_re = k.sre;
    p.scale_im = k.sim;
    std::shared_ptr<PtOrbit> orbit;
    std::shared_ptr<BlaTable> table;
    ScaledDev t;
    const int rc = scaled_dev_fill(ctx, cfg, c, bits, k, orbit, table, t);
    if (rc != FR_OK) return rc;
    const dim3 grid(groups), block(kSsRefineThreads);
    const bool julia = cfg->algo == 2;
    if (bits >= 0)
        ss_refine_instance(julia, a.linear, [&](auto J, auto L) { ss_refine_scaled_kernel<J(), true, L()><<<grid, block, 0, stream>>>(p, a, t); });
    else
        ss_refine_instance(julia, a.linear, [&](auto J, auto L) { ss_refine_scaled_kernel<J(), false, L()><<<grid, block, 0, stream>>>(p, a, t); });
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

}  // namespace fr

using namespace fr;

int fr_render_rows_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1,
                                    int channels, void *d_out, size_t out_len, void *hip_stream) {
    const Centre c{nullptr, centre, true};
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = check_scaled(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return rgb_rows_device(cfg, y0, y1, channels, d_out, out_len, hip_stream, scaled_rows(cfg, c, bits, y0, y1, (unsigned)channels, FR_OUT_RGB));
}

int fr_render_rows_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, int channels,
                             uint8_t *out, size_t out_len) {
    const Centre c{nullptr, centre, true};
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = check_scaled(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return rgb_rows_host(cfg, y0, y1, channels, out, out_len, scaled_rows(cfg, c, bits, y0, y1, (unsigned)channels, FR_OUT_RGB));
}

int fr_escape_rows_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, void *d_z,
                                    void *d_iters, void *hip_stream) {
    const Centre c{nullptr, centre, true};
    const int rc = check_scaled(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return raw_rows_device(cfg, y0, y1, d_z, d_iters, hip_stream, scaled_rows(cfg, c, bits, y0, y1, 0, FR_OUT_ESCAPE));
}

int fr_escape_rows_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, double *z,
                             uint32_t *iters) {
    const Centre c{nullptr, centre, true};
    const int rc = check_scaled(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return raw_rows_host(cfg, y0, y1, z, iters, 2, scaled_rows(cfg, c, bits, y0, y1, 0, FR_OUT_ESCAPE));
}

int fr_debug_pt_scaled_count(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, uint64_t *passes,
                             uint64_t *steps) {
    const Centre c{nullptr, centre, true};
    const int rc = check_scaled(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    if (!passes || !steps) return fail(FR_ERR_INVALID_ARGUMENT, "passes or steps is NULL");
    *passes = *steps = 0;
    if ((size_t)cfg->width * (size_t)(y1 - y0) == 0) return FR_OK;
    uint64_t *const sums[2] = {passes, steps};
    return count_rows(sums, scaled_rows(cfg, c, bits, y0, y1, 0, FR_OUT_COUNT));
}

int fr_debug_bla_table_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, int which, uint32_t level, double *out,
                              size_t cap, uint32_t *len) {
    const Centre c{nullptr, centre, true};
    const int rc = check_scaled(cfg, c, bits, 0, 0, true);
    if (rc != FR_OK) return rc;
    return bla_debug_table(cfg, c, bits, true, which, level, out, cap, len);
}

/* ---- the calls of the resumable state (the plain loop's: no bits) -------------------------------------------------------- */

int fr_escape_rows_pt_scaled_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                          void *d_iters, void *d_w, void *d_m, void *hip_stream) {
    return scaled_state_device(cfg, centre, y0, y1, nullptr, d_z, d_iters, d_w, d_m, hip_stream);
}

int fr_escape_extend_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                      uint32_t from_iterations, void *d_z, void *d_iters, void *d_w, void *d_m, void *hip_stream) {
    return scaled_state_device(cfg, centre, y0, y1, &from_iterations, d_z, d_iters, d_w, d_m, hip_stream);
}

int fr_escape_rows_pt_scaled_state(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                                   uint32_t *iters, double *w, uint32_t *m) {
    return scaled_state_host(cfg, centre, y0, y1, nullptr, z, iters, w, m);
}

int fr_escape_extend_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                               double *z, uint32_t *iters, double *w, uint32_t *m) {
    return scaled_state_host(cfg, centre, y0, y1, &from_iterations, z, iters, w, m);
}
