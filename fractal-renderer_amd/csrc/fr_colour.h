/*
 * fr_colour.h — the colour map (calc/src/lib.rs:214-234 + color_multiply) as the kernels evaluate it: the software
 * log2's table, ColourConsts, and colour_of / colour_pixel with the colour filter.  Device code only; included inside
 * the anonymous namespace of every translation unit that renders (fr_kernels.hip, fr_dd.hip), so each code object
 * carries its own copy.  Needs fr_kernels.h and fr_math.h first.
 */
#ifndef FR_COLOUR_H
#define FR_COLOUR_H

__device__ const double g_log2_tab[FR_LOG2_N][3] = FR_LOG2_TABLE_INIT;

/* ---- colour map: calc/src/lib.rs:214-234 -------------------------------------------------- */

struct ColourConsts {
    double stable_limit, exposure;
    double iterations_f64; /* config.iterations as f64 */
    double inv_iterations; /* exact reciprocal when iterations is a power of two, else 0 */
    uint32_t inside, smooth;
    double prim[3], sec[3]; /* stored r, g, b fields as f64 */
    uint32_t filter;        /* smooth colouring: try the f32 bracket first (see colour_outside_filtered) */
    double filt_k;          /* exposure / iterations, any rounding */
    double filt_d[3];       /* prim[k] * |filt_k| * FR_NU_BRACKET * (1 + 2^-20): the bracket's half-width in byte units */
    uint32_t filter32;      /* ... and before that, the same test carried out in f32 */
    float filt_k32, filt_d32[3], prim32[3];
    float filt_lo32;        /* f32 renders: an f32 squared distance at or above this is surely > stable_limit and >= 2 */
};

template <typename P>
__device__ __forceinline__ ColourConsts make_colour_consts(const P &p) {
    ColourConsts c;
    c.stable_limit = p.stable_limit;
    c.exposure = p.exposure;
    c.iterations_f64 = p.iterations_f64;
    c.inv_iterations = p.inv_iterations;
    c.inside = p.inside;
    c.smooth = p.smooth;
    for (int k = 0; k < 3; k++) {
        c.prim[k] = p.prim_f[k];
        c.sec[k] = p.sec_f[k];
        c.filt_d[k] = p.filt_d[k];
    }
    c.filter = p.colour_filter;
    c.filt_k = p.filt_k;
    c.filter32 = p.colour_filter32;
    c.filt_k32 = p.filt_k32;
    for (int k = 0; k < 3; k++) {
        c.filt_d32[k] = p.filt_d32[k];
        c.prim32[k] = p.prim32[k];
    }
    c.filt_lo32 = p.filt_lo32;
    return c;
}

/* Rust's `f64 as u8` (truncate, saturate, NaN -> 0) in two instructions: v_cvt_u32_f64 truncates
 * toward zero, saturates out-of-range inputs (negative -> 0, huge / +inf -> 0xFFFFFFFF) and maps
 * NaN to 0; the min brings it to u8 range.  (Inline asm because a plain C cast of an out-of-range
 * value is undefined behaviour to the optimiser.)  Checked against the host's fr_sat_u8 by
 * test_device_saturating_cast. */
__device__ __forceinline__ uint32_t sat_u8_dev(double v) {
    uint32_t u;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(u) : "v"(v));
    return u < 255u ? u : 255u;
}

__device__ __forceinline__ uint32_t sat_u8_dev(float v) { /* the same, from an f32 */
    uint32_t u;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(u) : "v"(v));
    return u < 255u ? u : 255u;
}

/* The same cast, from an f32, written straight into byte `k` of a packed word: v_floor_f32 + v_cvt_pk_u8_f32.
 * The pack instruction rounds to nearest even and saturates (NaN -> 0); behind a floor that is truncation for
 * every value that does not saturate to 0 anyway.  Equal to sat_u8_dev(float) on EVERY f32 bit pattern
 * (tools/ubench/cvt_pk_u8.hip scans them all; test_device_packed_saturating_cast does the same through the
 * library).  Two half-cost instructions instead of a convert and a full-cost integer min, and the three bytes
 * of a pixel arrive packed. */
template <int K>
__device__ __forceinline__ uint32_t sat_u8_pack(float v, uint32_t acc) {
    /* the compiler's own v_floor_f32 / v_cvt_pk_u8_f32 (inline asm here drew an s_nop before every dependent use) */
    return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_floorf(v), (uint32_t)K, acc);
}

__device__ __forceinline__ void colour_multiply(const double col[3], double mult, uint8_t out[3]) {
    out[0] = (uint8_t)sat_u8_dev(col[0] * mult);
    out[1] = (uint8_t)sat_u8_dev(col[2] * mult);
    out[2] = (uint8_t)sat_u8_dev(col[1] * mult);
}

/* outside colouring without the smooth term: a function of the escape index alone */
__device__ __forceinline__ void colour_outside_flat(const ColourConsts &c, uint32_t iters_u, uint8_t out[3]) {
    const double iters = (double)iters_u;
    const double q = (c.inv_iterations != 0.0) ? iters * c.inv_iterations : iters / c.iterations_f64;
    colour_multiply(c.prim, q * c.exposure, out); /* :228-229 */
}

/* Smooth colouring without the two f64 software log2s, when that is provably the same bytes.
 *
 * The reference computes (calc/src/lib.rs:222-229)
 *     nu   = log2(log2(sqrt(dist)) / 2)                  [= log2(log2(dist) / 4) over the reals]
 *     byte = (col * ((iters + 1 - nu) / iterations * exposure)) as u8
 * and every step after nu is monotone in nu (IEEE add, mul and div by a positive constant are monotone,
 * so is the truncating cast).  So if nu is known to lie in [a - E, a + E] and the value col * (...) taken
 * at a, widened by what E and the roundings can move it, stays strictly inside one integer cell, the byte
 * is decided without knowing nu any better.
 *
 * a comes from the hardware's f32 log2 (v_log_f32, twice: 2 + 2 VALU slots instead of ~110 f64
 * instructions).  Error budget on a, for 2 <= dist <= 2^120 (L = log2(dist) in [1, 120]):
 *     dist -> f32                 relative 2^-24, i.e. 8.6e-8 absolute on L
 *     v_log_f32                   <= 1 ulp of L (2^-23 relative)            [measured: fr_debug_math(4)]
 *     second v_log_f32            relative error of L times 1/ln 2, + 1 ulp of |nu| < 8 (4.8e-7)
 *     the f64 path's own nu       differs from the real nu by < 1e-14
 * total < 1e-6; the bracket used is FR_NU_BRACKET = 2^-18 = 3.8e-6 (fr_kernels.h; applied by the host in filt_d).  test_gpu_parity.py scans EVERY f32 in
 * [2, 2^120] on the device and asserts the composite error of a stays under 1.5e-6.
 * Pixels outside that range of dist, and pixels whose widened value touches a cell boundary (about one in
 * 10^5), take the exact path.  Same bytes either way; fr_set_colour_filter(0) forces the exact path. */
/* Stage 1, all in f32 (instructions at half the f64 cost), from an f32 squared distance d32:
 * v32 = col * ((iters + 1 - nu32) * K32).  Four f32 roundings and K's own put it within |v| * 2.4e-7 of
 * col * (iters + 1 - nu32) * K, which is within col * |K| * E of the real value (nu is within E of nu32); the
 * window used is |v32| * 2^-21 + filt_d32 (the host rounds that term up), twice the relative part, so that the
 * roundings of the window's own ends are covered too.  (iterations < 2^24 and 2^-60 <= |K| <= 2^60 — the host
 * checks — keep every step exact enough: iters + 1 converts exactly, nothing under- or overflows.)  Both ends of
 * the window are cast into packed bytes, so one comparison decides all three channels.  Returns, per lane,
 * whether the byte triple is decided (and then out[] holds it). */
/* itp1 = (float)(iters + 1), exact (iterations < 2^24); `lo` = the bytes r | g << 8 | b << 16 when decided */
__device__ __forceinline__ bool colour_filter_stage1_packed(const ColourConsts &c, float d32, float itp1, float &nu32,
                                                            uint32_t &lo) {
    const float l1 = __builtin_amdgcn_logf(d32);
    nu32 = __builtin_amdgcn_logf(l1 * 0.25f);
    const int ch[3] = {0, 2, 1}; /* color_multiply's RGB::new(r, b, g) swap, as in colour_multiply() */
    const float m32 = (itp1 - nu32) * c.filt_k32;
    const float v0 = c.prim32[ch[0]] * m32, v1 = c.prim32[ch[1]] * m32, v2 = c.prim32[ch[2]] * m32;
    const float w0 = __builtin_fmaf(__builtin_fabsf(v0), 0x1p-21f, c.filt_d32[ch[0]]);
    const float w1 = __builtin_fmaf(__builtin_fabsf(v1), 0x1p-21f, c.filt_d32[ch[1]]);
    const float w2 = __builtin_fmaf(__builtin_fabsf(v2), 0x1p-21f, c.filt_d32[ch[2]]);
    lo = sat_u8_pack<2>(v2 - w2, sat_u8_pack<1>(v1 - w1, sat_u8_pack<0>(v0 - w0, 0u)));
    const uint32_t hi = sat_u8_pack<2>(v2 + w2, sat_u8_pack<1>(v1 + w1, sat_u8_pack<0>(v0 + w0, 0u)));
    return lo == hi;
}
__device__ __forceinline__ bool colour_filter_stage1(const ColourConsts &c, float d32, bool in_range, uint32_t iters_u,
                                                     float &nu32, uint8_t out[3]) {
    uint32_t lo;
    const bool same = colour_filter_stage1_packed(c, d32, (float)(iters_u + 1u), nu32, lo);
    out[0] = (uint8_t)lo, out[1] = (uint8_t)(lo >> 8), out[2] = (uint8_t)(lo >> 16);
    return in_range && same;
}

__device__ __forceinline__ bool colour_outside_filtered(const ColourConsts &c, double dist, uint32_t iters_u, uint8_t out[3]) {
    const bool in_range = dist >= 2.0 && dist <= 0x1p120;
    const int ch[3] = {0, 2, 1};
    float nu32;
    /* A wave whose lanes all pass stage 1 is done; about one wave in fifty is not and goes on to stage 2. */
    if (c.filter32) {
        const bool same32 = colour_filter_stage1(c, (float)dist, in_range, iters_u, nu32, out);
        if (__ballot(!same32) == 0ull) return true;
    } else {
        nu32 = __builtin_amdgcn_logf(__builtin_amdgcn_logf((float)dist) * 0.25f);
    }
    /* Stage 2: the same test with the arithmetic after nu32 in f64 (window: |v| * 2^-46 + filt_d) */
    const double it2 = ((double)iters_u + 1.0) - (double)nu32; /* iters + 1 is exact */
    const double m = it2 * c.filt_k;
    bool same = in_range;
    for (int k = 0; k < 3; k++) {
        const double v = c.prim[ch[k]] * m;
        const double w = __builtin_fma(__builtin_fabs(v), 0x1p-46, c.filt_d[ch[k]]);
        const uint32_t lo = sat_u8_dev(v - w), hi = sat_u8_dev(v + w);
        same = same && lo == hi;
        out[k] = (uint8_t)lo;
    }
    return same;
}

/* `palette` (LDS) is non-NULL only when smooth == false: "LDS-staged palette lookup". */
__device__ __forceinline__ void colour_of(const ColourConsts &c, double dist, uint32_t iters_u,
                                          const double *lds_tab, const uint32_t *palette, uint8_t out[3]) {
    if (dist > c.stable_limit) { /* :216 */
        if (palette) {
            const uint32_t v = palette[iters_u];
            out[0] = (uint8_t)v;
            out[1] = (uint8_t)(v >> 8);
            out[2] = (uint8_t)(v >> 16);
        } else if (c.smooth) {
            bool exact = true;
            if (c.filter) exact = !colour_outside_filtered(c, dist, iters_u, out);
            /* the exact path is ~4x the filter: taken by the whole wave only when one of its lanes needs it */
            if (__ballot(exact) != 0ull && exact) {
                double iters = (double)iters_u;
                double log_zn = fr_log2_tab(__builtin_sqrt(dist), lds_tab) * 0.5; /* :222, x/2.0 == x*0.5 */
                double nu = fr_log2_tab(log_zn, lds_tab);                         /* :223 */
                iters += 1.0 - nu;                                                /* :225 */
                double q = (c.inv_iterations != 0.0) ? iters * c.inv_iterations : iters / c.iterations_f64;
                colour_multiply(c.prim, q * c.exposure, out); /* :228-229 */
            }
        } else {
            colour_outside_flat(c, iters_u, out);
        }
    } else if (c.inside) {
        colour_multiply(c.sec, dist, out); /* :231 */
    } else {
        out[0] = out[1] = out[2] = 0; /* :233 */
    }
}

/* The colour of the pixel recursive() left at (re, im) (r2 = re*re, i2 = im*im) after `iters_u`.
 *
 * f64 renders: dist = r2 + i2, the reference's squared_distance() (:214).  f32 renders: the reference's arithmetic
 * on the f32 position is zre*zre + zim*zim in f64 — two conversions, two multiplies, an add, and then three f64
 * compares and a conversion back before the filter's f32 stage can start: a third of the colour map's cost.  So
 * the f32 kernels first try with d32 = fl32(re*re + im*im), which is within 2^-23 (relative) of that f64 value:
 *   - d32 >= filt_lo32 (the host's max(stable_limit, 2) * (1 + 2^-20), rounded up) and d32 <= 2^120 (1 - 2^-20)
 *     PROVE dist > stable_limit and 2 <= dist <= 2^120, the branch and the range the filter needs;
 *   - as the logarithm's argument d32 moves nu by at most 2^-23 / (ln 2)^2 = 2.5e-7 on top of the 1.5e-6 the
 *     scan over every f32 allows (test_colour_filter_bracket_holds_for_every_f32): 1.75e-6, inside the bracket
 *     E = 2^-18 = 3.8e-6 the windows are built from.
 * A wave in which every lane passes both, and stage 1 decides every lane's bytes, never touches f64; any other
 * wave takes the general path below, which starts again from the f64 distance.  Same bytes either way. */
template <typename T>
__device__ __forceinline__ void colour_pixel(const ColourConsts &c, T re, T im, T r2, T i2, uint32_t iters_u,
                                             const double *lds_tab, const uint32_t *palette, uint8_t out[3]) {
    double dist;
    if constexpr (sizeof(T) == 8) {
        dist = (double)(r2 + i2);
    } else {
        if (c.filter32 && c.smooth && palette == nullptr) { /* wave-uniform */
            const float d32 = r2 + i2;
            const bool sure = d32 >= c.filt_lo32 && d32 <= 0x1.ffffep119f;
            if (__ballot(!sure) == 0ull) {
                float nu32;
                const bool decided = colour_filter_stage1(c, d32, true, iters_u, nu32, out);
                if (__ballot(!decided) == 0ull) return;
            }
        }
        const double zre = (double)re, zim = (double)im;
        dist = zre * zre + zim * zim;
    }
    colour_of(c, dist, iters_u, lds_tab, palette, out);
}

#endif
