/*
 * fr_ss_adaptive_de.hip — ADAPTIVE SUPERSAMPLED DE (include/fractal_hip.h): the distance-shaded s x s samples only at edge pixels
 * and at pixels whose probe lies closer to the set than the caller's reach.  ADAPTIVE SUPERSAMPLING (fr_ss_adaptive.hip) with the
 * DE roads underneath and one more reason to refine: the probe's own exterior distance D says how far the set is, so a pixel
 * with D < R * s is refined whatever its neighbours look like.  Four passes on the caller's stream, no host read between them:
 *   1. the DE probe: the road's EXISTING DE kernel on cfg_s over the strided pixel map (x_first = p, x_stride = s,
 *      y_first = s ya + p, y_stride = s, block_rows = 1), rows [ya, yb) = [max(y0 - 1, 0), min(y1 + 1, height)), into the
 *      workspace's z, der and iters: the full render's samples by construction (fr_ss_list.h: de_render_map over the road's launch);
 *   2. the probe colours: colour_de_rows_kernel (fr_de.h: fr_launch_colour_de_rows) over those arrays with cfg_s's pixels and the
 *      thickness T * s, into the workspace's colour area;
 *   3. ss_mark_de_kernel: ss_mark_kernel's tile and pieces (fr_ss_list.h) plus `near` from the lane's OWN (z, iters, der) through
 *      de_distance (fr_de_shade.h), the log2 table staged in LDS when the reach is not 0.  Writes P into d_out and appends the
 *      edge pixels to the list: one ballot and one atomic per wave;
 *   4. ss_refine_de_*_kernel<JULIA>, one per road, beside the road's DE loop (fr_de.hip, fr_de_bla.hip), through ss_refine_loop:
 *      F of the shaded samples over the probe bytes of the listed pixels.
 * `near` reads the pixel's own probe only, so a row piece needs the same one-row halo as the colour rule and no more.
 * The entry points: fr_ss_adaptive_de_workspace_bytes, fr_render_rows_ss_adaptive_de_device and fr_render_rows_ss_adaptive_de (the
 * same into a host buffer through context scratch, by row pieces above the host workspace cap).  fr_debug_ss_adaptive_grid
 * (fr_ss_adaptive.hip) sets the refine grid here too.  Each call is its domain check (ssad_check) and fr_ss_adaptive.h's skeleton
 * around ssad_render; the workspace's layout is that header's, with the DE arrays in front ("3.32").
 *
 * ADAPTIVE SUPERSAMPLED SCALED DE (include/fractal_hip.h): fr_render_rows_ss_adaptive_de_pt_scaled and its three other spellings,
 * the road that the calls above keep refusing.  Their own check (ssad_scaled_check: DE ON SCALED PT's domain on cfg_s, `pixels` from
 * the scaled view) and the scaled arm of ssad_render's two switches — the probe is de_render_map over scaled_de_launch, the refine pass
 * ss_refine_de_scaled_kernel (fr_de_scaled.hip); passes 2 and 3 run unchanged, the scaled view enters through `pixels` alone.
 */
#include "fr_bla.h" /* scaled_consts */
#include "fr_ctx.h"
#include "fr_de.h"
#include "fr_math.h"
#include "fr_ss_adaptive.h"
#include "fr_ss_list.h"

namespace {

#include "fr_colour.h"   /* the log2 table */
#include "fr_de_shade.h" /* de_distance */

struct ssmd_params {
    const uint8_t *probe;          /* probe colours of image rows [ya, yb), packed r,g,b */
    const double *z, *der;         /* the probe's DE arrays of the same rows: re, im per pixel */
    const uint32_t *iters;
    uint8_t *out;                  /* rows [y0, y0 + rows) of the output */
    uint32_t *list;
    unsigned long long *counters;  /* [0] the count */
    uint32_t width;                /* of the output */
    uint32_t ya, yb;               /* max(y0 - 1, 0), min(y1 + 1, height): rows outside are outside the IMAGE */
    uint32_t y0, rows;
    uint32_t tiles_x;
    uint32_t bpp;
    int tau;                       /* -1: every pixel is an edge; 255: the colour rule marks none */
    uint32_t iterations;
    double pixels;                 /* (double)(s * height) * min(|scale.re|, |scale.im|): the last factor of D on cfg_s */
    double rs;                     /* R * s in sample pixels; 0: `near` holds nowhere */
};

/* ss_mark_kernel (fr_ss_adaptive.hip) with the distance rule: edge = t < 0, or the neighbour rule on P, or near — the probe
 * escaped (iters < iterations) and its D lies under Rs.  de_distance gives 0 for an overflowed derivative (NaN and negatives
 * give 0), which is under every Rs > 0; a capped probe is never near. */
__global__ __launch_bounds__(kMarkThreads) void ss_mark_de_kernel(const ssmd_params q) {
    __shared__ uint32_t s_p[kMarkHalo];
    __shared__ double s_tab[FR_LOG2_N * 3];
    const uint32_t tid = threadIdx.x;
    const uint32_t ty = blockIdx.x / q.tiles_x, tx = blockIdx.x - ty * q.tiles_x;
    const uint32_t X0 = tx * kMarkW, R0 = ty * kMarkH;
    const bool reach = q.rs > 0.0; /* uniform */
    if (reach) {
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += kMarkThreads) s_tab[k] = gt[k];
    }
    ss_mark_stage(s_p, q.probe, q.width, q.ya, q.yb, q.y0, X0, R0, tid);
    __syncthreads();

    const uint32_t lx = tid % kMarkW, ly = tid / kMarkW;
    const uint32_t X = X0 + lx, row = R0 + ly;
    const bool valid = X < q.width && row < q.rows;
    const uint32_t *at = s_p + (ly + 1u) * kMarkPitch + lx + 1u;
    bool edge = false;
    if (valid) {
        edge = q.tau < 0 || ss_mark_neighbours(at, q.tau);
        if (!edge && reach) {
            const uint64_t k = (uint64_t)(q.y0 - q.ya + row) * q.width + X; /* the pixel's own probe */
            const uint32_t it = q.iters[k];
            if (it < q.iterations)
                edge = de_distance(q.z[2 * k], q.z[2 * k + 1], q.der[2 * k], q.der[2 * k + 1], it, q.iterations, q.pixels, s_tab) < q.rs;
        }
        ss_mark_write(q.out, q.bpp, (uint64_t)row * q.width + X, at[0]);
    }
    ss_mark_append(edge, row * q.width + X, q.list, q.counters, tid);
}

}  // namespace

namespace fr {
namespace {

/* what the calls have checked: the plan of cfg_s, the road with its centre and resolved bits, the shade and the rules */
struct SsadRoad {
    SsPlan pl;
    Centre c;
    int precision, road, bits;
    int tau;
    double ts, rs, pixels;
};

/* the head of both checks below: the sizes, the channels, the thickness, the reach, the threshold and the list's 32-bit indices */
int ssad_head(const fr_config *cfg, double thickness, uint32_t s, int threshold, double reach, uint32_t y0, uint32_t y1, int channels,
              SsadRoad &r) {
    int rc = ss_plan(cfg, s, y0, y1, r.pl);
    if (rc == FR_OK) rc = check_channels(channels);
    if (rc != FR_OK) return rc;
    rc = ss_de_thickness(thickness, s, r.ts);
    if (rc != FR_OK) return rc;
    r.rs = reach * (double)s;
    if (!(reach >= 0.0 && r.rs <= 0x1p20))
        return fail(FR_ERR_INVALID_ARGUMENT, "reach must be finite with 0 <= reach * supersample <= 2^20 (output pixels; 0 = the colour rule alone)");
    if (threshold < -1 || threshold > 255)
        return fail(FR_ERR_INVALID_ARGUMENT, "threshold must be -1 (every pixel is refined) or 0 .. 255");
    if ((uint64_t)cfg->width * (y1 - y0) > 0xFFFFFFFFull)
        return fail(FR_ERR_INVALID_ARGUMENT, "width * (y1 - y0) must be below 2^32: the edge list holds 32-bit pixel indices; call by row pieces");
    r.tau = threshold;
    return FR_OK;
}

/* everything the calls check before any device work, short of the buffers: the sizes, the thickness, the reach, the threshold,
 * then fr_render_rows_ss_de_device's argument rule per precision and road with the road's own DE domain on cfg_s */
int ssad_check(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
               double thickness, uint32_t s, int threshold, double reach, uint32_t y0, uint32_t y1, int channels, SsadRoad &r) {
    const int rc = ssad_head(cfg, thickness, s, threshold, reach, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    const fr_config *cs = &r.pl.cfg_s;
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + r.pl.src_rows);
    r.pixels = ss_de_pixels(cfg, s);
    r.precision = precision;
    r.road = road;
    r.bits = bits;
    r.c = Centre{pos_lo, centre};
    if (road == FR_PT_ROAD_SCALED)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PT_ROAD_SCALED: distance estimation on SCALED PT is out of scope; adaptive supersampled DE takes "
                                             "FR_PRECISION_F64, FR_PRECISION_PT (dd or wide centre) and BLA-PT");
    if (precision == FR_PRECISION_F32)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_F32 is out of scope of adaptive supersampled DE: precision must be FR_PRECISION_F64 or FR_PRECISION_PT");
    if (precision == FR_PRECISION_DD)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_DD is out of scope of adaptive supersampled DE: precision must be FR_PRECISION_F64 or FR_PRECISION_PT");
    if (precision != FR_PRECISION_F64 && precision != FR_PRECISION_PT)
        return fail(FR_ERR_INVALID_ARGUMENT, "precision must be FR_PRECISION_F64 or FR_PRECISION_PT");
    if (road != FR_PT_ROAD_PLAIN && road != FR_PT_ROAD_BLA)
        return fail(FR_ERR_INVALID_ARGUMENT, "road must be FR_PT_ROAD_PLAIN (0) or FR_PT_ROAD_BLA (1)");
    if (centre && pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "pos_lo must be NULL when a wide centre is given");
    if (precision == FR_PRECISION_F64) {
        if (road != FR_PT_ROAD_PLAIN) return fail(FR_ERR_INVALID_ARGUMENT, "road: FR_PT_ROAD_BLA needs FR_PRECISION_PT, the F64 road has no table");
        if (centre) return fail(FR_ERR_INVALID_ARGUMENT, "centre: a wide centre is for FR_PRECISION_PT only; the F64 road takes none");
    }
    if (road == FR_PT_ROAD_BLA) return bla_de_domain(cs, r.c, r.bits, Y0, Y1);
    if (bits != 0) return fail(FR_ERR_INVALID_ARGUMENT, "bits must be 0 with FR_PT_ROAD_PLAIN: the plain loop has no table");
    return de_domain(cs, precision, r.c, precision == FR_PRECISION_PT && centre != nullptr, Y0, Y1);
}

/* ADAPTIVE SUPERSAMPLED SCALED DE: the sizes, the thickness, the reach and the threshold as ssad_check takes them, then DE ON SCALED
 * PT's domain on cfg_s by the code its plain calls run, and `pixels` — the last factor of D on the scaled view of cfg_s — as
 * ss_de_scaled_check (fr_ss_de.hip) computes it */
int ssad_scaled_check(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t s, int threshold, double reach,
                      uint32_t y0, uint32_t y1, int channels, SsadRoad &r) {
    int rc = ssad_head(cfg, thickness, s, threshold, reach, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    r.precision = FR_PRECISION_PT;
    r.road = FR_PT_ROAD_SCALED;
    r.bits = bits;
    r.c = Centre{nullptr, centre, true};
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + r.pl.src_rows);
    rc = scaled_de_domain(&r.pl.cfg_s, r.c, r.bits, Y0, Y1);
    if (rc != FR_OK) return rc;
    const ScaledConsts k = scaled_consts(cfg); /* cfg_s shares cfg's scale */
    r.pixels = ss_de_pixels(cfg, s, k.sre, k.sim);
    return FR_OK;
}

/* Rows [y0, y1) of the adaptive DE render into d_out on `stream`: the four passes.  Arguments checked, the rows and the width not
 * empty, d_work holds ss_adaptive_layout's bytes.  No host synchronisation (PT roads: apart from computing and uploading the view's
 * orbit and table when the context does not hold them yet), no allocation; the count stays in the workspace's first counter. */
int ssad_render(Ctx &ctx, const SsadRoad &r, const fr_config *cfg, uint32_t s, int transfer, uint32_t y0, uint32_t y1, unsigned bpp, void *d_out,
                void *d_work, hipStream_t stream) {
    const fr_config *cs = &r.pl.cfg_s;
    const SsAdaptiveLayout l = ss_adaptive_layout(cfg, y0, y1, true);
    char *const base = static_cast<char *>(d_work);
    double *const d_z = reinterpret_cast<double *>(base), *const d_der = reinterpret_cast<double *>(base + l.der_off);
    uint32_t *const d_iters = reinterpret_cast<uint32_t *>(base + l.iters_off);
    uint8_t *const probe = reinterpret_cast<uint8_t *>(base + l.colour_off);
    uint32_t *const list = reinterpret_cast<uint32_t *>(base + l.list_off);
    unsigned long long *const counters = reinterpret_cast<unsigned long long *>(base + l.counters_off);
    const bool escape_algo = cfg->algo == FR_ALGO_MANDELBROT || cfg->algo == FR_ALGO_JULIA;
    const size_t n = (size_t)cfg->width * (l.yb - l.ya);
    int rc = prof_begin(stream);
    if (rc != FR_OK) return rc;
    HIP_TRY(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), stream));

    /* 1. the DE probe */
    const uint32_t half = s / 2u;
    const fr_ss_map map{cfg->width, l.yb - l.ya, half, s, s * l.ya + half, s};
    if (r.road == FR_PT_ROAD_SCALED)
        rc = de_render_map(ctx, cs, map, d_z, d_iters, d_der, stream, de_road(scaled_de_launch, cs, r.c, r.bits));
    else if (r.road == FR_PT_ROAD_BLA)
        rc = de_render_map(ctx, cs, map, d_z, d_iters, d_der, stream, de_road(bla_de_launch, cs, r.c, r.bits));
    else
        rc = de_render_map(ctx, cs, map, d_z, d_iters, d_der, stream, de_road(de_launch, cs, r.precision, r.c));
    if (rc != FR_OK) return rc;

    /* 2. the probe colours, shaded as the samples of cfg_s are */
    fr_kparams p;
    fill_params(cs, default_opts(), p);
    HIP_TRY(fr_launch_colour_de_rows(p, d_z, d_iters, d_der, n, r.pixels, r.ts, 3u, probe, stream));

    /* 3. P into d_out, the edge pixels into the list; an algorithm without orbits has none */
    ssmd_params q;
    q.probe = probe;
    q.z = d_z;
    q.der = d_der;
    q.iters = d_iters;
    q.out = static_cast<uint8_t *>(d_out);
    q.list = list;
    q.counters = counters;
    q.width = cfg->width;
    q.ya = l.ya;
    q.yb = l.yb;
    q.y0 = y0;
    q.rows = y1 - y0;
    q.tiles_x = (uint32_t)(((uint64_t)cfg->width + kMarkW - 1) / kMarkW);
    q.bpp = bpp;
    q.tau = escape_algo ? r.tau : 255;
    q.iterations = cfg->iterations;
    q.pixels = r.pixels;
    q.rs = escape_algo ? r.rs : 0.0;
    const uint64_t tiles = (uint64_t)q.tiles_x * (((uint64_t)q.rows + kMarkH - 1) / kMarkH);
    if (tiles > 0x7FFFFFFFull) return fail(FR_ERR_INVALID_ARGUMENT, "the row range holds too many tiles for one launch; call by row pieces");
    ss_mark_de_kernel<<<dim3((uint32_t)tiles), dim3(kMarkThreads), 0, stream>>>(q);
    HIP_TRY(hipGetLastError());

    /* 4. F over the probe bytes of the listed pixels; s = 1: F = P already; threshold 255 and reach 0: the list is empty */
    const char *kname = "ss_mark_de_kernel";
    if (s > 1 && escape_algo && (q.tau < 255 || q.rs > 0.0)) {
        const fr_ss_refine a = ss_refine_args(q.out, list, counters, cfg->width, y0, s, bpp, transfer);
        const uint32_t groups = ss_refine_groups(a, q.rows);
        const fr_ss_de_shade sh{r.pixels, r.ts};
        if (r.road == FR_PT_ROAD_SCALED) {
            rc = scaled_de_ss_refine(ctx, cs, r.c, r.bits, a, sh, groups, stream);
            kname = "ss_refine_de_scaled_kernel";
        } else if (r.road == FR_PT_ROAD_BLA) {
            rc = bla_de_ss_refine(ctx, cs, r.c, r.bits, a, sh, groups, stream);
            kname = "ss_refine_de_bla_kernel";
        } else {
            rc = de_ss_refine(ctx, cs, r.precision, r.c, a, sh, groups, stream);
            kname = r.precision == FR_PRECISION_PT ? "ss_refine_de_pt_kernel" : "ss_refine_de_f64_kernel";
        }
        if (rc != FR_OK) return rc;
    }
    return prof_end(stream, kname);
}

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

int fr_ss_adaptive_de_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *bytes) {
    return ss_adaptive_workspace_bytes(cfg, supersample, y0, y1, true, bytes);
}

int fr_render_rows_ss_adaptive_de_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                         int road, int bits, double thickness, uint32_t supersample, int transfer, int threshold, double reach,
                                         uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work, size_t work_len,
                                         void *d_refined, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsadRoad r;
    const int rc = ssad_check(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, threshold, reach, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_adaptive_device(cfg, true, "work_len < bytes of fr_ss_adaptive_de_workspace_bytes",
                              "d_work must be 8-byte aligned (z, der, the list and the counters lie in it)", y0, y1, channels, d_out, out_len, d_work,
                              work_len, d_refined, hip_stream, [&](Ctx &ctx, uint32_t ya, uint32_t yb, void *dst, void *work, hipStream_t stream) {
                                  return ssad_render(ctx, r, cfg, supersample, transfer, ya, yb, (unsigned)channels, dst, work, stream);
                              });
}

int fr_render_rows_ss_adaptive_de_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                         int road, int bits, double thickness, uint32_t supersample, int threshold, double reach,
                                         uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work, size_t work_len,
                                         void *d_refined, void *hip_stream) {
    return fr_render_rows_ss_adaptive_de_tf_device(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, threshold, reach, y0, y1, channels, d_out, out_len, d_work, work_len, d_refined, hip_stream);
}

int fr_render_rows_ss_adaptive_de_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                  int bits, double thickness, uint32_t supersample, int transfer, int threshold, double reach, uint32_t y0, uint32_t y1,
                                  int channels, uint8_t *out, size_t out_len, uint64_t *refined) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsadRoad r;
    const int rc = ssad_check(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, threshold, reach, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_adaptive_host(cfg, true, y0, y1, channels, out, out_len, refined,
                            [&](Ctx &ctx, uint32_t ya, uint32_t yb, void *dst, void *work, hipStream_t stream) {
                                return ssad_render(ctx, r, cfg, supersample, transfer, ya, yb, (unsigned)channels, dst, work, stream);
                            });
}

int fr_render_rows_ss_adaptive_de(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                  int bits, double thickness, uint32_t supersample, int threshold, double reach, uint32_t y0, uint32_t y1,
                                  int channels, uint8_t *out, size_t out_len, uint64_t *refined) {
    return fr_render_rows_ss_adaptive_de_tf(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, threshold, reach, y0, y1, channels, out, out_len, refined);
}

/* ---- ADAPTIVE SUPERSAMPLED SCALED DE: the four calls above on the scaled road, which they keep refusing ------------------------- */

int fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                                      uint32_t supersample, int transfer, int threshold, double reach, uint32_t y0, uint32_t y1,
                                                      int channels, void *d_out, size_t out_len, void *d_work, size_t work_len, void *d_refined,
                                                      void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsadRoad r;
    const int rc = ssad_scaled_check(cfg, centre, bits, thickness, supersample, threshold, reach, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_adaptive_device(cfg, true, "work_len < bytes of fr_ss_adaptive_de_workspace_bytes",
                              "d_work must be 8-byte aligned (z, der, the list and the counters lie in it)", y0, y1, channels, d_out, out_len, d_work,
                              work_len, d_refined, hip_stream, [&](Ctx &ctx, uint32_t ya, uint32_t yb, void *dst, void *work, hipStream_t stream) {
                                  return ssad_render(ctx, r, cfg, supersample, transfer, ya, yb, (unsigned)channels, dst, work, stream);
                              });
}

int fr_render_rows_ss_adaptive_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                                   uint32_t supersample, int threshold, double reach, uint32_t y0, uint32_t y1, int channels,
                                                   void *d_out, size_t out_len, void *d_work, size_t work_len, void *d_refined, void *hip_stream) {
    return fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(cfg, centre, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, threshold, reach, y0, y1, channels, d_out, out_len, d_work, work_len, d_refined, hip_stream);
}

int fr_render_rows_ss_adaptive_de_pt_scaled_tf(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample,
                                               int transfer, int threshold, double reach, uint32_t y0, uint32_t y1, int channels, uint8_t *out,
                                               size_t out_len, uint64_t *refined) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsadRoad r;
    const int rc = ssad_scaled_check(cfg, centre, bits, thickness, supersample, threshold, reach, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_adaptive_host(cfg, true, y0, y1, channels, out, out_len, refined,
                            [&](Ctx &ctx, uint32_t ya, uint32_t yb, void *dst, void *work, hipStream_t stream) {
                                return ssad_render(ctx, r, cfg, supersample, transfer, ya, yb, (unsigned)channels, dst, work, stream);
                            });
}

int fr_render_rows_ss_adaptive_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample,
                                            int threshold, double reach, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len,
                                            uint64_t *refined) {
    return fr_render_rows_ss_adaptive_de_pt_scaled_tf(cfg, centre, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, threshold, reach, y0, y1, channels, out, out_len, refined);
}

} /* extern "C" */
