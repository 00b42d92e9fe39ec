/*
 * fr_ss_adaptive.hip — ADAPTIVE SUPERSAMPLING (include/fractal_hip.h): the s x s samples only at edge pixels.  One sample per
 * output pixel — the probe, sample (p, p) of its block, p = floor(s / 2) — decides: a pixel whose probe differs from a
 * neighbour's by more than the threshold in some channel gets the box filter of all its samples, every other pixel keeps its
 * probe.  Three passes on the caller's stream, no host read between them:
 *   1. the probe pass: the road's EXISTING RGB kernel on cfg_s over the strided pixel map fr_kparams has (x_first = p,
 *      x_stride = s, y_first = s Ya + p, y_stride = s, block_rows = 1), rows [max(y0 - 1, 0), min(y1 + 1, height)) into the
 *      workspace: the bytes are the full render's samples by construction.  F64: ONE kernel choice, by name and size (no view
 *      sample: the call never blocks);
 *   2. ss_mark_kernel: one lane per output pixel, a 32 x 8 tile with its one-pixel halo in LDS as packed r | g << 8 | b << 16
 *      (~0: outside the image).  Writes P into d_out for every pixel of the rows (3 or 4 channels, 64-bit offsets) and appends
 *      the edge pixels to the list: one ballot and one atomic per wave;
 *   3. ss_refine_*_kernel<JULIA>, one per road, beside the road's loop (fr_pt.hip, fr_bla.hip, fr_scaled.hip; the F64 road's
 *      here: recursive() as written, escape_de_kernel's loop without the derivative): persistent waves claim
 *      ppw = floor(64 / s^2) list entries at a time (fr_ss_list.h: ss_refine_loop) and write F over the probe bytes.  The grid
 *      is fixed on the host — it fills the device, capped by the most work the rows can hold — and the count is read from
 *      device memory, which keeps the call asynchronous and balances the very uneven cost of edge pixels.
 * The entry points: fr_ss_adaptive_workspace_bytes, fr_render_rows_ss_adaptive_device, fr_render_rows_ss_adaptive (the same
 * into a host buffer through context scratch, by row pieces above the host workspace cap) and the test hook
 * fr_debug_ss_adaptive_grid.  Each call is its domain check (ssa_check) and fr_ss_adaptive.h's skeleton around ssa_render; the
 * workspace's layout is that header's too ("3.32").
 */
#include <algorithm>
#include <atomic>

#include "fr_bla.h"
#include "fr_math.h"
#include "fr_ss_adaptive.h"
#include "fr_ss_list.h"

namespace {

#include "fr_colour.h"

struct ssm_params {
    const uint8_t *probe;          /* probe colours of image rows [ya, yb), packed r,g,b */
    uint8_t *out;                  /* rows [y0, y0 + rows) of the output */
    uint32_t *list;
    unsigned long long *counters;  /* [0] the count */
    uint32_t width;                /* of the output */
    uint32_t ya, yb;               /* max(y0 - 1, 0), min(y1 + 1, height): rows outside are outside the IMAGE */
    uint32_t y0, rows;
    uint32_t tiles_x;
    uint32_t bpp;
    int tau;                       /* -1: every pixel is an edge; 255: none is */
};

__global__ __launch_bounds__(kMarkThreads) void ss_mark_kernel(const ssm_params q) {
    __shared__ uint32_t s_p[kMarkHalo];
    const uint32_t tid = threadIdx.x;
    const uint32_t ty = blockIdx.x / q.tiles_x, tx = blockIdx.x - ty * q.tiles_x;
    const uint32_t X0 = tx * kMarkW, R0 = ty * kMarkH;
    ss_mark_stage(s_p, q.probe, q.width, q.ya, q.yb, q.y0, X0, R0, tid);
    __syncthreads();

    const uint32_t lx = tid % kMarkW, ly = tid / kMarkW;
    const uint32_t X = X0 + lx, row = R0 + ly;
    const bool valid = X < q.width && row < q.rows;
    const uint32_t *at = s_p + (ly + 1u) * kMarkPitch + lx + 1u;
    bool edge = false;
    if (valid) {
        edge = q.tau < 0 || ss_mark_neighbours(at, q.tau);
        ss_mark_write(q.out, q.bpp, (uint64_t)row * q.width + X, at[0]);
    }
    ss_mark_append(edge, row * q.width + X, q.list, q.counters, tid);
}

/* The F64 road's refine pass (fr_ss_list.h: ss_refine_loop; fr_pt.hip: ss_refine_pt_kernel): each lane computes its sample's c
 * by coord_to_space on cfg_s (`p`) — the render kernels' operations on the same (x, y), hence the same bits — and runs
 * recursive() (calc/src/lib.rs:245-257) as written, escape_de_kernel's loop (fr_de.hip) without the derivative; the build has
 * -ffp-contract=off. */
template <bool JULIA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_f64_kernel(const fr_kparams p, const fr_ss_refine a) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kSsRefineThreads) s_tab[k] = gt[k];
    const uint16_t *const s_lt = ss_refine_tables<LINEAR>(); /* LINEAR-LIGHT SUPERSAMPLING: staged with the log2 table */
    __syncthreads();
    const double width = (double)p.width, height = (double)p.height;
    const double squared = p.limit * p.limit; /* :246 */
    const uint32_t iterations = p.iterations;
    ss_refine_loop<LINEAR>(a, s_lt, [&](uint64_t x, uint64_t y) {
        double re = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re + p.pos_re; /* coord_to_space, :182-184 */
        double im = (((double)y / height) - 0.5) / p.scale_im + p.pos_im;
        const double cre = JULIA ? p.julia_re : re, cim = JULIA ? p.julia_im : im; /* :209-210 */
        uint32_t i = 0;
        for (; i < iterations; i++) {
            const double tr = re + re;                    /* 2.0 * re is re + re, exactly */
            const double nre = (re * re - im * im) + cre; /* square() + c, :87-91 */
            const double nim = tr * im + cim;
            re = nre, im = nim;
            if (nre * nre + nim * nim > squared) break; /* (next, i); this lane leaves EXEC */
        }
        uint8_t rgb[3] = {0, 0, 0};
        const ColourConsts cc = make_colour_consts(p);
        colour_pixel<double>(cc, re, im, re * re, im * im, i, s_tab, nullptr, rgb);
        return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
    });
}

std::atomic<uint32_t> g_refine_groups{0}; /* fr_debug_ss_adaptive_grid: 0 = the default grid */

}  // namespace

namespace fr {

constexpr uint32_t kRefineGroupsDefault = 256 * 8; /* 256 CUs x 8 workgroups of 4 waves: every wave slot of the device */

/* fr_ss_list.h: the edge list as a refine kernel takes it, and the refine grid */
fr_ss_refine ss_refine_args(uint8_t *out, const uint32_t *list, unsigned long long *counters, uint32_t width, uint32_t y0, uint32_t s,
                            uint32_t bpp, int transfer) {
    fr_ss_refine a;
    a.linear = transfer == FR_SS_TRANSFER_SRGB;
    a.out = out;
    a.list = list;
    a.counters = counters;
    a.width = width;
    a.y0 = y0;
    a.s = s;
    a.s2 = s * s;
    a.ppw = 64u / a.s2;
    a.bpp = bpp;
    a.half = a.s2 / 2u;
    a.magic = (uint32_t)(((1ull << 31) + a.s2 - 1u) / a.s2);
    return a;
}

uint32_t ss_refine_groups(const fr_ss_refine &a, uint32_t rows) {
    /* the most work the rows can hold: every pixel an edge, ppw entries a claim, 4 waves a workgroup */
    const uint64_t claims = ((uint64_t)a.width * rows + a.ppw - 1) / a.ppw;
    const uint64_t cap = (claims + kSsRefineThreads / 64u - 1) / (kSsRefineThreads / 64u);
    const uint32_t groups = g_refine_groups.load();
    return groups ? groups : (uint32_t)std::min<uint64_t>(kRefineGroupsDefault, cap);
}

namespace {

/* what the adaptive calls have checked: the plan of cfg_s, the road with its centre and resolved bits */
struct SsaRoad {
    SsPlan pl;
    Centre c;
    int precision, road, bits;
    int tau;
};

/* everything the adaptive calls check before any device work, short of the buffers: the sizes, the threshold, then the road's own
 * domain on cfg_s with fr_render_rows_ss_de_device's argument rule per precision and road, plus FR_PT_ROAD_SCALED */
int ssa_check(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits, uint32_t s,
              int threshold, uint32_t y0, uint32_t y1, int channels, SsaRoad &r) {
    int rc = ss_plan(cfg, s, y0, y1, r.pl);
    if (rc == FR_OK) rc = check_channels(channels);
    if (rc != FR_OK) return rc;
    if (threshold < -1 || threshold > 255)
        return fail(FR_ERR_INVALID_ARGUMENT, "threshold must be -1 (every pixel is refined) or 0 .. 255");
    if ((uint64_t)cfg->width * (y1 - y0) > 0xFFFFFFFFull)
        return fail(FR_ERR_INVALID_ARGUMENT, "width * (y1 - y0) must be below 2^32: the edge list holds 32-bit pixel indices; call by row pieces");
    const fr_config *cs = &r.pl.cfg_s;
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + r.pl.src_rows);
    r.precision = precision;
    r.road = road;
    r.bits = bits;
    r.tau = threshold;
    r.c = Centre{pos_lo, centre};
    if (precision == FR_PRECISION_F32)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_F32 is out of scope of adaptive supersampling: precision must be FR_PRECISION_F64 or FR_PRECISION_PT");
    if (precision == FR_PRECISION_DD)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_DD is out of scope of adaptive supersampling: precision must be FR_PRECISION_F64 or FR_PRECISION_PT");
    if (precision != FR_PRECISION_F64 && precision != FR_PRECISION_PT)
        return fail(FR_ERR_INVALID_ARGUMENT, "precision must be FR_PRECISION_F64 or FR_PRECISION_PT");
    if (road != FR_PT_ROAD_PLAIN && road != FR_PT_ROAD_BLA && road != FR_PT_ROAD_SCALED)
        return fail(FR_ERR_INVALID_ARGUMENT, "road must be FR_PT_ROAD_PLAIN (0), FR_PT_ROAD_BLA (1) or FR_PT_ROAD_SCALED (2)");
    if (precision == FR_PRECISION_F64) {
        if (road != FR_PT_ROAD_PLAIN) return fail(FR_ERR_INVALID_ARGUMENT, "road: FR_PT_ROAD_BLA and FR_PT_ROAD_SCALED need FR_PRECISION_PT, the F64 road has no table");
        if (centre) return fail(FR_ERR_INVALID_ARGUMENT, "centre: a wide centre is for FR_PRECISION_PT only; the F64 road takes none");
        if (pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "pos_lo must be NULL unless precision is FR_PRECISION_PT");
        if (bits != 0) return fail(FR_ERR_INVALID_ARGUMENT, "bits must be 0 with FR_PT_ROAD_PLAIN: the plain loop has no table");
        return check_precision(precision);
    }
    switch (road) {
    case FR_PT_ROAD_PLAIN:
        if (bits != 0) return fail(FR_ERR_INVALID_ARGUMENT, "bits must be 0 with FR_PT_ROAD_PLAIN: the plain loop has no table");
        if (centre && pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "pos_lo must be NULL when a wide centre is given");
        return r.c.check(cs, FR_PRECISION_PT);
    case FR_PT_ROAD_BLA:
        return bla_check(cs, r.c, r.bits, Y0, Y1);
    default:
        if (pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: pos_lo must be NULL, the centre is the wide centre");
        r.c = Centre{nullptr, centre, true};
        return scaled_check(cs, r.c, r.bits, Y0, Y1);
    }
}

/* Rows [y0, y1) of the adaptive render into d_out on `stream`: the three passes.  Arguments checked, the rows and the width not
 * empty, d_work holds ss_adaptive_layout's bytes.  No host synchronisation (PT roads: apart from computing and uploading the view's
 * orbit and table when the context does not hold them yet), no allocation; the count stays in the workspace's first counter. */
int ssa_render(Ctx &ctx, const SsaRoad &r, const fr_config *cfg, uint32_t s, int transfer, uint32_t y0, uint32_t y1, unsigned bpp, void *d_out, void *d_work,
               hipStream_t stream) {
    const fr_config *cs = &r.pl.cfg_s;
    const SsAdaptiveLayout l = ss_adaptive_layout(cfg, y0, y1, false);
    uint8_t *const probe = static_cast<uint8_t *>(d_work) + l.colour_off; /* 0: no DE arrays in front */
    uint32_t *const list = reinterpret_cast<uint32_t *>(probe + l.list_off);
    unsigned long long *const counters = reinterpret_cast<unsigned long long *>(probe + l.counters_off);
    const bool escape_algo = cfg->algo == FR_ALGO_MANDELBROT || cfg->algo == FR_ALGO_JULIA;
    int rc = prof_begin(stream);
    if (rc != FR_OK) return rc;
    HIP_TRY(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), stream));

    /* 1. the probe pass */
    const uint32_t half = s / 2u;
    const fr_ss_map map{cfg->width, l.yb - l.ya, half, s, s * l.ya + half, s};
    fr_kout ko{};
    ko.rgb = probe;
    if (r.precision == FR_PRECISION_F64) {
        Opts o = default_opts();
        if (o.kernel_hint == -2) o.kernel_hint = -1; /* one choice, by name and size: no view sample, nothing blocks */
        fr_kparams p;
        fill_params(cs, o, p);
        map.apply(p);
        Profiling &pr = profiling(); /* the span is the call's: the probe's own events stay out of it */
        const bool was = pr.enabled;
        pr.enabled = false;
        rc = render_device(ctx, cs, p, FR_PRECISION_F64, o, probe, stream);
        pr.enabled = was;
    } else if (r.road == FR_PT_ROAD_BLA) {
        rc = bla_render_map(ctx, cs, r.c, r.bits, map, ko, stream);
    } else if (r.road == FR_PT_ROAD_SCALED) {
        rc = scaled_render_map(ctx, cs, r.c, r.bits, map, ko, stream);
    } else {
        fr_kparams p;
        fill_params(cs, default_opts(), p);
        map.apply(p);
        rc = launch_pt(ctx, cs, r.c, p, FR_OUT_RGB, ko, stream, nullptr);
    }
    if (rc != FR_OK) return rc;

    /* 2. the probe colours into d_out, the edge pixels into the list; an algorithm without orbits has none */
    ssm_params q;
    q.probe = probe;
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
    const uint64_t tiles = (uint64_t)q.tiles_x * (((uint64_t)q.rows + kMarkH - 1) / kMarkH);
    if (tiles > 0x7FFFFFFFull) return fail(FR_ERR_INVALID_ARGUMENT, "the row range holds too many tiles for one launch; call by row pieces");
    ss_mark_kernel<<<dim3((uint32_t)tiles), dim3(kMarkThreads), 0, stream>>>(q);
    HIP_TRY(hipGetLastError());

    /* 3. F over the probe bytes of the listed pixels; s = 1: F = P already; a threshold of 255: the list is empty */
    const char *kname = "ss_mark_kernel";
    if (s > 1 && escape_algo && r.tau < 255) {
        const fr_ss_refine a = ss_refine_args(q.out, list, counters, cfg->width, y0, s, bpp, transfer);
        const uint32_t groups = ss_refine_groups(a, q.rows);
        if (r.precision == FR_PRECISION_F64) {
            fr_kparams p;
            fill_params(cs, default_opts(), p);
            ss_refine_instance(cfg->algo == FR_ALGO_JULIA, a.linear, [&](auto J, auto L) {
                ss_refine_f64_kernel<J(), L()><<<dim3(groups), dim3(kSsRefineThreads), 0, stream>>>(p, a);
            });
            HIP_TRY(hipGetLastError());
            kname = "ss_refine_f64_kernel";
        } else if (r.road == FR_PT_ROAD_BLA) {
            rc = bla_ss_refine(ctx, cs, r.c, r.bits, a, groups, stream);
            kname = "ss_refine_bla_kernel";
        } else if (r.road == FR_PT_ROAD_SCALED) {
            rc = scaled_ss_refine(ctx, cs, r.c, r.bits, a, groups, stream);
            kname = "ss_refine_scaled_kernel";
        } else {
            rc = pt_ss_refine(ctx, cs, r.c, a, groups, stream);
            kname = "ss_refine_pt_kernel";
        }
        if (rc != FR_OK) return rc;
    }
    return prof_end(stream, kname);
}

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

int fr_ss_adaptive_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *bytes) {
    return ss_adaptive_workspace_bytes(cfg, supersample, y0, y1, false, bytes);
}

int fr_render_rows_ss_adaptive_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                      int bits, uint32_t supersample, int transfer, int threshold, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                      size_t out_len, void *d_work, size_t work_len, void *d_refined, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsaRoad r;
    const int rc = ssa_check(cfg, precision, pos_lo, centre, road, bits, supersample, threshold, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_adaptive_device(cfg, false, "work_len < bytes of fr_ss_adaptive_workspace_bytes",
                              "d_work must be 8-byte aligned (the list and the counters lie in it)", y0, y1, channels, d_out, out_len, d_work, work_len,
                              d_refined, hip_stream, [&](Ctx &ctx, uint32_t ya, uint32_t yb, void *dst, void *work, hipStream_t stream) {
                                  return ssa_render(ctx, r, cfg, supersample, transfer, ya, yb, (unsigned)channels, dst, work, stream);
                              });
}

int fr_render_rows_ss_adaptive_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                      int bits, uint32_t supersample, int threshold, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                      size_t out_len, void *d_work, size_t work_len, void *d_refined, void *hip_stream) {
    return fr_render_rows_ss_adaptive_tf_device(cfg, precision, pos_lo, centre, road, bits, supersample, FR_SS_TRANSFER_BYTES, threshold, y0, y1, channels, d_out, out_len, d_work, work_len, d_refined, hip_stream);
}

int fr_render_rows_ss_adaptive_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                               uint32_t supersample, int transfer, int threshold, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len,
                               uint64_t *refined) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsaRoad r;
    const int rc = ssa_check(cfg, precision, pos_lo, centre, road, bits, supersample, threshold, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_adaptive_host(cfg, false, y0, y1, channels, out, out_len, refined,
                            [&](Ctx &ctx, uint32_t ya, uint32_t yb, void *dst, void *work, hipStream_t stream) {
                                return ssa_render(ctx, r, cfg, supersample, transfer, ya, yb, (unsigned)channels, dst, work, stream);
                            });
}

int fr_render_rows_ss_adaptive(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                               uint32_t supersample, int threshold, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len,
                               uint64_t *refined) {
    return fr_render_rows_ss_adaptive_tf(cfg, precision, pos_lo, centre, road, bits, supersample, FR_SS_TRANSFER_BYTES, threshold, y0, y1, channels, out, out_len, refined);
}

int fr_debug_ss_adaptive_grid(uint32_t workgroups) {
    if (workgroups > (1u << 20)) return fail(FR_ERR_INVALID_ARGUMENT, "workgroups must be 0 (the default grid) or at most 2^20");
    g_refine_groups.store(workgroups);
    return FR_OK;
}

} /* extern "C" */
