/*
 * fr_ss.hip — supersampled rendering: render s times as large, box-filter on the device.
 *
 * The mode is DEFINED in include/fractal_hip.h ("supersampled rendering"): H = the image of cfg with width * s and
 * height * s, and out(X, Y, c) = (sum of the s x s block of H at (sX, sY) + floor(s*s / 2)) / (s*s), truncating.
 * Two pieces live here:
 *   - box_filter_kernel / fr_launch_box_filter: the reduction, one code path for every s in 1 .. FR_SS_MAX;
 *   - the entry points: fr_ss_workspace_bytes, fr_render_rows_ss_device (bands of source rows rendered into a workspace
 *     the caller lends, each filtered into its place, all on the caller's stream), fr_render_rows_ss (the same into a
 *     host buffer, through context scratch), fr_box_filter_rgb8(_device) (the filter alone).
 * The render kernels are not touched: a band is an ordinary row-range render of the large image.
 *
 * Kernel shape (memory-bound: it reads 3*s*s bytes and writes 3 or 4 per output pixel; DESIGN.md, "Supersampling"):
 *   - a workgroup of 256 lanes produces a tile of 256 output pixels x `ro` output rows (ro = 4, 2, 1 for s <= 2, 3, >= 4:
 *     12 .. 49 KiB of source per workgroup);
 *   - phase 1: the tile's s*ro source row segments (3*s*256 bytes each, any alignment: pixels are 3 bytes and the row
 *     pitch 3*s*W is whatever it is) go to LDS.  Each segment is cut at the 16-byte boundaries of its GLOBAL address:
 *     the aligned body moves as 16 bytes per lane (global_load_dwordx4 -> ds_write_b128, four loads in flight per lane),
 *     the < 16 head and < 16 tail bytes as single bytes by 32 lanes per row.  The segment sits in LDS at its address
 *     modulo 16, so the body's LDS stores are 16-byte aligned too.  Nothing outside the segment is read;
 *   - phase 2: lane x sums the s x s x 3 bytes of output pixel x out of LDS, adds floor(s*s/2) and divides by s*s with
 *     one v_mul_hi (2n * ceil(2^31 / d) >> 32: exact for n < 2^31 / d, and n <= 64 * 255 + 32);
 *   - RGBA: the lane stores its pixel as one dword (the destination is 4-byte aligned).  RGB: the bytes go back to LDS at
 *     the destination row's address modulo 4, and phase 3 writes the row segment as aligned dwords plus < 4 head and
 *     < 4 tail bytes;
 *   - 64-bit byte offsets throughout (a source may exceed 4 GiB); plain vector loads and stores only.
 */
#include "fr_ctx.h"

#include <algorithm>

namespace {

constexpr uint32_t kSsThreads = 256;                     /* lanes = output pixels per tile row */
constexpr uint32_t kSsOutPitch = 3 * kSsThreads + 16;    /* LDS bytes per staged RGB output row (3 spare + padding) */

__host__ __device__ inline uint32_t ss_in_pitch(uint32_t s) { return (3u * s * kSsThreads + 15u + 16u) & ~15u; }
inline uint32_t ss_tile_rows(uint32_t s) { return s <= 2 ? 4u : s == 3 ? 2u : 1u; }

struct ss_params {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t src_pitch; /* 3 * s * width */
    uint32_t width, rows; /* of the output */
    uint32_t s, ro;       /* supersample factor; output rows per tile */
    uint32_t tiles_x;
    uint32_t bpp;         /* 3 or 4 */
    uint32_t half, magic; /* floor(s*s / 2); ceil(2^31 / (s*s)) */
};

/* Chunk `idx` of the tile's flattened (source row, 16-byte chunk) list: loads it into v and returns its LDS offset, or
 * ~0u when idx names no whole aligned chunk of its row. */
__device__ inline uint32_t ss_load_chunk(uint32_t idx, uint32_t total, uint32_t cmax, uint32_t seg, uint32_t in_pitch,
                                         const uint8_t *seg0, uint64_t src_pitch, uint4 &v) {
    v = make_uint4(0u, 0u, 0u, 0u);
    if (idx >= total) return ~0u;
    const uint32_t k = idx / cmax, c = idx - k * cmax;
    const uint8_t *a = seg0 + (uint64_t)k * src_pitch;
    const uint32_t mis = (uint32_t)(uintptr_t)a & 15u;
    const uint32_t head = min(seg, (16u - mis) & 15u);
    const uint32_t body = (seg - head) / 16u; /* whole aligned chunks behind the head */
    if (c >= body) return ~0u;
    v = *static_cast<const uint4 *>(__builtin_assume_aligned(a + head + 16u * c, 16));
    return k * in_pitch + mis + head + 16u * c;
}

__global__ __launch_bounds__(kSsThreads) void box_filter_kernel(const ss_params p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
    const uint32_t x0 = tx * kSsThreads;
    const uint32_t nx = min(kSsThreads, p.width - x0); /* output pixels of this tile's rows */
    const uint32_t r0 = ty * p.ro;
    const uint32_t nr = min(p.ro, p.rows - r0);        /* output rows of this tile */
    const uint32_t s = p.s;
    const uint32_t nsrc = nr * s;                      /* source rows */
    const uint32_t seg = 3u * s * nx;                  /* bytes per source row segment */
    const uint32_t in_pitch = ss_in_pitch(s);
    const uint8_t *seg0 = p.src + (uint64_t)r0 * s * p.src_pitch + (uint64_t)3u * s * x0; /* row k: + k * src_pitch */

    /* ---- phase 1: source segments -> LDS, row k at lds[k * in_pitch + (address & 15)] ---- */
    const uint32_t cmax = seg / 16u + 1u; /* bound on a row's 16-byte chunks */
    const uint32_t total = nsrc * cmax;
    for (uint32_t base = 0; base < total; base += 4u * kSsThreads) {
        /* four chunks per lane, every load issued before the first LDS store (plain variables: an array indexed in an
         * unrolled loop went to scratch) */
        uint4 v0, v1, v2, v3;
        const uint32_t a0 = ss_load_chunk(base + tid, total, cmax, seg, in_pitch, seg0, p.src_pitch, v0);
        const uint32_t a1 = ss_load_chunk(base + kSsThreads + tid, total, cmax, seg, in_pitch, seg0, p.src_pitch, v1);
        const uint32_t a2 = ss_load_chunk(base + 2u * kSsThreads + tid, total, cmax, seg, in_pitch, seg0, p.src_pitch, v2);
        const uint32_t a3 = ss_load_chunk(base + 3u * kSsThreads + tid, total, cmax, seg, in_pitch, seg0, p.src_pitch, v3);
        if (a0 != ~0u) *static_cast<uint4 *>(__builtin_assume_aligned(lds + a0, 16)) = v0;
        if (a1 != ~0u) *static_cast<uint4 *>(__builtin_assume_aligned(lds + a1, 16)) = v1;
        if (a2 != ~0u) *static_cast<uint4 *>(__builtin_assume_aligned(lds + a2, 16)) = v2;
        if (a3 != ~0u) *static_cast<uint4 *>(__builtin_assume_aligned(lds + a3, 16)) = v3;
    }
    if (tid < nsrc * 32u) { /* heads and tails: lanes 0-15 of a row's 32 take the head bytes, 16-31 the tail bytes */
        const uint32_t k = tid >> 5, b = tid & 15u;
        const uint8_t *a = seg0 + (uint64_t)k * p.src_pitch;
        const uint32_t mis = (uint32_t)(uintptr_t)a & 15u;
        const uint32_t head = min(seg, (16u - mis) & 15u);
        const uint32_t tail = (seg - head) & 15u;
        if (tid & 16u) {
            if (b < tail) lds[k * in_pitch + mis + seg - tail + b] = a[seg - tail + b];
        } else {
            if (b < head) lds[k * in_pitch + mis + b] = a[b];
        }
    }
    __syncthreads();

    /* ---- phase 2: one output pixel per lane and tile row ---- */
    uint8_t *lds_out = lds + p.ro * s * in_pitch;
    for (uint32_t r = 0; r < nr; r++) {
        uint8_t *drow = p.dst + ((uint64_t)(r0 + r) * p.width + x0) * p.bpp;
        const uint32_t dmis = p.bpp == 4 ? 0u : (uint32_t)(uintptr_t)drow & 3u;
        if (tid < nx) {
            uint32_t sum[3] = {p.half, p.half, p.half};
            for (uint32_t j = 0; j < s; j++) {
                const uint32_t k = r * s + j;
                const uint32_t mis = (uint32_t)(uintptr_t)(seg0 + (uint64_t)k * p.src_pitch) & 15u;
                const uint8_t *q = lds + k * in_pitch + mis + 3u * s * tid;
                for (uint32_t i = 0; i < s; i++) {
                    sum[0] += q[3u * i];
                    sum[1] += q[3u * i + 1u];
                    sum[2] += q[3u * i + 2u];
                }
            }
            const uint32_t cr = __umulhi(2u * sum[0], p.magic), cg = __umulhi(2u * sum[1], p.magic),
                           cb = __umulhi(2u * sum[2], p.magic);
            if (p.bpp == 4) {
                reinterpret_cast<uint32_t *>(drow)[tid] = cr | cg << 8 | cb << 16 | 0xFF000000u;
            } else {
                uint8_t *o = lds_out + r * kSsOutPitch + dmis + 3u * tid;
                o[0] = (uint8_t)cr;
                o[1] = (uint8_t)cg;
                o[2] = (uint8_t)cb;
            }
        }
    }
    if (p.bpp == 4) return;
    __syncthreads();

    /* ---- phase 3 (RGB): the staged rows -> aligned dwords + head and tail bytes ---- */
    const uint32_t obytes = 3u * nx;
    for (uint32_t r = 0; r < nr; r++) {
        uint8_t *drow = p.dst + ((uint64_t)(r0 + r) * p.width + x0) * 3u;
        const uint32_t dmis = (uint32_t)(uintptr_t)drow & 3u;
        const uint32_t head = min(obytes, (4u - dmis) & 3u);
        const uint32_t body = (obytes - head) / 4u, tail = (obytes - head) & 3u;
        const uint8_t *o = lds_out + r * kSsOutPitch + dmis; /* o + head is 4-byte aligned */
        if (tid < body) {
            reinterpret_cast<uint32_t *>(drow + head)[tid] = reinterpret_cast<const uint32_t *>(o + head)[tid];
        } else if (tid >= 3u * kSsThreads / 4u) { /* 192 .. 197: lanes no body dword ever uses */
            const uint32_t b = tid - 3u * kSsThreads / 4u;
            if (b < head) drow[b] = o[b];
            else if (b >= 3u && b - 3u < tail) drow[obytes - tail + b - 3u] = o[obytes - tail + b - 3u];
        }
    }
}

}  // namespace

hipError_t fr_launch_box_filter(const void *src, uint32_t width, uint64_t rows, uint32_t s, uint32_t bpp, void *dst,
                                hipStream_t stream) {
    if (width == 0 || rows == 0) return hipSuccess;
    if (s < 1 || s > FR_SS_MAX || (bpp != 3 && bpp != 4)) return hipErrorInvalidValue;
    ss_params p;
    p.src_pitch = (uint64_t)3u * s * width;
    p.width = width;
    p.s = s;
    p.ro = ss_tile_rows(s);
    p.tiles_x = (uint32_t)(((uint64_t)width + kSsThreads - 1) / kSsThreads);
    p.bpp = bpp;
    p.half = s * s / 2u;
    p.magic = (uint32_t)(((1ull << 31) + s * s - 1u) / (s * s));
    const size_t lds_bytes = (size_t)p.ro * s * ss_in_pitch(s) + (bpp == 3 ? (size_t)p.ro * kSsOutPitch : 0u);
    /* launches of at most 2^30 workgroups (whole tile rows) */
    const uint64_t rows_per_launch = std::max<uint64_t>(1, (1ull << 30) / p.tiles_x) * p.ro;
    for (uint64_t ra = 0; ra < rows; ra += rows_per_launch) {
        const uint64_t n = std::min(rows - ra, rows_per_launch);
        if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
        p.src = static_cast<const uint8_t *>(src) + ra * s * p.src_pitch;
        p.dst = static_cast<uint8_t *>(dst) + ra * width * bpp;
        p.rows = (uint32_t)n;
        const uint64_t tiles = (uint64_t)p.tiles_x * ((n + p.ro - 1) / p.ro);
        box_filter_kernel<<<dim3((uint32_t)tiles), dim3(kSsThreads), lds_bytes, stream>>>(p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace fr {
namespace {

constexpr size_t kSsBestCap = (size_t)1 << 30;     /* fr_ss_workspace_bytes' best_bytes */
constexpr size_t kSsHostWorkCap = (size_t)256 << 20; /* the host road's workspace: the context keeps it */

struct SsPlan {
    fr_config cfg_s;      /* cfg with width * s, height * s */
    uint64_t src_rows;    /* s * (y1 - y0) */
    uint64_t row_bytes;   /* 3 * s * width: one source row */
    size_t min_bytes, best_bytes;
};

/* the part of the domain that needs no precision: cfg, s, the sizes, the rows */
int ss_plan(const fr_config *cfg, uint32_t s, uint32_t y0, uint32_t y1, SsPlan &pl) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (s < 1 || s > FR_SS_MAX) return fail(FR_ERR_INVALID_ARGUMENT, "supersample must be 1 .. FR_SS_MAX (8)");
    if ((uint64_t)cfg->width * s > 0xFFFFFFFFull)
        return fail(FR_ERR_INVALID_ARGUMENT, "supersample * width does not fit in 32 bits");
    if ((uint64_t)cfg->height * s > 0xFFFFFFFFull)
        return fail(FR_ERR_INVALID_ARGUMENT, "supersample * height does not fit in 32 bits");
    const int rc = check_rows(cfg, y0, y1); /* (cfg was read above: its NULL check stays in front of the sizes') */
    if (rc != FR_OK) return rc;
    pl.cfg_s = *cfg;
    pl.cfg_s.width = cfg->width * s;
    pl.cfg_s.height = cfg->height * s;
    pl.src_rows = (uint64_t)s * (y1 - y0);
    pl.row_bytes = (uint64_t)3u * s * cfg->width;
    if (s == 1) {
        pl.min_bytes = pl.best_bytes = 0;
        return FR_OK;
    }
    const uint64_t total = pl.src_rows * pl.row_bytes;
    const uint64_t mn = std::min<uint64_t>(8u * s, pl.src_rows) * pl.row_bytes;
    pl.min_bytes = (size_t)mn;
    pl.best_bytes = (size_t)std::max<uint64_t>(mn, std::min<uint64_t>(total, kSsBestCap));
    return FR_OK;
}

/* Source rows per band for a workspace of work_len >= min_bytes: the largest multiple of 8 * s that fits (or all the
 * rows), then evened out — nb = ceil(rows / Bmax) bands of ceil(rows / nb) rows rounded up to 8 * s. */
uint64_t ss_band_rows(const SsPlan &pl, uint32_t s, size_t work_len) {
    const uint64_t unit = 8u * s;
    uint64_t bmax = (uint64_t)work_len / pl.row_bytes;
    if (bmax >= pl.src_rows) return pl.src_rows;
    bmax = bmax / unit * unit;
    const uint64_t nb = (pl.src_rows + bmax - 1) / bmax;
    const uint64_t b = (pl.src_rows + nb - 1) / nb;
    return (b + unit - 1) / unit * unit;
}

/* Rows [y0, y1) supersampled into device memory on `stream`; arguments already checked, s >= 2, the range and the
 * width not empty.  No host synchronisation beyond what a plain device-pointer render of cfg_s has. */
int render_ss_device(Ctx &ctx, const SsPlan &pl, int precision, const fr_imaginary *pos_lo, uint32_t s, uint32_t y0,
                     unsigned bpp, void *d_out, void *d_work, size_t work_len, hipStream_t stream, const Opts &o) {
    const fr_config *cs = &pl.cfg_s;
    const uint32_t width = cs->width / s;
    const bool deep = precision == FR_PRECISION_DD || precision == FR_PRECISION_PT;
    const uint64_t band = ss_band_rows(pl, s, work_len);
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + pl.src_rows);
    Opts ob = o;
    if (!deep) decide_kernel(ctx, cs, precision, Y0, Y1, ob, stream, true); /* ONE choice for every band, as the host path's bands */
    const int pending_sample = ob.pending_sample;
    ob.pending_sample = -1;
    /* profiling: the span of the whole call — the first band records the start (and the render kernel's name), the
     * later bands record nothing, the end goes behind the last filter */
    Profiling &pr = profiling();
    struct ProfGuard {
        Profiling &pr;
        bool was;
        ~ProfGuard() { pr.enabled = was; }
    } prof_guard{pr, pr.enabled};
    int rc = FR_OK;
    for (uint64_t ya = Y0; ya < Y1 && rc == FR_OK; ya += band) {
        const uint32_t yb = (uint32_t)std::min<uint64_t>(ya + band, Y1);
        if (deep) {
            rc = render_deep_device(ctx, precision, cs, Centre{pos_lo, nullptr}, o, (uint32_t)ya, yb, 3, d_work, stream);
        } else {
            fr_kparams p;
            rows_params(cs, ob, (uint32_t)ya, yb, 3, p);
            rc = render_device(ctx, cs, p, precision, ob, d_work, stream);
        }
        if (rc != FR_OK) break;
        pr.enabled = false;
        uint8_t *dst = static_cast<uint8_t *>(d_out) + (uint64_t)(((uint32_t)ya - Y0) / s) * width * bpp;
        const hipError_t e = fr_launch_box_filter(d_work, width, (yb - (uint32_t)ya) / s, s, bpp, dst, stream);
        if (e != hipSuccess) rc = fail_hip(e, "fr_launch_box_filter");
    }
    ctx.post_sample(pending_sample, stream); /* behind the last band */
    if (rc == FR_OK && prof_guard.was && pr.have) HIP_TRY(hipEventRecord(pr.e1, stream));
    return rc;
}

/* everything fr_render_rows_ss(_device) check before any device work; fills pl and o */
int ss_check(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t s, uint32_t y0, uint32_t y1,
             int channels, const fr_render_opts *opts, SsPlan &pl, Opts &o) {
    int rc = ss_plan(cfg, s, y0, y1, pl);
    if (rc == FR_OK) rc = check_channels(channels);
    if (rc != FR_OK) return rc;
    if (pos_lo && precision != FR_PRECISION_DD && precision != FR_PRECISION_PT)
        return fail(FR_ERR_INVALID_ARGUMENT, "pos_lo must be NULL unless precision is FR_PRECISION_DD or FR_PRECISION_PT");
    rc = check_precision_lo(&pl.cfg_s, precision, pos_lo);
    if (rc == FR_OK) rc = resolve_opts(opts, o);
    return rc;
}

int box_filter_check(uint32_t width, uint32_t rows, uint32_t s, int channels) {
    if (s < 1 || s > FR_SS_MAX) return fail(FR_ERR_INVALID_ARGUMENT, "supersample must be 1 .. FR_SS_MAX (8)");
    if ((uint64_t)width * s > 0xFFFFFFFFull || (uint64_t)rows * s > 0xFFFFFFFFull)
        return fail(FR_ERR_INVALID_ARGUMENT, "supersample * width and supersample * rows must fit in 32 bits");
    return check_channels(channels);
}

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

int fr_ss_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *min_bytes,
                          size_t *best_bytes) {
    SsPlan pl;
    const int rc = ss_plan(cfg, supersample, y0, y1, pl);
    if (rc != FR_OK) return rc;
    if (min_bytes) *min_bytes = pl.min_bytes;
    if (best_bytes) *best_bytes = pl.best_bytes;
    return FR_OK;
}

int fr_render_rows_ss_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample,
                             uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work,
                             size_t work_len, void *hip_stream, const fr_render_opts *opts) {
    SsPlan pl;
    Opts o;
    int rc = ss_check(cfg, precision, pos_lo, supersample, y0, y1, channels, opts, pl, o);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * cfg->width * (size_t)(y1 - y0);
    if (need == 0) return FR_OK;
    if (!d_out) return fail(FR_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*(y1-y0)");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output (d_out) must be 4-byte aligned");
    if (supersample > 1) {
        if (work_len < pl.min_bytes)
            return fail(FR_ERR_BUFFER_TOO_SMALL, "work_len < min_bytes of fr_ss_workspace_bytes");
        if (!d_work) return fail(FR_ERR_INVALID_ARGUMENT, "d_work is NULL");
    }
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) {
        if (supersample == 1) { /* the plain render, byte for byte */
            if (precision == FR_PRECISION_DD || precision == FR_PRECISION_PT)
                return render_deep_device(ctx, precision, cfg, Centre{pos_lo, nullptr}, o, y0, y1, (unsigned)channels, d_out, stream);
            fr_kparams p;
            rows_params(cfg, o, y0, y1, (unsigned)channels, p);
            return render_device(ctx, cfg, p, precision, o, d_out, stream);
        }
        return render_ss_device(ctx, pl, precision, pos_lo, supersample, y0, (unsigned)channels, d_out, d_work, work_len, stream, o);
    });
}

int fr_render_rows_ss(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, uint32_t y0,
                      uint32_t y1, int channels, uint8_t *out, size_t out_len, const fr_render_opts *opts) {
    SsPlan pl;
    Opts o;
    int rc = ss_check(cfg, precision, pos_lo, supersample, y0, y1, channels, opts, pl, o);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * cfg->width * (size_t)(y1 - y0);
    if (need == 0) return FR_OK;
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*(y1-y0)");
    if (supersample == 1) { /* the plain host roads */
        if (precision == FR_PRECISION_DD || precision == FR_PRECISION_PT)
            return fr_host_render_rows_deep(cfg, precision, Centre{pos_lo, nullptr}, y0, y1, out, out_len, (unsigned)channels, opts);
        return fr_host_render_rows(cfg, precision, y0, y1, out, out_len, (unsigned)channels, opts);
    }
    const size_t work_len = std::max(pl.min_bytes, std::min(pl.best_bytes, kSsHostWorkCap));
    return host_rgb(out, need, [&](Ctx &ctx, void *d_out, hipStream_t stream) {
        int rc = ctx.reserve(ctx.ss_work, work_len);
        if (rc != FR_OK) return rc;
        rc = render_ss_device(ctx, pl, precision, pos_lo, supersample, y0, (unsigned)channels, d_out, ctx.ss_work.ptr, work_len, stream, o);
        if (rc != FR_OK) (void)hipStreamSynchronize(stream); /* the scratch is reused by the next call */
        return rc;
    });
}

int fr_box_filter_rgb8_device(const void *d_src, uint32_t width, uint32_t rows, uint32_t supersample, int channels,
                              void *d_out, size_t out_len, void *hip_stream) {
    const int rc = box_filter_check(width, rows, supersample, channels);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!d_src || !d_out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (d_src, d_out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output (d_out) must be 4-byte aligned");
    HIP_TRY(fr_launch_box_filter(d_src, width, rows, supersample, (uint32_t)channels, d_out, static_cast<hipStream_t>(hip_stream)));
    return FR_OK;
}

int fr_box_filter_rgb8(const uint8_t *src, uint32_t width, uint32_t rows, uint32_t supersample, int channels, uint8_t *out,
                       size_t out_len) {
    int rc = box_filter_check(width, rows, supersample, channels);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!src || !out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (src, out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    const size_t src_bytes = (size_t)3u * supersample * width * ((size_t)supersample * rows);
    LifeShared ls;
    Ctx *ctx;
    rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rc = ctx->reserve(ctx->ss_work, src_bytes);
    if (rc == FR_OK) rc = ctx->reserve(ctx->rgb, need);
    if (rc != FR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ss_work.ptr, src, src_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(fr_launch_box_filter(ctx->ss_work.ptr, width, rows, supersample, (uint32_t)channels, ctx->rgb.ptr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, ctx->rgb.ptr, need, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

} /* extern "C" */
