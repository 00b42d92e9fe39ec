/*
 * fr_ss_de.hip — SUPERSAMPLED DE (include/fractal_hip.h): distance estimation and supersampling at once.  The DE arrays
 * (z, iters, der) of cfg_s — width * s, height * s — coloured, distance-shaded with the thickness T * s in sample pixels and
 * box-filtered, byte for byte what fr_colour_de_rows_device followed by fr_box_filter_rgb8_device give.  Two pieces live here:
 *   - colour_de_filter_kernel<S> / fr_launch_colour_de_filter: colour map + distance shade + box filter in one pass, no RGB
 *     image of cfg_s in between;
 *   - the entry points: fr_colour_de_rows_ss_device / fr_colour_de_ss_rgb8 (a KEPT anti-aliased DE view recoloured),
 *     fr_ss_de_workspace_bytes, fr_render_rows_ss_de_device (bands of source rows rendered into a workspace the caller lends — the
 *     road's own DE launch between the profiling events, fr_de.h: de_render_rows — each shaded and filtered into its place, all on the caller's stream) and
 *     fr_render_rows_ss_de (the same into a host buffer, through context scratch), and SUPERSAMPLED SCALED DE's
 *     fr_render_rows_ss_de_pt_scaled(_device): the same band loop and the same fused kernel with DE ON SCALED PT's launch
 *     (fr_de.h: scaled_de_launch) and the scaled view's pixels.
 * The render kernels are not touched: a band is an ordinary row-range DE render of the large image.  The band loop, the two
 * halves of a banded call and the thickness and pixels of the shade are fr_ss.h's ("3.32"); the recolour's host form
 * goes through host_rgb (fr_ctx.h).
 *
 * Kernel shape: colour_filter_kernel<S>'s (fr_ss.hip), which it differs from in phase 1 only.  Memory-bound:
 * 36 B per sample in, 3 or 4 B per output pixel out.
 *   - a workgroup of 256 lanes owns tiles of 64 output pixels x cf_tile_rows(S) output rows, cf_tiles_per_group(S) of them a
 *     grid's width apart; the 3 KB log2 table is staged once per workgroup WHENEVER the algorithm has orbits: the colour map
 *     reads it only when smooth, the distance always;
 *   - phase 1: one sample per lane, four in flight: consecutive lanes load consecutive samples of a source row — z and der as
 *     one 16-byte access each (the arrays are 8-byte aligned, which a global load of four dwords takes), iters as 4 bytes —
 *     colour them with colour_of, shade them exactly as colour_de_rows_kernel does (fr_de_shade.h: de_distance, the same
 *     operation order) and park the packed r | g << 8 | b << 16 in LDS.  The two f64 square roots and the two divisions
 *     stand behind `iters < iterations && Ts > 0`: a wave of capped samples, or any wave at Ts == 0, never executes them;
 *   - LDS: table 3 KiB + samples 4 S S ro 64 B (4, 9, 16, 12.5, 18, 12.25, 16 KiB for S = 2 .. 8) + RGB staging 208 ro B: at
 *     most 21.4 KiB (S = 6), seven workgroups a CU by LDS; registers decide before that;
 *   - 64-bit element offsets (a kept 3840 x 2160 DE view at s = 4 is 4.8 GB); plain vector loads and stores only.
 */
#include <algorithm>

#include "fr_bla.h" /* scaled_consts */
#include "fr_ctx.h"
#include "fr_de.h"
#include "fr_math.h"
#include "fr_ss.h"

namespace {

#include "fr_colour.h"   /* the colour map of the renders */
#include "fr_de_shade.h" /* de_distance */
#include "fr_srgb.h"     /* LINEAR-LIGHT SUPERSAMPLING: the tables of the filter's LINEAR instances */

/* The tile: colour_filter_kernel's (fr_ss.hip), restated.  That kernel keeps its own copy: routing both kernels through one
 * shared function changed colour_filter_kernel's instruction stream (tools/isa_digest.py), and this file leaves the device code
 * of the existing units as it was. */
constexpr uint32_t kCfTileW = 64;                    /* output pixels per tile row: one wave */
constexpr uint32_t kCfThreads = 256;
constexpr uint32_t kCfOutPitch = 3 * kCfTileW + 16;  /* LDS bytes per staged RGB output row (3 spare + padding; a multiple of 4) */
__host__ __device__ constexpr uint32_t cf_tile_rows(uint32_t s) { return s <= 4 ? 4u : s <= 6 ? 2u : 1u; }
/* tiles per workgroup: at least 4096 samples behind one staging of the table */
constexpr uint32_t cf_tiles_per_group(uint32_t s) {
    const uint32_t per_tile = kCfTileW * s * s * cf_tile_rows(s);
    return (4096u + per_tile - 1u) / per_tile;
}

/* kernel arguments re-read where the colour map needs them (fr_kernels.hip: FR_COLD_PARAMS; `p` is argument 0) */
typedef const __attribute__((address_space(4))) fr_kparams *CfKArgs;

struct cfd_params {
    const double *z, *der;
    const uint32_t *iters;
    uint8_t *dst;
    uint64_t pitch;       /* s * width: samples per source row */
    uint32_t width, rows; /* of the output */
    uint32_t tiles_x, n_tiles;
    uint32_t bpp;         /* 3 or 4 */
    double pixels;        /* (double)(s * height) * min(|scale.re|, |scale.im|): sample pixels per unit of the plane */
    double thickness;     /* Ts = T * s, in sample pixels */
};

/* Phases 2 and 3 of one tile, called by all 256 lanes behind the barrier that ends phase 1.  s_px holds the tile's packed
 * r | g << 8 | b << 16 words at [source row][sample] (`have` false: an algorithm without orbits, every sum is 0); lane l of wave
 * w owns output pixel (x0 + l, r0 + w) of q.dst.  RGBA leaves as one dword per lane; RGB goes to s_out at the destination row's address
 * modulo 4 and, behind one barrier, out as aligned dwords (lanes 0 .. 47) plus < 4 head and < 4 tail bytes (lanes 48 .. 53).
 * LINEAR (LINEAR-LIGHT SUPERSAMPLING): s_lt is the workgroup's staged tables (fr_srgb.h); a sample's three bytes are decoded as
 * its word is read, the sums (22 bits) have a register each, the quotients are encoded.  The byte form does not read s_lt. */
template <uint32_t S, bool LINEAR>
__device__ __forceinline__ void cf_filter_tile(const uint32_t *s_px, uint8_t *s_out, const uint16_t *s_lt, bool have, const cfd_params &q,
                                               uint32_t x0, uint32_t r0, uint32_t nx, uint32_t nr, uint32_t w, uint32_t l) {
    constexpr uint32_t SW = kCfTileW * S;
    constexpr uint32_t HALF = S * S / 2u, MAGIC = (uint32_t)(((1ull << 31) + S * S - 1u) / (S * S));
    /* ---- phase 2: one output pixel per lane ---- */
    const bool live = w < nr && l < nx;
    uint8_t *drow = q.dst + ((uint64_t)(r0 + (w < nr ? w : 0u)) * q.width + x0) * q.bpp; /* the wave's output row */
    const uint32_t dmis = q.bpp == 4u ? 0u : (uint32_t)(uintptr_t)drow & 3u;
    if (live) {
        [[maybe_unused]] uint32_t rb = HALF | HALF << 16, gg = HALF; /* r and b in the halves of one word: a sum is at most 64 * 255 + 32 */
        [[maybe_unused]] uint32_t lr = HALF, lg = HALF, lb = HALF;   /* LINEAR: a sum is at most 64 * 65535 + 32 */
        if (have) {
            for (uint32_t j = 0; j < S; j++) {
                const uint32_t *row = s_px + (w * S + j) * SW + l * S;
                if constexpr (LINEAR) {
                    for (uint32_t i = 0; i < S; i++) {
                        const uint32_t v = row[i];
                        lr += srgb_decode(s_lt, v & 0xFFu);
                        lg += srgb_decode(s_lt, v >> 8 & 0xFFu);
                        lb += srgb_decode(s_lt, v >> 16);
                    }
                } else if constexpr (S % 4u == 0u) {
                    for (uint32_t i = 0; i < S; i += 4u) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(row + i);
                        rb += (v.x & 0x00FF00FFu) + (v.y & 0x00FF00FFu) + (v.z & 0x00FF00FFu) + (v.w & 0x00FF00FFu);
                        gg += (v.x >> 8 & 0xFFu) + (v.y >> 8 & 0xFFu) + (v.z >> 8 & 0xFFu) + (v.w >> 8 & 0xFFu);
                    }
                } else if constexpr (S % 2u == 0u) {
                    for (uint32_t i = 0; i < S; i += 2u) {
                        const uint2 v = *reinterpret_cast<const uint2 *>(row + i);
                        rb += (v.x & 0x00FF00FFu) + (v.y & 0x00FF00FFu);
                        gg += (v.x >> 8 & 0xFFu) + (v.y >> 8 & 0xFFu);
                    }
                } else {
                    for (uint32_t i = 0; i < S; i++) {
                        const uint32_t v = row[i];
                        rb += v & 0x00FF00FFu;
                        gg += v >> 8 & 0xFFu;
                    }
                }
            }
        }
        uint32_t cr, cg, cb;
        if constexpr (LINEAR) {
            cr = srgb_encode(s_lt, __umulhi(2u * lr, MAGIC));
            cg = srgb_encode(s_lt, __umulhi(2u * lg, MAGIC));
            cb = srgb_encode(s_lt, __umulhi(2u * lb, MAGIC));
        } else {
            cr = __umulhi(2u * (rb & 0xFFFFu), MAGIC), cg = __umulhi(2u * gg, MAGIC), cb = __umulhi(2u * (rb >> 16), MAGIC);
        }
        if (q.bpp == 4u) {
            reinterpret_cast<uint32_t *>(drow)[l] = cr | cg << 8 | cb << 16 | 0xFF000000u;
        } else {
            uint8_t *o = s_out + w * kCfOutPitch + dmis + 3u * l;
            o[0] = (uint8_t)cr;
            o[1] = (uint8_t)cg;
            o[2] = (uint8_t)cb;
        }
    }
    if (q.bpp == 4u) return; /* uniform */
    __syncthreads();

    /* ---- phase 3 (RGB): wave w's staged row -> aligned dwords + head and tail bytes ---- */
    if (w < nr) {
        const uint32_t obytes = 3u * nx;
        const uint32_t head = min(obytes, (4u - dmis) & 3u);
        const uint32_t body = (obytes - head) / 4u, tail = (obytes - head) & 3u; /* body <= 48 */
        const uint8_t *o = s_out + w * kCfOutPitch + dmis; /* o + head is 4-byte aligned */
        if (l < body) {
            reinterpret_cast<uint32_t *>(drow + head)[l] = reinterpret_cast<const uint32_t *>(o + head)[l];
        } else if (l >= 48u) { /* 48 .. 53: lanes no body dword ever uses */
            const uint32_t b = l - 48u;
            if (b < head) drow[b] = o[b];
            else if (b >= 3u && b - 3u < tail) drow[obytes - tail + b - 3u] = o[obytes - tail + b - 3u];
        }
    }
}

/* re, im of one sample: 16 bytes moved at once from an 8-byte aligned array */
struct __attribute__((aligned(8))) cfd_pair {
    double x, y;
};

struct cfd_sample {
    cfd_pair z, d;
    uint32_t iters;
    uint32_t at; /* the sample's LDS word, ~0u = none */
};

/* sample `idx` of the tile's flattened (source row, column) grid: loaded when it lies inside the image */
template <uint32_t S>
__device__ __forceinline__ cfd_sample cfd_load(uint32_t idx, uint32_t nsx, uint32_t nsy, const cfd_params &q, uint64_t k00) {
    constexpr uint32_t SW = kCfTileW * S, N = SW * S * cf_tile_rows(S);
    cfd_sample v{{0.0, 0.0}, {0.0, 0.0}, 0u, ~0u};
    const uint32_t k = idx / SW, c = idx - k * SW;
    if (idx < N && k < nsy && c < nsx) {
        const uint64_t g = k00 + (uint64_t)k * q.pitch + c;
        v.z = reinterpret_cast<const cfd_pair *>(q.z)[g];
        v.d = reinterpret_cast<const cfd_pair *>(q.der)[g];
        v.iters = q.iters[g];
        v.at = idx;
    }
    return v;
}

/* colour_de_rows_kernel's pixel (fr_de.hip), operation for operation, into the sample's LDS word */
__device__ __forceinline__ void cfd_colour(const cfd_sample &v, uint32_t iterations, double pixels, double thickness, const double *s_tab,
                                           uint32_t *s_px) {
    if (v.at == ~0u) return;
    uint8_t rgb[3] = {0, 0, 0};
    {
        CfKArgs kp = (CfKArgs)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp)); /* opaque: the ~40 constants are loaded here, not held across the kernel */
        const ColourConsts cc = make_colour_consts(*kp);
        colour_of(cc, v.z.x * v.z.x + v.z.y * v.z.y, v.iters, s_tab, nullptr, rgb);
    }
    uint32_t r = rgb[0], g = rgb[1], b = rgb[2];
    if (v.iters < iterations && thickness > 0.0) {
        const double s = de_distance(v.z.x, v.z.y, v.d.x, v.d.y, v.iters, iterations, pixels, s_tab) / thickness;
        if (s < 1.0) { /* 0 <= byte * s < 255: the cast truncates, nothing saturates */
            r = (uint32_t)((double)r * s);
            g = (uint32_t)((double)g * s);
            b = (uint32_t)((double)b * s);
        }
    }
    s_px[v.at] = r | (g << 8) | (b << 16);
}

template <uint32_t S, bool LINEAR>
__global__ __launch_bounds__(kCfThreads) void colour_de_filter_kernel(const fr_kparams p, const cfd_params q) {
    constexpr uint32_t RO = cf_tile_rows(S), SW = kCfTileW * S, N = SW * S * RO;
    __shared__ double s_tab[FR_LOG2_N * 3];
    __shared__ __attribute__((aligned(16))) uint32_t s_px[N];
    __shared__ uint32_t s_out_words[RO * kCfOutPitch / 4u];
    uint8_t *const s_out = reinterpret_cast<uint8_t *>(s_out_words);
    const uint32_t tid = threadIdx.x;
    const bool escape_algo = p.algo == 0 || p.algo == 2;
    if (escape_algo) { /* uniform; the distance reads the table whether the colour map does or not */
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += kCfThreads) s_tab[k] = gt[k];
    }
    const uint16_t *s_lt = nullptr;
    if constexpr (LINEAR) { /* 1 KiB beside the log2 table, before the first tile's barrier */
        __shared__ uint16_t s_srgb[kSrgbLdsWords];
        srgb_stage(s_srgb, tid, kCfThreads);
        s_lt = s_srgb;
    }
    const uint32_t iterations = p.iterations;
    const uint32_t w = tid >> 6, l = tid & 63u; /* phase 2 and 3: output row of the tile, output pixel of the row */
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
        const uint32_t x0 = tx * kCfTileW, r0 = ty * RO;
        const uint32_t nx = min(kCfTileW, q.width - x0), nr = min(RO, q.rows - r0);
        __syncthreads(); /* the table is staged; the previous tile's rows have left s_out */

        /* ---- phase 1: samples -> shaded colours -> LDS ---- */
        if (escape_algo) {
            const uint64_t k00 = (uint64_t)r0 * S * q.pitch + (uint64_t)x0 * S;
            const uint32_t nsx = nx * S, nsy = nr * S;
            for (uint32_t base = 0; base < N; base += 4u * kCfThreads) {
                const cfd_sample v0 = cfd_load<S>(base + tid, nsx, nsy, q, k00);
                const cfd_sample v1 = cfd_load<S>(base + kCfThreads + tid, nsx, nsy, q, k00);
                const cfd_sample v2 = cfd_load<S>(base + 2u * kCfThreads + tid, nsx, nsy, q, k00);
                const cfd_sample v3 = cfd_load<S>(base + 3u * kCfThreads + tid, nsx, nsy, q, k00);
                cfd_colour(v0, iterations, q.pixels, q.thickness, s_tab, s_px);
                cfd_colour(v1, iterations, q.pixels, q.thickness, s_tab, s_px);
                cfd_colour(v2, iterations, q.pixels, q.thickness, s_tab, s_px);
                cfd_colour(v3, iterations, q.pixels, q.thickness, s_tab, s_px);
            }
        }
        __syncthreads();

        /* ---- phases 2 and 3: the s x s sums, the division, the way out ---- */
        cf_filter_tile<S, LINEAR>(s_px, s_out, s_lt, escape_algo, q, x0, r0, nx, nr, w, l);
    }
}

template <uint32_t S>
hipError_t cfd_launch(const fr_kparams &p, const cfd_params &q, bool linear, hipStream_t stream) {
    const uint32_t groups = (q.n_tiles + cf_tiles_per_group(S) - 1u) / cf_tiles_per_group(S);
    if (linear) colour_de_filter_kernel<S, true><<<dim3(groups), dim3(kCfThreads), 0, stream>>>(p, q);
    else colour_de_filter_kernel<S, false><<<dim3(groups), dim3(kCfThreads), 0, stream>>>(p, q);
    return hipGetLastError();
}

}  // namespace

hipError_t fr_launch_colour_de_filter(const fr_kparams &p, const double *z, const uint32_t *iters, const double *der, uint32_t width,
                                      uint64_t rows, uint32_t s, double pixels, double thickness, uint32_t bpp, void *dst,
                                      hipStream_t stream, int transfer) {
    if (width == 0 || rows == 0) return hipSuccess;
    if (s < 1 || s > FR_SS_MAX || (bpp != 3 && bpp != 4)) return hipErrorInvalidValue;
    const bool linear = transfer == FR_SS_TRANSFER_SRGB;
    if (s == 1) /* nothing to filter */
        return fr_launch_colour_de_rows(p, z, iters, der, (size_t)width * rows, pixels, thickness, bpp, dst, stream);
    cfd_params q;
    q.pitch = (uint64_t)s * width;
    q.width = width;
    q.tiles_x = (uint32_t)(((uint64_t)width + kCfTileW - 1) / kCfTileW);
    q.bpp = bpp;
    q.pixels = pixels;
    q.thickness = thickness;
    const uint32_t ro = cf_tile_rows(s);
    /* launches of at most 2^30 tiles (whole tile rows) */
    const uint64_t rows_per_launch = std::max<uint64_t>(1, (1ull << 30) / q.tiles_x) * ro;
    for (uint64_t ra = 0; ra < rows; ra += rows_per_launch) {
        const uint64_t n = std::min(rows - ra, rows_per_launch);
        const uint64_t first = ra * s * q.pitch; /* the launch's first sample */
        q.z = z + first * 2u;
        q.der = der + first * 2u;
        q.iters = iters + first;
        q.dst = static_cast<uint8_t *>(dst) + ra * width * bpp;
        q.rows = (uint32_t)n;
        q.n_tiles = (uint32_t)(q.tiles_x * ((n + ro - 1) / ro));
        hipError_t e;
        switch (s) {
        case 2: e = cfd_launch<2>(p, q, linear, stream); break;
        case 3: e = cfd_launch<3>(p, q, linear, stream); break;
        case 4: e = cfd_launch<4>(p, q, linear, stream); break;
        case 5: e = cfd_launch<5>(p, q, linear, stream); break;
        case 6: e = cfd_launch<6>(p, q, linear, stream); break;
        case 7: e = cfd_launch<7>(p, q, linear, stream); break;
        default: e = cfd_launch<8>(p, q, linear, stream); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace fr {
namespace {

/* the domain of fr_colour_de_rows_ss_device / fr_colour_de_ss_rgb8 short of the buffers */
int colour_de_ss_check(const fr_config *cfg, uint32_t width, uint32_t rows, uint32_t s, double thickness, int channels, double &ts) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (s < 1 || s > FR_SS_MAX) return fail(FR_ERR_INVALID_ARGUMENT, "supersample must be 1 .. FR_SS_MAX (8)");
    if ((uint64_t)width * s > 0xFFFFFFFFull || (uint64_t)rows * s > 0xFFFFFFFFull || (uint64_t)cfg->height * s > 0xFFFFFFFFull)
        return fail(FR_ERR_INVALID_ARGUMENT, "supersample * width, supersample * rows and supersample * cfg->height must fit in 32 bits");
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = ss_de_thickness(thickness, s, ts);
    return rc;
}

/* what fr_render_rows_ss_de(_device) have checked: the plan at 36 bytes per sample, the road, its centre and resolved bits */
struct SsDeRoad {
    SsPlan pl;
    Centre c;
    int precision, road, bits;
    double ts, pixels;
    /* source rows [ya, yb) of cfg_s with their derivatives on the road */
    int rows(Ctx &ctx, uint32_t ya, uint32_t yb, double *d_z, uint32_t *d_iters, double *d_der, hipStream_t stream) const {
        const fr_config *const cs = &pl.cfg_s;
        if (road == FR_PT_ROAD_SCALED) return de_render_rows(ctx, cs, ya, yb, d_z, d_iters, d_der, stream, de_road(scaled_de_launch, cs, c, bits));
        if (road == FR_PT_ROAD_BLA) return de_render_rows(ctx, cs, ya, yb, d_z, d_iters, d_der, stream, de_road(bla_de_launch, cs, c, bits));
        return de_render_rows(ctx, cs, ya, yb, d_z, d_iters, d_der, stream, de_road(de_launch, cs, precision, c));
    }
};

/* the head of both checks below: the sizes at 36 bytes per sample, the channels, the thickness; then the road as it was asked for */
int ss_de_head(const fr_config *cfg, int precision, const Centre &c, int road, int bits, double thickness, uint32_t s, uint32_t y0, uint32_t y1,
               int channels, SsDeRoad &r) {
    int rc = ss_plan(cfg, s, y0, y1, r.pl, kDeSampleBytes);
    if (rc == FR_OK) rc = check_channels(channels);
    if (rc == FR_OK) rc = ss_de_thickness(thickness, s, r.ts);
    r.precision = precision;
    r.road = road;
    r.bits = bits;
    r.c = c;
    return rc;
}

/* everything fr_render_rows_ss_de(_device) check before any device work: the sizes, the thickness, then the road's own DE
 * domain on cfg_s, by the code its plain calls run */
int ss_de_check(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                double thickness, uint32_t s, uint32_t y0, uint32_t y1, int channels, SsDeRoad &r) {
    const int rc = ss_de_head(cfg, precision, Centre{pos_lo, centre}, road, bits, thickness, s, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    const fr_config *cs = &r.pl.cfg_s;
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + r.pl.src_rows);
    r.pixels = ss_de_pixels(cfg, s);
    if (road == FR_PT_ROAD_SCALED)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PT_ROAD_SCALED: distance estimation on SCALED PT is out of scope; supersampled DE takes "
                                             "FR_PRECISION_F64, FR_PRECISION_PT (dd or wide centre) and BLA-PT");
    if (road != FR_PT_ROAD_PLAIN && road != FR_PT_ROAD_BLA)
        return fail(FR_ERR_INVALID_ARGUMENT, "road must be FR_PT_ROAD_PLAIN (0) or FR_PT_ROAD_BLA (1)");
    if (centre && pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "pos_lo must be NULL when a wide centre is given");
    if (precision == FR_PRECISION_F64) {
        if (road != FR_PT_ROAD_PLAIN) return fail(FR_ERR_INVALID_ARGUMENT, "FR_PT_ROAD_BLA needs FR_PRECISION_PT: the F64 road has no table");
        if (centre) return fail(FR_ERR_INVALID_ARGUMENT, "a wide centre is for FR_PRECISION_PT only; the F64 road takes none");
    }
    if (road == FR_PT_ROAD_BLA && precision == FR_PRECISION_PT) return bla_de_domain(cs, r.c, r.bits, Y0, Y1);
    if (bits != 0 && (precision == FR_PRECISION_F64 || precision == FR_PRECISION_PT))
        return fail(FR_ERR_INVALID_ARGUMENT, "bits must be 0 with FR_PT_ROAD_PLAIN: the plain loop has no table");
    /* F64 and plain PT; every other precision meets DE's scope message here */
    return de_domain(cs, precision, r.c, precision == FR_PRECISION_PT && centre != nullptr, Y0, Y1);
}

/* SUPERSAMPLED SCALED DE: everything fr_render_rows_ss_de_pt_scaled(_device) check before any device work — the sizes, the
 * thickness, then DE ON SCALED PT's domain on cfg_s, by the code its plain calls run.  The road's arm of SsDeRoad: rows() is
 * fr_escape_rows_de_pt_scaled's launch and `pixels` the last factor of D on the scaled view of cfg_s. */
int ss_de_scaled_check(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t s, uint32_t y0, uint32_t y1,
                       int channels, SsDeRoad &r) {
    int rc = ss_de_head(cfg, FR_PRECISION_PT, Centre{nullptr, centre, true}, FR_PT_ROAD_SCALED, bits, thickness, s, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + r.pl.src_rows);
    rc = scaled_de_domain(&r.pl.cfg_s, r.c, r.bits, Y0, Y1);
    if (rc != FR_OK) return rc;
    const ScaledConsts k = scaled_consts(cfg); /* cfg_s shares cfg's scale */
    r.pixels = ss_de_pixels(cfg, s, k.sre, k.sim);
    return FR_OK;
}

/* The bands: ss_bands (fr_ss.h) with the DE arrays in the workspace and the fused kernel behind each band.  A band of n samples
 * lies at d_work as z (16 n bytes) | der (16 n) | iters (4 n). */
int render_ss_de_bands(Ctx &ctx, const SsDeRoad &r, uint32_t s, int transfer, uint32_t y0, unsigned bpp, void *d_out, void *d_work, size_t work_len,
                       hipStream_t stream) {
    const uint32_t width = r.pl.cfg_s.width / s;
    fr_kparams p;
    fill_params(&r.pl.cfg_s, default_opts(), p);
    return ss_bands(ctx, r.pl, s, y0, bpp, d_out, work_len, stream, -1,
                    [&](Ctx &c, uint32_t ya, uint32_t yb, uint8_t *dst, uint32_t out_rows, hipStream_t st) {
                        const uint64_t n = (uint64_t)(yb - ya) * r.pl.cfg_s.width;
                        double *const d_z = static_cast<double *>(d_work), *const d_der = d_z + 2 * n;
                        uint32_t *const d_iters = reinterpret_cast<uint32_t *>(d_der + 2 * n);
                        const int rc = r.rows(c, ya, yb, d_z, d_iters, d_der, st);
                        if (rc != FR_OK) return rc;
                        const hipError_t e = fr_launch_colour_de_filter(p, d_z, d_iters, d_der, width, out_rows, s, r.pixels, r.ts, bpp, dst, st, transfer);
                        return e == hipSuccess ? FR_OK : fail_hip(e, "fr_launch_colour_de_filter");
                    });
}

/* the four banded entry points behind their checks (fr_ss.h: ss_rows_device, ss_rows_host) */
int ss_de_rows_device(const fr_config *cfg, const SsDeRoad &r, uint32_t s, int transfer, uint32_t y0, uint32_t y1, int channels, void *d_out,
                      size_t out_len, void *d_work, size_t work_len, void *hip_stream) {
    return ss_rows_device(cfg, r.pl, "work_len < min_bytes of fr_ss_de_workspace_bytes", true, y0, y1, channels, d_out, out_len, d_work, work_len,
                          hip_stream, [&](Ctx &ctx, const fr_kout &ko, void *work, size_t len, hipStream_t stream) {
                              return render_ss_de_bands(ctx, r, s, transfer, y0, (unsigned)channels, ko.rgb, work, len, stream);
                          });
}

int ss_de_rows_host(const fr_config *cfg, const SsDeRoad &r, uint32_t s, int transfer, uint32_t y0, uint32_t y1, int channels, uint8_t *out,
                    size_t out_len) {
    return ss_rows_host(cfg, ss_host_work_len(r.pl), y0, y1, channels, out, out_len,
                        [&](Ctx &ctx, const fr_kout &ko, void *work, size_t len, hipStream_t stream) {
                            return render_ss_de_bands(ctx, r, s, transfer, y0, (unsigned)channels, ko.rgb, work, len, stream);
                        });
}

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

int fr_colour_de_rows_ss_tf_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, uint32_t width, uint32_t rows,
                                uint32_t supersample, int transfer, double thickness, int channels, void *d_out, size_t out_len, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    double ts;
    const int rc = colour_de_ss_check(cfg, width, rows, supersample, thickness, channels, ts);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!d_z || !d_iters || !d_der || !d_out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (d_z, d_iters, d_der, d_out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    if ((reinterpret_cast<uintptr_t>(d_z) & 7u) || (reinterpret_cast<uintptr_t>(d_der) & 7u) || (reinterpret_cast<uintptr_t>(d_iters) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "d_z and d_der must be 8-byte aligned and d_iters 4-byte aligned");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output (d_out) must be 4-byte aligned");
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    HIP_TRY(fr_launch_colour_de_filter(p, static_cast<const double *>(d_z), static_cast<const uint32_t *>(d_iters),
                                       static_cast<const double *>(d_der), width, rows, supersample, ss_de_pixels(cfg, supersample), ts,
                                       (uint32_t)channels, d_out, static_cast<hipStream_t>(hip_stream), transfer));
    return FR_OK;
}

int fr_colour_de_rows_ss_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, uint32_t width, uint32_t rows,
                                uint32_t supersample, double thickness, int channels, void *d_out, size_t out_len, void *hip_stream) {
    return fr_colour_de_rows_ss_tf_device(cfg, d_z, d_iters, d_der, width, rows, supersample, FR_SS_TRANSFER_BYTES, thickness, channels, d_out, out_len, hip_stream);
}

int fr_colour_de_ss_rgb8_tf(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, uint32_t width, uint32_t rows,
                         uint32_t supersample, int transfer, double thickness, int channels, uint8_t *out, size_t out_len) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    double ts;
    int rc = colour_de_ss_check(cfg, width, rows, supersample, thickness, channels, ts);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!z || !iters || !der || !out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (z, iters, der, out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    const size_t n = (size_t)supersample * width * ((size_t)supersample * rows);
    const size_t zb = n * 2 * sizeof(double), ib = n * sizeof(uint32_t);
    return host_rgb(out, need, [&](Ctx &ctx, void *d_out, hipStream_t stream) -> int {
        int rc = ctx.reserve(ctx.z, 2 * zb); /* z, then der */
        if (rc == FR_OK) rc = ctx.reserve(ctx.iters, ib);
        if (rc != FR_OK) return rc;
        double *const d_z = static_cast<double *>(ctx.z.ptr), *const d_der = d_z + 2 * n;
        fr_kparams p;
        fill_params(cfg, default_opts(), p);
        HIP_TRY(hipMemcpyAsync(d_z, z, zb, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_der, der, zb, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(ctx.iters.ptr, iters, ib, hipMemcpyHostToDevice, stream));
        HIP_TRY(fr_launch_colour_de_filter(p, d_z, static_cast<const uint32_t *>(ctx.iters.ptr), d_der, width, rows, supersample,
                                           ss_de_pixels(cfg, supersample), ts, (uint32_t)channels, d_out, stream, transfer));
        return FR_OK;
    });
}

int fr_colour_de_ss_rgb8(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, uint32_t width, uint32_t rows,
                         uint32_t supersample, double thickness, int channels, uint8_t *out, size_t out_len) {
    return fr_colour_de_ss_rgb8_tf(cfg, z, iters, der, width, rows, supersample, FR_SS_TRANSFER_BYTES, thickness, channels, out, out_len);
}

int fr_ss_de_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *min_bytes, size_t *best_bytes) {
    SsPlan pl;
    const int rc = ss_plan(cfg, supersample, y0, y1, pl, kDeSampleBytes);
    if (rc != FR_OK) return rc;
    if (min_bytes) *min_bytes = pl.min_bytes;
    if (best_bytes) *best_bytes = pl.best_bytes;
    return FR_OK;
}

int fr_render_rows_ss_de_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                int bits, double thickness, uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                size_t out_len, void *d_work, size_t work_len, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsDeRoad r;
    const int rc = ss_de_check(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_de_rows_device(cfg, r, supersample, transfer, y0, y1, channels, d_out, out_len, d_work, work_len, hip_stream);
}

int fr_render_rows_ss_de_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                int bits, double thickness, uint32_t supersample, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                size_t out_len, void *d_work, size_t work_len, void *hip_stream) {
    return fr_render_rows_ss_de_tf_device(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, d_out, out_len, d_work, work_len, hip_stream);
}

/* ---- SUPERSAMPLED SCALED DE: the two calls above on the scaled road, which fr_render_rows_ss_de keeps refusing ---------------- */

int fr_render_rows_ss_de_pt_scaled_tf_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                          uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                          void *d_work, size_t work_len, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsDeRoad r;
    const int rc = ss_de_scaled_check(cfg, centre, bits, thickness, supersample, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_de_rows_device(cfg, r, supersample, transfer, y0, y1, channels, d_out, out_len, d_work, work_len, hip_stream);
}

int fr_render_rows_ss_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                          uint32_t supersample, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                          void *d_work, size_t work_len, void *hip_stream) {
    return fr_render_rows_ss_de_pt_scaled_tf_device(cfg, centre, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, d_out, out_len, d_work, work_len, hip_stream);
}

int fr_render_rows_ss_de_pt_scaled_tf(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample, int transfer,
                                   uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsDeRoad r;
    const int rc = ss_de_scaled_check(cfg, centre, bits, thickness, supersample, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_de_rows_host(cfg, r, supersample, transfer, y0, y1, channels, out, out_len);
}

int fr_render_rows_ss_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample,
                                   uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    return fr_render_rows_ss_de_pt_scaled_tf(cfg, centre, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, out, out_len);
}

int fr_render_rows_ss_de_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                         double thickness, uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsDeRoad r;
    const int rc = ss_de_check(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_de_rows_host(cfg, r, supersample, transfer, y0, y1, channels, out, out_len);
}

int fr_render_rows_ss_de(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                         double thickness, uint32_t supersample, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    return fr_render_rows_ss_de_tf(cfg, precision, pos_lo, centre, road, bits, thickness, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, out, out_len);
}

} /* extern "C" */
