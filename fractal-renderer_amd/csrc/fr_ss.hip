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
 *   - the same on the deep roads (WIDE PT, BLA-PT, SCALED PT): fr_render_rows_ss_pt(_device), the band loop above with the
 *     road's own row launch in place of the precision's;
 *   - colour_filter_kernel / fr_launch_colour_filter and fr_colour_rows_ss_device / fr_colour_ss_rgb8: a KEPT anti-aliased
 *     view — (z, iters) of cfg_s in device memory — coloured and filtered in one kernel, no RGB workspace in between.
 *
 * The host plumbing is fr_ss.h's ("3.32"): the band loop ss_bands under render_ss_bands, ss_rows_device / ss_rows_host
 * behind fr_render_rows_ss_pt's checks and under fr_render_rows_ss's host form, host_rgb (fr_ctx.h) under the filter's and the
 * recolour's host forms.  fr_render_rows_ss_device keeps its own buffer rules: it looks at the output before the workspace.
 *
 * LINEAR-LIGHT SUPERSAMPLING (include/fractal_hip.h): every entry point here is a one-line forward to its _tf form, which holds
 * the body and takes `transfer`; FR_SS_TRANSFER_SRGB launches the LINEAR instance of the filter (fr_srgb.h: the two tables in
 * 1 KiB of LDS, a decode where the byte is read, three 22-bit sums, the same division, an eight-step bisection to encode).
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
#include "fr_bla.h" /* fr_ctx.h, and the BLA-PT / SCALED PT row launches */
#include "fr_ss.h"

#include <algorithm>
#include <atomic>

#include "fr_math.h"

namespace {

#include "fr_colour.h" /* the colour map of the renders: colour_filter_kernel's bytes are its bytes */
#include "fr_srgb.h"   /* LINEAR-LIGHT SUPERSAMPLING: the tables of the filters' LINEAR instances */

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

/* LINEAR (LINEAR-LIGHT SUPERSAMPLING) differs in phase 2 only: the two tables sit in 1 KiB of LDS behind the staged output rows
 * (staged before phase 1's barrier), a sample's byte is decoded as it is read, the three sums (22 bits) have a register each and
 * the quotient of the same division is encoded by srgb_encode.  The byte instance is the kernel as it was. */
template <bool LINEAR>
__global__ __launch_bounds__(kSsThreads) void box_filter_kernel(const ss_params p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint16_t *s_lt = nullptr;
    if constexpr (LINEAR) { /* behind the source rows and the output rows (both multiples of 16 bytes) */
        uint16_t *t = reinterpret_cast<uint16_t *>(lds + p.ro * p.s * ss_in_pitch(p.s) + p.ro * kSsOutPitch);
        srgb_stage(t, tid, kSsThreads);
        s_lt = t;
    }
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
                    if constexpr (LINEAR) {
                        sum[0] += srgb_decode(s_lt, q[3u * i]);
                        sum[1] += srgb_decode(s_lt, q[3u * i + 1u]);
                        sum[2] += srgb_decode(s_lt, q[3u * i + 2u]);
                    } else {
                        sum[0] += q[3u * i];
                        sum[1] += q[3u * i + 1u];
                        sum[2] += q[3u * i + 2u];
                    }
                }
            }
            uint32_t cr = __umulhi(2u * sum[0], p.magic), cg = __umulhi(2u * sum[1], p.magic), cb = __umulhi(2u * sum[2], p.magic);
            if constexpr (LINEAR) {
                cr = srgb_encode(s_lt, cr);
                cg = srgb_encode(s_lt, cg);
                cb = srgb_encode(s_lt, cb);
            }
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


/* ---- colour_filter_kernel: colour map + box filter over the stored results of cfg_s --------------------------------
 *
 * out = fr_box_filter_rgb8(fr_colour_rows(z, iters)) without the 3 * s * s bytes per output pixel in between.  Memory-bound:
 * 20 B (z_width 2) or 36 B (z_width 4; the low parts are skipped, not read) per sample in, 3 or 4 B per output pixel out.
 *   - a workgroup of 256 lanes owns a tile of kCfTileW = 64 output pixels x ro output rows (ro = 4, 2, 1 for s <= 4, <= 6,
 *     <= 8: one wave per output row), i.e. 64 s x s ro samples; it takes cf_tiles_per_group(s) tiles, a grid's width apart,
 *     so that the 3 KB log2 table — staged only when the colour map reads it — is paid once per >= 4096 samples;
 *   - phase 1: one sample per lane, four in flight: consecutive lanes load consecutive samples of a source row (16 B of z
 *     as two 8-byte loads — d_z is 8-byte aligned — and 4 B of iters each; a wave never straddles two rows), colour them
 *     with colour_of — the renders' own map — and park
 *     the packed r | g << 8 | b << 16 in LDS at [source row][sample]: 4 s s ro 64 bytes, 16 KiB at s = 4 and 8, 18 at 6;
 *   - phase 2, after one barrier: lane l of wave w sums the s x s block of output pixel (l, w): r and b together in the
 *     halves of one register, g in another; the LDS reads are 16 / 8 / 4 bytes wide for s % 4 == 0 / even / odd s (a lane's
 *     s samples of a row are contiguous and aligned to their own size).  + floor(s s / 2), then the division of
 *     box_filter_kernel: __umulhi(2 n, ceil(2^31 / (s s)));
 *   - RGBA leaves as one dword per lane; RGB through box_filter_kernel's staging: bytes to LDS at the destination row's
 *     address modulo 4, then aligned dwords (lanes 0 .. 47 of the row's wave) plus < 4 head and < 4 tail bytes (lanes 48 .. 53);
 *   - s is a template parameter (2 .. 8; s = 1 is colour_rows_kernel): every index above is a shift or a constant multiply;
 *   - 64-bit element offsets (a kept 3840 x 2160 view at s = 4 is 2.6 GB of z); plain vector loads and stores only. */
constexpr uint32_t kCfTileW = 64;                    /* output pixels per tile row: one wave */
constexpr uint32_t kCfThreads = 256;
constexpr uint32_t kCfOutPitch = 3 * kCfTileW + 16;  /* LDS bytes per staged RGB output row (3 spare + padding; a multiple of 4) */
__host__ __device__ constexpr uint32_t cf_tile_rows(uint32_t s) { return s <= 4 ? 4u : s <= 6 ? 2u : 1u; }
/* tiles per workgroup: at least 4096 samples behind one staging of the table */
constexpr uint32_t cf_tiles_per_group(uint32_t s) {
    const uint32_t per_tile = kCfTileW * s * s * cf_tile_rows(s);
    return (4096u + per_tile - 1u) / per_tile;
}

struct cf_params {
    const double *z;
    const uint32_t *iters;
    uint8_t *dst;
    uint64_t pitch;       /* s * width: samples per source row */
    uint32_t width, rows; /* of the output */
    uint32_t tiles_x, n_tiles;
    uint32_t zw, bpp;     /* doubles of z per sample (2 or 4); 3 or 4 */
};

/* kernel arguments re-read where the colour map needs them (fr_kernels.hip: FR_COLD_PARAMS; `p` is argument 0) */
typedef const __attribute__((address_space(4))) fr_kparams *CfKArgs;

struct cf_sample {
    double re, im;
    uint32_t iters;
    uint32_t at; /* the sample's LDS word, ~0u = none */
};

/* sample `idx` of the tile's flattened (source row, column) grid: loaded when it lies inside the image */
template <uint32_t S>
__device__ __forceinline__ cf_sample cf_load(uint32_t idx, uint32_t nsx, uint32_t nsy, const cf_params &q, uint64_t k00) {
    constexpr uint32_t SW = kCfTileW * S, N = SW * S * cf_tile_rows(S);
    cf_sample v{0.0, 0.0, 0u, ~0u};
    const uint32_t k = idx / SW, c = idx - k * SW;
    if (idx < N && k < nsy && c < nsx) {
        const uint64_t g = k00 + (uint64_t)k * q.pitch + c;
        if (q.zw == 2u) { /* uniform */
            v.re = q.z[2u * g];
            v.im = q.z[2u * g + 1u];
        } else {
            v.re = q.z[4u * g];
            v.im = q.z[4u * g + 2u];
        }
        v.iters = q.iters[g];
        v.at = idx;
    }
    return v;
}

__device__ __forceinline__ void cf_colour(const cf_sample &v, const double *s_tab, uint32_t *s_px) {
    if (v.at == ~0u) return;
    uint8_t rgb[3] = {0, 0, 0};
    CfKArgs kp = (CfKArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp)); /* opaque: the ~40 constants are loaded here, not held across the kernel */
    const ColourConsts cc = make_colour_consts(*kp);
    colour_of(cc, v.re * v.re + v.im * v.im, v.iters, s_tab, nullptr, rgb); /* pos.squared_distance(), :214 */
    s_px[v.at] = (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
}

/* LINEAR (LINEAR-LIGHT SUPERSAMPLING) differs in phase 2 only: the two tables are staged beside the log2 table (1 KiB more LDS), a
 * sample's three bytes are decoded as its word is read, the sums (22 bits) have a register each, and the quotients are encoded
 * by srgb_encode.  The byte instances are the kernel as it was. */
template <uint32_t S, bool LINEAR>
__global__ __launch_bounds__(kCfThreads) void colour_filter_kernel(const fr_kparams p, const cf_params q) {
    constexpr uint32_t RO = cf_tile_rows(S), SW = kCfTileW * S, N = SW * S * RO;
    constexpr uint32_t HALF = S * S / 2u, MAGIC = (uint32_t)(((1ull << 31) + S * S - 1u) / (S * S));
    __shared__ double s_tab[FR_LOG2_N * 3];
    __shared__ __attribute__((aligned(16))) uint32_t s_px[N];
    __shared__ uint32_t s_out_words[RO * kCfOutPitch / 4u];
    uint8_t *const s_out = reinterpret_cast<uint8_t *>(s_out_words);
    const uint32_t tid = threadIdx.x;
    const bool escape_algo = p.algo == 0 || p.algo == 2;
    if (escape_algo && p.smooth) { /* uniform */
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += kCfThreads) s_tab[k] = gt[k];
    }
    const uint16_t *s_lt = nullptr;
    if constexpr (LINEAR) {
        __shared__ uint16_t s_srgb[kSrgbLdsWords];
        srgb_stage(s_srgb, tid, kCfThreads);
        s_lt = s_srgb;
    }
    const uint32_t w = tid >> 6, l = tid & 63u; /* phase 2 and 3: output row of the tile, output pixel of the row */
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
        const uint32_t x0 = tx * kCfTileW, r0 = ty * RO;
        const uint32_t nx = min(kCfTileW, q.width - x0), nr = min(RO, q.rows - r0);
        __syncthreads(); /* the table is staged; the previous tile's rows have left s_out */

        /* ---- phase 1: samples -> colours -> LDS ---- */
        if (escape_algo) {
            const uint64_t k00 = (uint64_t)r0 * S * q.pitch + (uint64_t)x0 * S;
            const uint32_t nsx = nx * S, nsy = nr * S;
            for (uint32_t base = 0; base < N; base += 4u * kCfThreads) {
                const cf_sample v0 = cf_load<S>(base + tid, nsx, nsy, q, k00);
                const cf_sample v1 = cf_load<S>(base + kCfThreads + tid, nsx, nsy, q, k00);
                const cf_sample v2 = cf_load<S>(base + 2u * kCfThreads + tid, nsx, nsy, q, k00);
                const cf_sample v3 = cf_load<S>(base + 3u * kCfThreads + tid, nsx, nsy, q, k00);
                cf_colour(v0, s_tab, s_px);
                cf_colour(v1, s_tab, s_px);
                cf_colour(v2, s_tab, s_px);
                cf_colour(v3, s_tab, s_px);
            }
        }
        __syncthreads();

        /* ---- phase 2: one output pixel per lane ---- */
        const bool live = w < nr && l < nx;
        uint8_t *drow = q.dst + ((uint64_t)(r0 + (w < nr ? w : 0u)) * q.width + x0) * q.bpp; /* the wave's output row */
        const uint32_t dmis = q.bpp == 4u ? 0u : (uint32_t)(uintptr_t)drow & 3u;
        if (live) {
            [[maybe_unused]] uint32_t rb = HALF | HALF << 16, gg = HALF; /* r and b in the halves of one word: a sum is at most 64 * 255 + 32 */
            [[maybe_unused]] uint32_t lr = HALF, lg = HALF, lb = HALF;   /* LINEAR: a sum is at most 64 * 65535 + 32 */
            if (escape_algo) {
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
        if (q.bpp == 4u) continue; /* uniform */
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
}

template <uint32_t S>
hipError_t cf_launch(const fr_kparams &p, const cf_params &q, bool linear, hipStream_t stream) {
    const uint32_t groups = (q.n_tiles + cf_tiles_per_group(S) - 1u) / cf_tiles_per_group(S);
    if (linear) colour_filter_kernel<S, true><<<dim3(groups), dim3(kCfThreads), 0, stream>>>(p, q);
    else colour_filter_kernel<S, false><<<dim3(groups), dim3(kCfThreads), 0, stream>>>(p, q);
    return hipGetLastError();
}

}  // namespace

hipError_t fr_launch_box_filter(const void *src, uint32_t width, uint64_t rows, uint32_t s, uint32_t bpp, void *dst,
                                hipStream_t stream, int transfer) {
    if (width == 0 || rows == 0) return hipSuccess;
    if (s < 1 || s > FR_SS_MAX || (bpp != 3 && bpp != 4)) return hipErrorInvalidValue;
    const bool linear = transfer == FR_SS_TRANSFER_SRGB;
    ss_params p;
    p.src_pitch = (uint64_t)3u * s * width;
    p.width = width;
    p.s = s;
    p.ro = ss_tile_rows(s);
    p.tiles_x = (uint32_t)(((uint64_t)width + kSsThreads - 1) / kSsThreads);
    p.bpp = bpp;
    p.half = s * s / 2u;
    p.magic = (uint32_t)(((1ull << 31) + s * s - 1u) / (s * s));
    /* LINEAR: the output rows' place is kept for either bpp and the two tables lie behind it (51 216 bytes at s = 8) */
    const size_t lds_bytes = linear ? (size_t)p.ro * s * ss_in_pitch(s) + (size_t)p.ro * kSsOutPitch + kSrgbLdsWords * sizeof(uint16_t)
                                    : (size_t)p.ro * s * ss_in_pitch(s) + (bpp == 3 ? (size_t)p.ro * kSsOutPitch : 0u);
    /* launches of at most 2^30 workgroups (whole tile rows) */
    const uint64_t rows_per_launch = std::max<uint64_t>(1, (1ull << 30) / p.tiles_x) * p.ro;
    for (uint64_t ra = 0; ra < rows; ra += rows_per_launch) {
        const uint64_t n = std::min(rows - ra, rows_per_launch);
        if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
        p.src = static_cast<const uint8_t *>(src) + ra * s * p.src_pitch;
        p.dst = static_cast<uint8_t *>(dst) + ra * width * bpp;
        p.rows = (uint32_t)n;
        const uint64_t tiles = (uint64_t)p.tiles_x * ((n + p.ro - 1) / p.ro);
        if (linear) box_filter_kernel<true><<<dim3((uint32_t)tiles), dim3(kSsThreads), lds_bytes, stream>>>(p);
        else box_filter_kernel<false><<<dim3((uint32_t)tiles), dim3(kSsThreads), lds_bytes, stream>>>(p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t fr_launch_colour_filter(const fr_kparams &p, const double *z, uint32_t z_width, const uint32_t *iters, uint32_t width,
                                   uint64_t rows, uint32_t s, uint32_t bpp, void *dst, hipStream_t stream, int transfer) {
    if (width == 0 || rows == 0) return hipSuccess;
    if (s < 1 || s > FR_SS_MAX || (bpp != 3 && bpp != 4) || (z_width != 2 && z_width != 4)) return hipErrorInvalidValue;
    const bool linear = transfer == FR_SS_TRANSFER_SRGB;
    if (s == 1) return fr_launch_colour_rows(p, z, z_width, iters, (size_t)width * rows, bpp, dst, stream); /* nothing to filter */
    cf_params q;
    q.pitch = (uint64_t)s * width;
    q.width = width;
    q.tiles_x = (uint32_t)(((uint64_t)width + kCfTileW - 1) / kCfTileW);
    q.zw = z_width;
    q.bpp = bpp;
    const uint32_t ro = cf_tile_rows(s);
    /* launches of at most 2^30 tiles (whole tile rows) */
    const uint64_t rows_per_launch = std::max<uint64_t>(1, (1ull << 30) / q.tiles_x) * ro;
    for (uint64_t ra = 0; ra < rows; ra += rows_per_launch) {
        const uint64_t n = std::min(rows - ra, rows_per_launch);
        const uint64_t first = ra * s * q.pitch; /* the launch's first sample */
        q.z = z + first * z_width;
        q.iters = iters + first;
        q.dst = static_cast<uint8_t *>(dst) + ra * width * bpp;
        q.rows = (uint32_t)n;
        q.n_tiles = (uint32_t)(q.tiles_x * ((n + ro - 1) / ro));
        hipError_t e;
        switch (s) {
        case 2: e = cf_launch<2>(p, q, linear, stream); break;
        case 3: e = cf_launch<3>(p, q, linear, stream); break;
        case 4: e = cf_launch<4>(p, q, linear, stream); break;
        case 5: e = cf_launch<5>(p, q, linear, stream); break;
        case 6: e = cf_launch<6>(p, q, linear, stream); break;
        case 7: e = cf_launch<7>(p, q, linear, stream); break;
        default: e = cf_launch<8>(p, q, linear, stream); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace fr {

static std::atomic<size_t> g_host_work_cap{0}; /* fr_debug_ss_host_work_cap: 0 = kSsHostWorkCap */

size_t ss_host_work_cap() {
    const size_t cap = g_host_work_cap.load();
    return cap ? cap : kSsHostWorkCap;
}

int check_transfer(int transfer) {
    if (transfer != FR_SS_TRANSFER_BYTES && transfer != FR_SS_TRANSFER_SRGB)
        return fail(FR_ERR_INVALID_ARGUMENT, "transfer must be FR_SS_TRANSFER_BYTES (0) or FR_SS_TRANSFER_SRGB (1)");
    return FR_OK;
}

/* the part of the domain that needs no precision: cfg, s, the sizes, the rows (fr_ss.h) */
int ss_plan(const fr_config *cfg, uint32_t s, uint32_t y0, uint32_t y1, SsPlan &pl, uint32_t sample_bytes) {
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
    pl.row_bytes = (uint64_t)sample_bytes * s * cfg->width;
    if (s == 1 && sample_bytes == 3u) {
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

namespace {

/* The packed-RGB bands of fr_render_rows_ss and fr_render_rows_ss_pt: ss_bands (fr_ss.h) with the box filter behind each band.
 * band(ctx, ya, yb, ko, stream) is the launch of source rows [ya, yb) of cfg_s as packed r,g,b into ko.rgb, the workspace;
 * s >= 2. */
template <class Band>
int render_ss_bands(Ctx &ctx, const SsPlan &pl, uint32_t s, int transfer, uint32_t y0, unsigned bpp, void *d_out, void *d_work, size_t work_len,
                    hipStream_t stream, int pending_sample, Band &&band) {
    const uint32_t width = pl.cfg_s.width / s;
    fr_kout ko{};
    ko.rgb = static_cast<uint8_t *>(d_work);
    return ss_bands(ctx, pl, s, y0, bpp, d_out, work_len, stream, pending_sample,
                    [&](Ctx &c, uint32_t ya, uint32_t yb, uint8_t *dst, uint32_t out_rows, hipStream_t st) {
                        const int rc = band(c, ya, yb, ko, st);
                        if (rc != FR_OK) return rc;
                        const hipError_t e = fr_launch_box_filter(d_work, width, out_rows, s, bpp, dst, st, transfer);
                        return e == hipSuccess ? FR_OK : fail_hip(e, "fr_launch_box_filter");
                    });
}

/* the bands of fr_render_rows_ss(_device): the precision's own row render */
int render_ss_device(Ctx &ctx, const SsPlan &pl, int precision, const fr_imaginary *pos_lo, uint32_t s, int transfer, uint32_t y0,
                     unsigned bpp, void *d_out, void *d_work, size_t work_len, hipStream_t stream, const Opts &o) {
    const fr_config *cs = &pl.cfg_s;
    const bool deep = precision == FR_PRECISION_DD || precision == FR_PRECISION_PT;
    Opts ob = o;
    if (!deep) /* ONE choice for every band, as the host path's bands */
        decide_kernel(ctx, cs, precision, s * y0, (uint32_t)(s * y0 + pl.src_rows), ob, stream, true);
    const int pending_sample = ob.pending_sample;
    ob.pending_sample = -1;
    return render_ss_bands(ctx, pl, s, transfer, y0, bpp, d_out, d_work, work_len, stream, pending_sample,
                           [&](Ctx &c, uint32_t ya, uint32_t yb, const fr_kout &ko, hipStream_t st) {
                               if (deep) return render_deep_device(c, precision, cs, Centre{pos_lo, nullptr}, o, ya, yb, 3, ko.rgb, st);
                               fr_kparams p;
                               rows_params(cs, ob, ya, yb, 3, p);
                               return render_device(c, cs, p, precision, ob, ko.rgb, st);
                           });
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

/* ---- the deep roads, supersampled (include/fractal_hip.h, "supersampled rendering on the deep roads") ------------------- */

/* what fr_render_rows_ss_pt(_device) have checked: the plan, the road's centre and its resolved bits */
struct SsRoad {
    SsPlan pl;
    Centre c;
    int road, bits;
    Opts o; /* PLAIN: render_deep_device's */
    /* rows [ya, yb) of `cfg` (cfg_s for a band, the caller's cfg for s = 1) on the road */
    int rows(Ctx &ctx, const fr_config *cfg, uint32_t ya, uint32_t yb, unsigned channels, const fr_kout &ko, hipStream_t stream) const {
        if (road == FR_PT_ROAD_BLA) return bla_render_rows(ctx, cfg, c, bits, ya, yb, channels, ko, stream);
        if (road == FR_PT_ROAD_SCALED) return scaled_render_rows(ctx, cfg, c, bits, ya, yb, channels, ko, stream);
        return render_deep_device(ctx, FR_PRECISION_PT, cfg, c, o, ya, yb, channels, ko.rgb, stream);
    }
};

/* everything fr_render_rows_ss_pt(_device) check before any device work: the sizes, then the road's own domain on cfg_s */
int ss_road_check(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits, uint32_t s,
                  uint32_t y0, uint32_t y1, int channels, SsRoad &r) {
    int rc = ss_plan(cfg, s, y0, y1, r.pl);
    if (rc == FR_OK) rc = check_channels(channels);
    if (rc != FR_OK) return rc;
    const fr_config *cs = &r.pl.cfg_s;
    const uint32_t Y0 = s * y0, Y1 = (uint32_t)(Y0 + r.pl.src_rows);
    r.road = road;
    r.bits = bits;
    switch (road) {
    case FR_PT_ROAD_PLAIN:
        if (bits != 0) return fail(FR_ERR_INVALID_ARGUMENT, "bits must be 0 with FR_PT_ROAD_PLAIN: the plain loop has no table");
        if (centre && pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "pos_lo must be NULL when a wide centre is given");
        r.c = Centre{pos_lo, centre};
        rc = r.c.check(cs, FR_PRECISION_PT);
        if (rc == FR_OK) rc = resolve_opts(nullptr, r.o);
        return rc;
    case FR_PT_ROAD_BLA:
        r.c = Centre{pos_lo, centre};
        return bla_check(cs, r.c, r.bits, Y0, Y1);
    case FR_PT_ROAD_SCALED:
        if (pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: pos_lo must be NULL, the centre is the wide centre");
        r.c = Centre{nullptr, centre, true};
        return scaled_check(cs, r.c, r.bits, Y0, Y1);
    default:
        return fail(FR_ERR_INVALID_ARGUMENT, "road must be FR_PT_ROAD_PLAIN (0), FR_PT_ROAD_BLA (1) or FR_PT_ROAD_SCALED (2)");
    }
}

/* rows [y0, y1) of cfg on the road into ko.rgb: s = 1 the road's plain render, byte for byte; else its bands of cfg_s through
 * the workspace, each filtered into place */
int ss_road_rows(Ctx &ctx, const SsRoad &r, const fr_config *cfg, uint32_t s, int transfer, uint32_t y0, uint32_t y1, unsigned bpp, const fr_kout &ko,
                 void *d_work, size_t work_len, hipStream_t stream) {
    if (s == 1) return r.rows(ctx, cfg, y0, y1, bpp, ko, stream);
    return render_ss_bands(ctx, r.pl, s, transfer, y0, bpp, ko.rgb, d_work, work_len, stream, -1,
                           [&](Ctx &c, uint32_t ya, uint32_t yb, const fr_kout &band, hipStream_t st) {
                               return r.rows(c, &r.pl.cfg_s, ya, yb, 3, band, st);
                           });
}

/* the domain of fr_colour_rows_ss_device / fr_colour_ss_rgb8 short of the buffers */
int colour_ss_check(const fr_config *cfg, int z_width, uint32_t width, uint32_t rows, uint32_t s, int channels) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (z_width != 2 && z_width != 4) return fail(FR_ERR_INVALID_ARGUMENT, "z_width must be 2 (re, im) or 4 (re.hi, re.lo, im.hi, im.lo)");
    return box_filter_check(width, rows, s, channels);
}

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

int fr_ss_transfer_tables(fr_ss_table *decode256, fr_ss_table *thresholds255) {
    static const uint16_t decode[256] = FR_SRGB_DECODE_INIT;
    static const uint16_t thresholds[255] = FR_SRGB_THRESHOLD_INIT;
    if (decode256) *decode256 = decode;
    if (thresholds255) *thresholds255 = thresholds;
    return FR_OK;
}

int fr_debug_ss_host_work_cap(size_t bytes) {
    if (bytes & 7u) return fail(FR_ERR_INVALID_ARGUMENT, "bytes must be 0 (the default cap of 256 MiB) or a multiple of 8");
    g_host_work_cap.store(bytes);
    return FR_OK;
}

int fr_ss_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *min_bytes,
                          size_t *best_bytes) {
    SsPlan pl;
    const int rc = ss_plan(cfg, supersample, y0, y1, pl);
    if (rc != FR_OK) return rc;
    if (min_bytes) *min_bytes = pl.min_bytes;
    if (best_bytes) *best_bytes = pl.best_bytes;
    return FR_OK;
}

int fr_render_rows_ss_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, int transfer,
                             uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work,
                             size_t work_len, void *hip_stream, const fr_render_opts *opts) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
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
        return render_ss_device(ctx, pl, precision, pos_lo, supersample, transfer, y0, (unsigned)channels, d_out, d_work, work_len, stream, o);
    });
}

int fr_render_rows_ss_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample,
                             uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work,
                             size_t work_len, void *hip_stream, const fr_render_opts *opts) {
    return fr_render_rows_ss_tf_device(cfg, precision, pos_lo, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, d_out, out_len, d_work, work_len, hip_stream, opts);
}

int fr_render_rows_ss_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, int transfer, uint32_t y0,
                      uint32_t y1, int channels, uint8_t *out, size_t out_len, const fr_render_opts *opts) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
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
    return ss_rows_host(cfg, ss_host_work_len(pl), y0, y1, channels, out, out_len,
                        [&](Ctx &ctx, const fr_kout &ko, void *d_work, size_t work_len, hipStream_t stream) {
                            return render_ss_device(ctx, pl, precision, pos_lo, supersample, transfer, y0, (unsigned)channels, ko.rgb, d_work, work_len, stream, o);
                        });
}

int fr_render_rows_ss(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, uint32_t y0,
                      uint32_t y1, int channels, uint8_t *out, size_t out_len, const fr_render_opts *opts) {
    return fr_render_rows_ss_tf(cfg, precision, pos_lo, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, out, out_len, opts);
}

int fr_box_filter_rgb8_tf_device(const void *d_src, uint32_t width, uint32_t rows, uint32_t supersample, int transfer, int channels,
                              void *d_out, size_t out_len, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    const int rc = box_filter_check(width, rows, supersample, channels);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!d_src || !d_out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (d_src, d_out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output (d_out) must be 4-byte aligned");
    HIP_TRY(fr_launch_box_filter(d_src, width, rows, supersample, (uint32_t)channels, d_out, static_cast<hipStream_t>(hip_stream), transfer));
    return FR_OK;
}

int fr_box_filter_rgb8_device(const void *d_src, uint32_t width, uint32_t rows, uint32_t supersample, int channels,
                              void *d_out, size_t out_len, void *hip_stream) {
    return fr_box_filter_rgb8_tf_device(d_src, width, rows, supersample, FR_SS_TRANSFER_BYTES, channels, d_out, out_len, hip_stream);
}

int fr_box_filter_rgb8_tf(const uint8_t *src, uint32_t width, uint32_t rows, uint32_t supersample, int transfer, int channels, uint8_t *out,
                       size_t out_len) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    int rc = box_filter_check(width, rows, supersample, channels);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!src || !out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (src, out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    const size_t src_bytes = (size_t)3u * supersample * width * ((size_t)supersample * rows);
    return host_rgb(out, need, [&](Ctx &ctx, void *d_out, hipStream_t stream) -> int {
        const int rc = ctx.reserve(ctx.ss_work, src_bytes);
        if (rc != FR_OK) return rc;
        HIP_TRY(hipMemcpyAsync(ctx.ss_work.ptr, src, src_bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(fr_launch_box_filter(ctx.ss_work.ptr, width, rows, supersample, (uint32_t)channels, d_out, stream, transfer));
        return FR_OK;
    });
}

int fr_box_filter_rgb8(const uint8_t *src, uint32_t width, uint32_t rows, uint32_t supersample, int channels, uint8_t *out,
                       size_t out_len) {
    return fr_box_filter_rgb8_tf(src, width, rows, supersample, FR_SS_TRANSFER_BYTES, channels, out, out_len);
}

int fr_render_rows_ss_pt_tf_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                                uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                void *d_work, size_t work_len, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsRoad r;
    const int rc = ss_road_check(cfg, pos_lo, centre, road, bits, supersample, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_rows_device(cfg, r.pl, "work_len < min_bytes of fr_ss_workspace_bytes", false, y0, y1, channels, d_out, out_len, d_work, work_len,
                          hip_stream, [&](Ctx &ctx, const fr_kout &ko, void *work, size_t len, hipStream_t stream) {
                              return ss_road_rows(ctx, r, cfg, supersample, transfer, y0, y1, (unsigned)channels, ko, work, len, stream);
                          });
}

int fr_render_rows_ss_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                                uint32_t supersample, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                void *d_work, size_t work_len, void *hip_stream) {
    return fr_render_rows_ss_pt_tf_device(cfg, pos_lo, centre, road, bits, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, d_out, out_len, d_work, work_len, hip_stream);
}

int fr_render_rows_ss_pt_tf(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                         uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    SsRoad r;
    const int rc = ss_road_check(cfg, pos_lo, centre, road, bits, supersample, y0, y1, channels, r);
    if (rc != FR_OK) return rc;
    return ss_rows_host(cfg, ss_host_work_len(r.pl), y0, y1, channels, out, out_len, /* s = 1: a plan of 0 bytes */
                        [&](Ctx &ctx, const fr_kout &ko, void *work, size_t len, hipStream_t stream) {
                            return ss_road_rows(ctx, r, cfg, supersample, transfer, y0, y1, (unsigned)channels, ko, work, len, stream);
                        });
}

int fr_render_rows_ss_pt(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                         uint32_t supersample, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len) {
    return fr_render_rows_ss_pt_tf(cfg, pos_lo, centre, road, bits, supersample, FR_SS_TRANSFER_BYTES, y0, y1, channels, out, out_len);
}

int fr_colour_rows_ss_tf_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, uint32_t width, uint32_t rows,
                             uint32_t supersample, int transfer, int channels, void *d_out, size_t out_len, void *hip_stream) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    const int rc = colour_ss_check(cfg, z_width, width, rows, supersample, channels);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!d_z || !d_iters || !d_out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (d_z, d_iters, d_out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    if ((reinterpret_cast<uintptr_t>(d_z) & 7u) || (reinterpret_cast<uintptr_t>(d_iters) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "d_z must be 8-byte aligned and d_iters 4-byte aligned");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output (d_out) must be 4-byte aligned");
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    HIP_TRY(fr_launch_colour_filter(p, static_cast<const double *>(d_z), (uint32_t)z_width, static_cast<const uint32_t *>(d_iters), width,
                                    rows, supersample, (uint32_t)channels, d_out, static_cast<hipStream_t>(hip_stream), transfer));
    return FR_OK;
}

int fr_colour_rows_ss_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, uint32_t width, uint32_t rows,
                             uint32_t supersample, int channels, void *d_out, size_t out_len, void *hip_stream) {
    return fr_colour_rows_ss_tf_device(cfg, d_z, z_width, d_iters, width, rows, supersample, FR_SS_TRANSFER_BYTES, channels, d_out, out_len, hip_stream);
}

int fr_colour_ss_rgb8_tf(const fr_config *cfg, const double *z, int z_width, const uint32_t *iters, uint32_t width, uint32_t rows,
                      uint32_t supersample, int transfer, int channels, uint8_t *out, size_t out_len) {
    if (const int trc = check_transfer(transfer); trc != FR_OK) return trc;
    int rc = colour_ss_check(cfg, z_width, width, rows, supersample, channels);
    if (rc != FR_OK) return rc;
    const size_t need = (size_t)channels * width * (size_t)rows;
    if (need == 0) return FR_OK;
    if (!z || !iters || !out) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array (z, iters, out)");
    if (out_len < need) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*rows");
    const size_t n = (size_t)supersample * width * ((size_t)supersample * rows);
    const size_t zb = n * (size_t)z_width * sizeof(double), ib = n * sizeof(uint32_t);
    return host_rgb(out, need, [&](Ctx &ctx, void *d_out, hipStream_t stream) -> int {
        int rc = ctx.reserve(ctx.z, zb);
        if (rc == FR_OK) rc = ctx.reserve(ctx.iters, ib);
        if (rc != FR_OK) return rc;
        fr_kparams p;
        fill_params(cfg, default_opts(), p);
        HIP_TRY(hipMemcpyAsync(ctx.z.ptr, z, zb, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(ctx.iters.ptr, iters, ib, hipMemcpyHostToDevice, stream));
        HIP_TRY(fr_launch_colour_filter(p, static_cast<const double *>(ctx.z.ptr), (uint32_t)z_width, static_cast<const uint32_t *>(ctx.iters.ptr),
                                        width, rows, supersample, (uint32_t)channels, d_out, stream, transfer));
        return FR_OK;
    });
}

int fr_colour_ss_rgb8(const fr_config *cfg, const double *z, int z_width, const uint32_t *iters, uint32_t width, uint32_t rows,
                      uint32_t supersample, int channels, uint8_t *out, size_t out_len) {
    return fr_colour_ss_rgb8_tf(cfg, z, z_width, iters, width, rows, supersample, FR_SS_TRANSFER_BYTES, channels, out, out_len);
}

} /* extern "C" */
