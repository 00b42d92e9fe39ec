/*
 * fr_ss_list.h — internal: what the pieces of ADAPTIVE SUPERSAMPLING (include/fractal_hip.h) share — the strided pixel map of
 * the probe pass, the mark pass's tile and its pieces, the edge list as a refine kernel sees it, the claim loop of the persistent refine waves, the one
 * launch of a refine kernel's JULIA x LINEAR instance, the DE probe over a road's launch (fr_de.h), and the road launches that
 * fr_ss_adaptive.hip and fr_ss_adaptive_de.hip call.  The refine kernels themselves sit beside their road's loop (fr_pt.hip, fr_bla.hip,
 * fr_scaled.hip; the F64 road's in fr_ss_adaptive.hip) — and ADAPTIVE SUPERSAMPLED DE's (fr_ss_adaptive_de.hip) beside their road's
 * DE loop (fr_de.hip, fr_de_bla.hip, fr_de_scaled.hip).  The device code here has internal linkage: each translation unit
 * compiles its own copy into its own kernels.
 */
#ifndef FR_SS_LIST_H
#define FR_SS_LIST_H

#include <type_traits>

#include "fr_ctx.h"

/* The probe's local grid on cfg_s: column X of local row r is sample (x_first + X * x_stride, y_first + r * y_stride) — the
 * strided map fr_kparams has, block_rows = 1 (fr_api.hip: fr_count_iterations sets it the same way). */
struct fr_ss_map {
    uint32_t ncols, nrows;
    uint32_t x_first, x_stride, y_first, y_stride;
    void apply(fr_kparams &p) const {
        p.ncols = ncols;
        p.nrows = nrows;
        p.x_first = x_first;
        p.x_stride = x_stride;
        p.y_first = y_first;
        p.y_stride = y_stride;
        p.block_rows = 1;
        p.out_in_place = 0;
        p.out_rgba = 0;
    }
};

/* The edge list and the output as a refine kernel sees them.  list[k], k < counters[0], is an edge pixel as row * width + X,
 * `row` counted from y0; counters[1] is the claim cursor (both zeroed on the stream by every call; the count is complete
 * before the refine kernel starts: ss_mark_kernel is the launch before it). */
struct fr_ss_refine {
    uint8_t *out;                  /* rows [y0, y1) of the output, bpp bytes a pixel: the probe colours, F written over them */
    const uint32_t *list;
    unsigned long long *counters;  /* [0] count, [1] claim cursor */
    uint32_t width;                /* of the output */
    uint32_t y0;                   /* the output row of list row 0 */
    uint32_t s, s2, ppw;           /* supersample; s * s; floor(64 / s2): entries a wave claims at a time */
    uint32_t bpp;                  /* 3 or 4 */
    uint32_t half, magic;          /* floor(s2 / 2); ceil(2^31 / s2): the box filter's division (fr_ss.hip) */
    uint32_t linear;               /* LINEAR-LIGHT SUPERSAMPLING: the launch takes the kernel's LINEAR instance (the host reads it) */
};

constexpr uint32_t kSsRefineThreads = 256; /* 4 waves; a wave claims on its own, the workgroup only shares the log2 table */

/* The thickness and the pixels of the distance shade as a DE refine kernel takes them (ADAPTIVE SUPERSAMPLED DE): Ts = T * s in
 * sample pixels and (double)(s * height) * min(|scale.re|, |scale.im|), what colour_de_rows_kernel is handed for cfg_s. */
struct fr_ss_de_shade {
    double pixels, thickness;
};

/* The mark pass's tile (ss_mark_kernel, ss_mark_de_kernel): one lane per output pixel, a wave = two tile rows, a one-pixel halo
 * around it in LDS as packed r | g << 8 | b << 16. */
constexpr uint32_t kMarkW = 32, kMarkH = 8;
constexpr uint32_t kMarkThreads = kMarkW * kMarkH;
constexpr uint32_t kMarkPitch = kMarkW + 2, kMarkHalo = kMarkPitch * (kMarkH + 2);
constexpr uint32_t kMarkOutside = 0xFFFFFFFFu; /* a halo position outside the image */

namespace {

#include "fr_srgb.h" /* LINEAR-LIGHT SUPERSAMPLING: the tables of the refine kernels' LINEAR instances */

/* ---- the mark pass's shared pieces ---- */

/* the probe colours of the tile at (X0, y0 + R0) with its halo into s_p; rows outside [ya, yb) and columns outside the width are
 * outside the IMAGE.  `probe` holds rows [ya, yb) as packed r,g,b.  The caller synchronises. */
__device__ __forceinline__ void ss_mark_stage(uint32_t *s_p, const uint8_t *probe, uint32_t width, uint32_t ya, uint32_t yb, uint32_t y0,
                                              uint32_t X0, uint32_t R0, uint32_t tid) {
    for (uint32_t k = tid; k < kMarkHalo; k += kMarkThreads) {
        const uint32_t hr = k / kMarkPitch, hc = k - hr * kMarkPitch;
        const int64_t X = (int64_t)X0 + hc - 1, Y = (int64_t)y0 + R0 + hr - 1; /* image coordinates */
        uint32_t v = kMarkOutside;
        if (X >= 0 && X < (int64_t)width && Y >= (int64_t)ya && Y < (int64_t)yb) {
            const uint8_t *c = probe + ((uint64_t)(Y - ya) * width + (uint64_t)X) * 3u;
            v = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
        }
        s_p[k] = v;
    }
}

__device__ __forceinline__ bool ss_mark_differs(uint32_t c, uint32_t n, int tau) {
    if (n == kMarkOutside) return false;
    const int dr = (int)(c & 0xFFu) - (int)(n & 0xFFu), dg = (int)(c >> 8 & 0xFFu) - (int)(n >> 8 & 0xFFu),
              db = (int)(c >> 16 & 0xFFu) - (int)(n >> 16 & 0xFFu);
    return abs(dr) > tau || abs(dg) > tau || abs(db) > tau;
}

/* the neighbour rule at `at`, the lane's own word in the staged tile: some of the 8 neighbours inside the image differs */
__device__ __forceinline__ bool ss_mark_neighbours(const uint32_t *at, int tau) {
    const uint32_t c = at[0];
    return ss_mark_differs(c, at[-(int)kMarkPitch - 1], tau) || ss_mark_differs(c, at[-(int)kMarkPitch], tau) ||
           ss_mark_differs(c, at[-(int)kMarkPitch + 1], tau) || ss_mark_differs(c, at[-1], tau) || ss_mark_differs(c, at[1], tau) ||
           ss_mark_differs(c, at[kMarkPitch - 1u], tau) || ss_mark_differs(c, at[kMarkPitch], tau) ||
           ss_mark_differs(c, at[kMarkPitch + 1u], tau);
}

/* P of pixel `px` (row * width + X, rows from y0) into the output */
__device__ __forceinline__ void ss_mark_write(uint8_t *out, uint32_t bpp, uint64_t px, uint32_t c) {
    if (bpp == 4u) {
        reinterpret_cast<uint32_t *>(out)[px] = c | 0xFF000000u;
    } else {
        uint8_t *o = out + 3ull * px;
        o[0] = (uint8_t)c;
        o[1] = (uint8_t)(c >> 8);
        o[2] = (uint8_t)(c >> 16);
    }
}

/* the wave's edge pixels onto the list: one ballot, one atomic (every lane of the wave is here) */
__device__ __forceinline__ void ss_mark_append(bool edge, uint32_t idx, uint32_t *list, unsigned long long *counters, uint32_t tid) {
    const unsigned long long mask = __ballot(edge);
    if (mask == 0ull) return; /* wave-uniform */
    const uint32_t lane = tid & 63u;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(counters, (unsigned long long)__builtin_popcountll(mask));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
    base = ((unsigned long long)hi << 32) | lo;
    if (edge) {
        const uint32_t rank = (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
        list[base + rank] = idx; /* < 2^32: the domain */
    }
}

/* The sRGB tables of a refine kernel's LINEAR instance in LDS (1 KiB), staged by the whole workgroup: call it before the barrier
 * that follows the log2 table's staging.  The byte instance has none. */
template <bool LINEAR>
__device__ __forceinline__ const uint16_t *ss_refine_tables() {
    if constexpr (LINEAR) {
        __shared__ uint16_t s_lt[kSrgbLdsWords];
        srgb_stage(s_lt, threadIdx.x, kSsRefineThreads);
        return s_lt;
    } else {
        return nullptr;
    }
}

/* The claim loop of one persistent wave. Called by every lane of the wave, converged, AFTER the workgroup's last barrier: the
 * loop runs a different number of times per wave and holds none.  Each pass claims ppw entries with one atomic on the cursor
 * (lane 0; the answer is made wave-uniform, so the exit is taken by the whole wave); lane l takes sample l % s2 of entry
 * l / s2 — (i, j) = (k % s, k / s) of output pixel (X, Y) — and sample(x, y) returns the packed r | g << 8 | b << 16 of sample
 * pixel (x, y) of cfg_s.  Lanes with no sample (at or past ppw * s2, or past the count: the list is read only below it) skip
 * the orbit with 0 and rejoin for the shuffles, which every lane of the wave executes: the s2 triples of an entry are summed
 * by each of its lanes out of its neighbours' registers (integers: the order does not matter), and the entry's first lane
 * writes F over the probe bytes.
 * LINEAR (LINEAR-LIGHT SUPERSAMPLING): s_lt is the workgroup's staged tables (fr_srgb.h: srgb_stage, before that last barrier).
 * Each lane decodes its own sample before the shuffles — L[r] | L[g] << 16 in one register, L[b] in another, two shuffles a
 * sample — the three sums (22 bits) have a register each, and the entry's first lane encodes the three quotients.  The byte
 * form does not read s_lt. */
template <bool LINEAR, class Sample>
__device__ __forceinline__ void ss_refine_loop(const fr_ss_refine &a, const uint16_t *s_lt, Sample &&sample) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long count = a.counters[0];
    const uint32_t e = lane / a.s2, k = lane - e * a.s2;
    const uint32_t j = k / a.s, i = k - j * a.s;
    for (;;) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.counters + 1, (unsigned long long)a.ppw);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
        base = ((unsigned long long)hi << 32) | lo;
        if (base >= count) break; /* wave-uniform */
        const bool live = e < a.ppw && base + e < count;
        uint32_t X = 0, row = 0, packed = 0;
        if (live) {
            const uint32_t idx = a.list[base + e];
            row = idx / a.width;
            X = idx - row * a.width;
            packed = sample((uint64_t)a.s * X + i, (uint64_t)a.s * ((uint64_t)a.y0 + row) + j);
        }
        const uint32_t first = e * a.s2;
        if constexpr (LINEAR) {
            const uint32_t lrg = srgb_decode(s_lt, packed & 0xFFu) | srgb_decode(s_lt, packed >> 8 & 0xFFu) << 16;
            const uint32_t lb = srgb_decode(s_lt, packed >> 16 & 0xFFu);
            uint32_t sr = a.half, sg = a.half, sb = a.half; /* a sum is at most 64 * 65535 + 32 */
            for (uint32_t t = 0; t < a.s2; t++) { /* uniform trip count; a source lane past 63 belongs to no entry */
                const int from = (int)((first + t) & 63u);
                const uint32_t v = (uint32_t)__shfl((int)lrg, from, 64);
                sr += v & 0xFFFFu;
                sg += v >> 16;
                sb += (uint32_t)__shfl((int)lb, from, 64);
            }
            if (live && k == 0) {
                const uint32_t cr = srgb_encode(s_lt, __umulhi(2u * sr, a.magic)), cg = srgb_encode(s_lt, __umulhi(2u * sg, a.magic)),
                               cb = srgb_encode(s_lt, __umulhi(2u * sb, a.magic));
                const uint64_t px = (uint64_t)row * a.width + X;
                if (a.bpp == 4u) {
                    reinterpret_cast<uint32_t *>(a.out)[px] = cr | cg << 8 | cb << 16 | 0xFF000000u;
                } else {
                    uint8_t *o = a.out + 3ull * px;
                    o[0] = (uint8_t)cr;
                    o[1] = (uint8_t)cg;
                    o[2] = (uint8_t)cb;
                }
            }
            continue;
        }
        uint32_t rb = a.half | a.half << 16, gg = a.half; /* r and b in the halves of one word: a sum is at most 64 * 255 + 32 */
        for (uint32_t t = 0; t < a.s2; t++) { /* uniform trip count; a source lane past 63 belongs to no entry */
            const uint32_t v = (uint32_t)__shfl((int)packed, (int)((first + t) & 63u), 64);
            rb += v & 0x00FF00FFu;
            gg += v >> 8 & 0xFFu;
        }
        if (live && k == 0) {
            const uint32_t cr = __umulhi(2u * (rb & 0xFFFFu), a.magic), cg = __umulhi(2u * gg, a.magic), cb = __umulhi(2u * (rb >> 16), a.magic);
            const uint64_t px = (uint64_t)row * a.width + X;
            if (a.bpp == 4u) {
                reinterpret_cast<uint32_t *>(a.out)[px] = cr | cg << 8 | cb << 16 | 0xFF000000u;
            } else {
                uint8_t *o = a.out + 3ull * px;
                o[0] = (uint8_t)cr;
                o[1] = (uint8_t)cg;
                o[2] = (uint8_t)cb;
            }
        }
    }
}

}  // namespace

namespace fr {

/* The road launches of the adaptive call on cfg_s (`cfg` below), arguments already checked, an escape-time algorithm for the
 * refine launches.  *_render_map: the road's existing RGB kernel over the probe's map into out.rgb (packed r,g,b), the sibling
 * of the row helpers, which build their grid from (y0, y1).  *_ss_refine: `groups` workgroups of the road's refine kernel.  The
 * orbit and the table are cfg's, from the context's caches: made by the probe, found by the refine.  PT's probe is launch_pt
 * (fr_ctx.h) itself. */
int pt_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, const fr_ss_refine &a, uint32_t groups, hipStream_t stream);
int bla_render_map(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_map &map, const fr_kout &out, hipStream_t stream);
int bla_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, uint32_t groups, hipStream_t stream);
int scaled_render_map(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_map &map, const fr_kout &out, hipStream_t stream);
int scaled_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, uint32_t groups, hipStream_t stream);

/* What the two adaptive calls share on the host (fr_ss_adaptive.hip).  ss_refine_args: the edge list of `rows` rows from y0 of
 * a width-wide output as a refine kernel takes it.  ss_refine_groups: the refine grid in workgroups — fr_debug_ss_adaptive_grid's
 * when one is set, else every wave slot of the device, capped by the most work the rows can hold (every pixel an edge, ppw
 * entries a claim, 4 waves a workgroup). */
fr_ss_refine ss_refine_args(uint8_t *out, const uint32_t *list, unsigned long long *counters, uint32_t width, uint32_t y0, uint32_t s,
                            uint32_t bpp, int transfer = 0);
uint32_t ss_refine_groups(const fr_ss_refine &a, uint32_t rows);

/* The launch of a refine kernel, written once for all eight: launch(J, L) is handed the kernel's JULIA and LINEAR template
 * arguments for the run-time `julia` and `linear` (a.linear) as std::true_type / std::false_type values, and launches
 * kernel<J(), L()>, or kernel<J(), BLA, L()> inside the scaled roads' branch on `bla`. */
template <class Launch>
void ss_refine_instance(bool julia, bool linear, Launch &&launch) {
    if (julia) {
        if (linear) launch(std::true_type{}, std::true_type{});
        else launch(std::true_type{}, std::false_type{});
    } else {
        if (linear) launch(std::false_type{}, std::true_type{});
        else launch(std::false_type{}, std::false_type{});
    }
}

/* ADAPTIVE SUPERSAMPLED DE's road launches (fr_ss_adaptive_de.hip calls them) on cfg_s (`cfg` below), arguments already checked.
 * de_render_map: the probe — a road's DE launch (fr_de.h: de_road) over the strided map, the sibling of de_render_rows, which
 * builds its grid from (y0, y1); no profiling events.  *_de_ss_refine: `groups` workgroups of the road's DE refine kernel, for an
 * escape-time algorithm; the orbit and the table are the context's, made by the probe.  The scaled road's: bits < 0 is the plain
 * scaled loop, no table, and sh.pixels is the scaled view's. */
template <class Road>
int de_render_map(Ctx &ctx, const fr_config *cfg, const fr_ss_map &map, double *d_z, uint32_t *d_iters, double *d_der, hipStream_t stream,
                  Road road) {
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    map.apply(p);
    const char *kname;
    return road(ctx, p, d_z, d_iters, d_der, stream, kname);
}
int de_ss_refine(Ctx &ctx, const fr_config *cfg, int precision, const Centre &c, const fr_ss_refine &a, const fr_ss_de_shade &sh,
                 uint32_t groups, hipStream_t stream);
int bla_de_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, const fr_ss_de_shade &sh,
                     uint32_t groups, hipStream_t stream);
int scaled_de_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, const fr_ss_de_shade &sh,
                        uint32_t groups, hipStream_t stream);

}  // namespace fr

#endif
