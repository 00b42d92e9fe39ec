/*
 * fr_ss_list.h — internal: what the pieces of ADAPTIVE SUPERSAMPLING (include/fractal_hip.h) share — the strided pixel map of
 * the probe pass, the edge list as a refine kernel sees it, the claim loop of the persistent refine waves, and the road
 * launches that fr_ss_adaptive.hip calls.  The refine kernels themselves sit beside their road's loop (fr_pt.hip, fr_bla.hip,
 * fr_scaled.hip; the F64 road's in fr_ss_adaptive.hip).  The device code here has internal linkage: each translation unit
 * compiles its own copy into its own kernels.
 */
#ifndef FR_SS_LIST_H
#define FR_SS_LIST_H

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
};

constexpr uint32_t kSsRefineThreads = 256; /* 4 waves; a wave claims on its own, the workgroup only shares the log2 table */

namespace {

/* The claim loop of one persistent wave.  Called by every lane of the wave, converged, AFTER the workgroup's last barrier: the
 * loop runs a different number of times per wave and holds none.  Each pass claims ppw entries with one atomic on the cursor
 * (lane 0; the answer is made wave-uniform, so the exit is taken by the whole wave); lane l takes sample l % s2 of entry
 * l / s2 — (i, j) = (k % s, k / s) of output pixel (X, Y) — and sample(x, y) returns the packed r | g << 8 | b << 16 of sample
 * pixel (x, y) of cfg_s.  Lanes with no sample (at or past ppw * s2, or past the count: the list is read only below it) skip
 * the orbit with 0 and rejoin for the shuffles, which every lane of the wave executes: the s2 triples of an entry are summed
 * by each of its lanes out of its neighbours' registers (integers: the order does not matter), and the entry's first lane
 * writes F over the probe bytes. */
template <class Sample>
__device__ __forceinline__ void ss_refine_loop(const fr_ss_refine &a, Sample &&sample) {
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
        uint32_t rb = a.half | a.half << 16, gg = a.half; /* r and b in the halves of one word: a sum is at most 64 * 255 + 32 */
        const uint32_t first = e * a.s2;
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

}  // namespace fr

#endif
