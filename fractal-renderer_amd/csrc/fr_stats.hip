/*
 * fr_stats.hip — escape-index statistics of a kept view, reduced on the device (include/fractal_hip.h, "statistics of a
 * kept view"): class counts, min / max / sum and a 1024-bin histogram of the escape indices, and the two host helpers
 * that turn the record into a percentile and into an exposure for the colour map.
 *
 * The record is DEFINED in the header; every field is an integer function of the input, so the kernels below may add in
 * any order.  A memset and two launches on the caller's stream, no host read between them:
 *
 *   hipMemsetAsync          the record to zero, whatever it held.
 *   view_stats_range_kernel class counts, sum, min and max.  A workgroup of 1024 lanes walks tiles of 4096 pixels, a grid's
 *                           width apart: a lane a pixel, four pixels per lane in flight (z as one 16-byte load for z_width
 *                           2, the two hi parts as 8-byte loads for z_width 4), running values in registers; then a
 *                           reduction across the wave (cross-lane moves), across the sixteen waves through LDS, and ONE set
 *                           of global atomics per workgroup.  While the kernel runs, min_iters holds the COMPLEMENT of the
 *                           minimum, gathered with atomicMax: zero is then the neutral element of every field and the
 *                           memset is the whole initialisation.
 *   view_stats_hist_kernel  reads min / max, derives `shift`, classifies the pixels again (the same two multiplications
 *                           and one addition) and bins class E into a per-workgroup LDS histogram of 1024 32-bit
 *                           counters; non-zero bins leave with 64-bit global atomics.  A deep view is the bad case for
 *                           atomics — large areas escape at one index and hit one bin (same-address atomics run at 88 M/s
 *                           where 64 addresses take 4.1 G/s: profiles/r02_atomic_rates.txt) — so a wave first peels its
 *                           pixels by bin: the lanes that agree with the first active lane's bin (one readfirstlane
 *                           comparison and a ballot) are added as ONE popcount; two such rounds, then whoever is left
 *                           adds 1 by itself.  The last workgroup to finish (a ticket in `reserved`, which it puts back to
 *                           0) writes `shift` and turns the complement into min_iters, or min = max = 0 when E is empty.
 *
 * The grid is min(ceil(n / 4096), kStatsMaxGroups) workgroups, and never fewer than n / 2^31: a workgroup bins at most
 * 2^31 pixels (+ a tile), so a 32-bit LDS counter cannot wrap, nor can a lane's 32-bit class count (n <= 2^40 is part of
 * the domain: at most 512 workgroups).
 */
#include "fr_ctx.h"

#include <cmath>
#include <cstring>

namespace {

constexpr uint32_t kStatsThreads = 1024;
constexpr uint32_t kStatsPerLane = 4;
constexpr uint32_t kStatsTile = kStatsThreads * kStatsPerLane; /* pixels a workgroup takes per step */
/* One workgroup of 16 waves per compute unit.  The record is one or two cache lines for every workgroup's atomics, which the
 * memory side takes one after the other: 1024 workgroups of 256 lanes with six atomics each were measured at 54 us for the
 * range kernel on a 1080p view whose 41 MB stream in 10 */
constexpr uint32_t kStatsMaxGroups = 256;
constexpr size_t kStatsMaxN = (size_t)1 << 40;

static_assert(sizeof(struct fr_view_stats) == 8248, "fr_view_stats is part of the ABI");
static_assert(FR_STATS_BINS == kStatsThreads, "a lane zeroes and flushes one bin");

/* 16 bytes in one load from an address that is only 8-byte aligned */
typedef double stats_z2 __attribute__((ext_vector_type(2), aligned(8)));

struct StatsPixel {
    double re, im;
    uint32_t it;
};

/* pixel k's position as the colour map reads it, and its escape index */
__device__ __forceinline__ StatsPixel stats_load(const double *z, const uint32_t zw, const uint32_t *iters, const size_t k) {
    StatsPixel px;
    if (zw == 2u) {
        const stats_z2 v = *reinterpret_cast<const stats_z2 *>(z + 2 * k);
        px.re = v.x;
        px.im = v.y;
    } else {
        px.re = z[4 * k];
        px.im = z[4 * k + 2];
    }
    px.it = iters[k];
    return px;
}

/* 0 = S (stable), 1 = C (capped), 2 = E (escaped): the colour map's own branches (fr_colour.h: colour_of) */
__device__ __forceinline__ uint32_t stats_class(const StatsPixel &px, const double stable_limit, const uint32_t iterations) {
    const double dist = px.re * px.re + px.im * px.im; /* pos.squared_distance(), as colour_rows_kernel forms it */
    if (!(dist > stable_limit)) return 0u;
    return px.it >= iterations ? 1u : 2u;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kStatsThreads) void view_stats_range_kernel(const double *z, const uint32_t zw, const uint32_t *iters,
                                                                        const size_t n, const double stable_limit,
                                                                        const uint32_t iterations, struct fr_view_stats *stats) {
    __shared__ unsigned long long s_part[kStatsThreads / 64][6];
    uint32_t n_s = 0, n_c = 0, n_e = 0, not_min = 0, max_it = 0; /* not_min = ~min over E, 0 while the lane has none */
    unsigned long long sum = 0;
    for (size_t base = (size_t)blockIdx.x * kStatsTile; base < n; base += (size_t)gridDim.x * kStatsTile) {
        StatsPixel px[kStatsPerLane];
        bool valid[kStatsPerLane];
#pragma unroll
        for (uint32_t j = 0; j < kStatsPerLane; j++) {
            const size_t k = base + j * kStatsThreads + threadIdx.x;
            valid[j] = k < n;
            px[j] = stats_load(z, zw, iters, valid[j] ? k : n - 1); /* an in-bounds load either way: four in flight */
        }
#pragma unroll
        for (uint32_t j = 0; j < kStatsPerLane; j++) {
            if (!valid[j]) continue;
            const uint32_t cls = stats_class(px[j], stable_limit, iterations);
            n_s += cls == 0u;
            n_c += cls == 1u;
            if (cls == 2u) {
                n_e++;
                sum += px[j].it;
                not_min = max(not_min, ~px[j].it); /* it < iterations <= 2^32 - 1, so ~it >= 1 */
                max_it = max(max_it, px[j].it);
            }
        }
    }
    n_s = wave_sum(n_s);
    n_c = wave_sum(n_c);
    n_e = wave_sum(n_e);
    sum = wave_sum(sum);
    not_min = wave_max(not_min);
    max_it = wave_max(max_it);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_part[wave][0] = n_s;
        s_part[wave][1] = n_c;
        s_part[wave][2] = n_e;
        s_part[wave][3] = sum;
        s_part[wave][4] = not_min;
        s_part[wave][5] = max_it;
    }
    __syncthreads();
    if (wave != 0u) return;
    /* the first wave reduces the waves' partials, a lane a wave (one lane walking all 16 x 6 of them unrolls into 48 LDS
     * reads in flight, which under this kernel's 128-register cap spilled to scratch) */
    const uint32_t w = threadIdx.x;
    const bool has = w < kStatsThreads / 64;
    const unsigned long long t_s = wave_sum(has ? s_part[w][0] : 0ull), t_c = wave_sum(has ? s_part[w][1] : 0ull);
    const unsigned long long t_e = wave_sum(has ? s_part[w][2] : 0ull), t_sum = wave_sum(has ? s_part[w][3] : 0ull);
    const uint32_t t_not_min = wave_max(has ? (uint32_t)s_part[w][4] : 0u), t_max = wave_max(has ? (uint32_t)s_part[w][5] : 0u);
    if (threadIdx.x != 0u) return;
    if (blockIdx.x == 0u) stats->n = n; /* nobody else writes it */
    if (t_s) atomicAdd(reinterpret_cast<unsigned long long *>(&stats->stable), t_s);
    if (t_c) atomicAdd(reinterpret_cast<unsigned long long *>(&stats->capped), t_c);
    if (t_e) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&stats->escaped), t_e);
        atomicAdd(reinterpret_cast<unsigned long long *>(&stats->sum_iters), t_sum);
        atomicMax(&stats->min_iters, t_not_min);
        atomicMax(&stats->max_iters, t_max);
    }
}

/* the smallest s >= 0 with range >> s < FR_STATS_BINS */
__host__ __device__ inline uint32_t stats_shift(const uint32_t range) {
    uint32_t s = 0;
    while ((range >> s) >= (uint32_t)FR_STATS_BINS) s++;
    return s;
}

__global__ __launch_bounds__(kStatsThreads) void view_stats_hist_kernel(const double *z, const uint32_t zw, const uint32_t *iters,
                                                                       const size_t n, const double stable_limit,
                                                                       const uint32_t iterations, struct fr_view_stats *stats) {
    __shared__ uint32_t s_hist[FR_STATS_BINS];
    /* What view_stats_range_kernel left.  These three loads must stay HERE, above the first barrier: the last workgroup
     * rewrites min_iters once every workgroup has drawn its ticket below, and the only thing that orders that store behind
     * the other workgroups' loads is that each has used the loaded values (to bin) before its own ticket.  A re-read of
     * stats->min_iters further down, or a last workgroup that reads `hist`, would need a release / acquire hand-over. */
    const bool any = stats->escaped != 0ull;
    const uint32_t min_it = ~stats->min_iters, max_it = stats->max_iters;
    const uint32_t shift = any ? stats_shift(max_it - min_it) : 0u;
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    if (any) { /* uniform */
        for (size_t base = (size_t)blockIdx.x * kStatsTile; base < n; base += (size_t)gridDim.x * kStatsTile) {
            StatsPixel px[kStatsPerLane];
            bool valid[kStatsPerLane];
#pragma unroll
            for (uint32_t j = 0; j < kStatsPerLane; j++) {
                const size_t k = base + j * kStatsThreads + threadIdx.x;
                valid[j] = k < n;
                px[j] = stats_load(z, zw, iters, valid[j] ? k : n - 1);
            }
#pragma unroll
            for (uint32_t j = 0; j < kStatsPerLane; j++) {
                bool todo = valid[j] && stats_class(px[j], stable_limit, iterations) == 2u;
                const uint32_t bin = todo ? (px[j].it - min_it) >> shift : 0u; /* < FR_STATS_BINS by the choice of shift */
                /* peel by bin: the lanes that agree with the first active lane leave as one add of their number */
#pragma unroll
                for (int round = 0; round < 2; round++) {
                    if (todo) {
                        const uint32_t b0 = __builtin_amdgcn_readfirstlane(bin);
                        const unsigned long long same = __ballot(bin == b0);
                        if (bin == b0) {
                            if (lane == (uint32_t)__ffsll(same) - 1u) atomicAdd(&s_hist[b0], (uint32_t)__popcll(same));
                            todo = false;
                        }
                    }
                }
                if (todo) atomicAdd(&s_hist[bin], 1u);
            }
        }
    }
    __syncthreads();
    {
        const uint32_t c = s_hist[threadIdx.x];
        if (c) atomicAdd(reinterpret_cast<unsigned long long *>(&stats->hist[threadIdx.x]), (unsigned long long)c);
    }
    /* The last workgroup finishes the record.  No fence is needed: it reads nothing another workgroup wrote in this launch,
     * and the write-after-read on min_iters is ordered as the comment at the top of the kernel says.  (A __threadfence()
     * here is an L2 write-back and invalidate per wave: DESIGN.md §3.19.) */
    __syncthreads();
    if (threadIdx.x != 0u) return;
    if (atomicAdd(&stats->reserved, 1u) != gridDim.x - 1u) return;
    stats->shift = shift;
    stats->min_iters = any ? min_it : 0u;
    stats->reserved = 0u;
}

} /* namespace */

hipError_t fr_launch_view_stats(const double *z, uint32_t z_width, const uint32_t *iters, size_t n, double stable_limit,
                                uint32_t iterations, void *stats, hipStream_t stream) {
    if (!stats || (z_width != 2 && z_width != 4) || n > kStatsMaxN || (n && (!z || !iters))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(stats, 0, sizeof(struct fr_view_stats), stream);
    if (e != hipSuccess || n == 0) return e;
    size_t groups = (n + kStatsTile - 1) / kStatsTile;
    if (groups > kStatsMaxGroups) groups = kStatsMaxGroups; /* the kernels stride on */
    if (groups < (n >> 31)) groups = n >> 31;               /* at most 2^31 (+ a tile) pixels per workgroup: see the head of the file */
    struct fr_view_stats *s = static_cast<struct fr_view_stats *>(stats);
    hipLaunchKernelGGL(view_stats_range_kernel, dim3((uint32_t)groups), dim3(kStatsThreads), 0, stream, z, z_width, iters, n, stable_limit,
                       iterations, s);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(view_stats_hist_kernel, dim3((uint32_t)groups), dim3(kStatsThreads), 0, stream, z, z_width, iters, n, stable_limit,
                       iterations, s);
    return hipGetLastError();
}

using namespace fr;

/* the domain of fr_view_stats(_device) short of the record's own pointer */
static int view_stats_check(const fr_config *cfg, const void *z, int z_width, const void *iters, size_t n) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (z_width != 2 && z_width != 4) return fail(FR_ERR_INVALID_ARGUMENT, "z_width must be 2 (re, im) or 4 (re.hi, re.lo, im.hi, im.lo)");
    if (n > kStatsMaxN) return fail(FR_ERR_INVALID_ARGUMENT, "n > 2^40: one call covers one array of at most 2^40 pixels");
    if (std::isnan(cfg->stable_limit)) return fail(FR_ERR_INVALID_ARGUMENT, "stable_limit is NaN: the classes are not defined");
    if (n == 0) return FR_OK;
    if (!z || !iters) return fail(FR_ERR_INVALID_ARGUMENT, "NULL array: the statistics need both z and iters");
    if ((reinterpret_cast<uintptr_t>(z) & 7u) || (reinterpret_cast<uintptr_t>(iters) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "z must be 8-byte aligned and iters 4-byte aligned");
    return FR_OK;
}

extern "C" {

int fr_view_stats_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, size_t n, void *d_stats,
                         void *hip_stream) {
    const int rc = view_stats_check(cfg, d_z, z_width, d_iters, n);
    if (rc != FR_OK) return rc;
    if (!d_stats) return fail(FR_ERR_INVALID_ARGUMENT, "d_stats is NULL");
    if (reinterpret_cast<uintptr_t>(d_stats) & 7u) return fail(FR_ERR_INVALID_ARGUMENT, "d_stats must be 8-byte aligned");
    HIP_TRY(fr_launch_view_stats(static_cast<const double *>(d_z), (uint32_t)z_width, static_cast<const uint32_t *>(d_iters), n,
                                 cfg->stable_limit, cfg->iterations, d_stats, static_cast<hipStream_t>(hip_stream)));
    return FR_OK;
}

int fr_view_stats(const fr_config *cfg, const double *z, int z_width, const uint32_t *iters, size_t n, struct fr_view_stats *out) {
    int rc = view_stats_check(cfg, z, z_width, iters, n);
    if (rc != FR_OK) return rc;
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    if (n == 0) {
        std::memset(out, 0, sizeof *out);
        return FR_OK;
    }
    const size_t zb = n * (size_t)z_width * sizeof(double), ib = n * sizeof(uint32_t);
    LifeShared ls;
    Ctx *ctx;
    rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rc = ctx->reserve(ctx->z, zb);
    if (rc == FR_OK) rc = ctx->reserve(ctx->iters, ib);
    if (rc == FR_OK) rc = ctx->reserve(ctx->misc, sizeof(struct fr_view_stats));
    if (rc != FR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->z.ptr, z, zb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->iters.ptr, iters, ib, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(fr_launch_view_stats(static_cast<const double *>(ctx->z.ptr), (uint32_t)z_width, static_cast<const uint32_t *>(ctx->iters.ptr), n,
                                 cfg->stable_limit, cfg->iterations, ctx->misc.ptr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, ctx->misc.ptr, sizeof(struct fr_view_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

/* a record no call of this library writes is refused, not read as if it were one */
static int stats_record_check(const struct fr_view_stats *s, double p) {
    if (!s) return fail(FR_ERR_INVALID_ARGUMENT, "the statistics record is NULL");
    if (!(p >= 0.0 && p <= 1.0)) return fail(FR_ERR_INVALID_ARGUMENT, "p must be finite and within [0, 1]");
    if (s->shift >= 32u) return fail(FR_ERR_INVALID_ARGUMENT, "inconsistent statistics record: shift >= 32");
    if (s->min_iters > s->max_iters) return fail(FR_ERR_INVALID_ARGUMENT, "inconsistent statistics record: min_iters > max_iters");
    return FR_OK;
}

int fr_stats_percentile(const struct fr_view_stats *s, double p, uint32_t *iters_out) {
    const int rc = stats_record_check(s, p);
    if (rc != FR_OK) return rc;
    if (!iters_out) return fail(FR_ERR_INVALID_ARGUMENT, "iters_out is NULL");
    if (s->escaped == 0) {
        *iters_out = 0;
        return FR_OK;
    }
    const double want = std::ceil(p * (double)s->escaped);
    uint64_t k = want < 1.0 ? 1 : (uint64_t)want;
    if (k > s->escaped) k = s->escaped;
    uint64_t cum = 0;
    for (uint32_t b = 0; b < (uint32_t)FR_STATS_BINS; b++) {
        cum += s->hist[b];
        if (cum >= k) {
            const uint64_t last = (uint64_t)s->min_iters + ((uint64_t)(b + 1) << s->shift) - 1; /* the bin's last index */
            *iters_out = last < s->max_iters ? (uint32_t)last : s->max_iters;
            return FR_OK;
        }
    }
    return fail(FR_ERR_INVALID_ARGUMENT, "inconsistent statistics record: the histogram holds fewer pixels than `escaped`");
}

int fr_auto_exposure(const fr_config *cfg, const struct fr_view_stats *s, double p, double *exposure_out) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    uint32_t q = 0;
    const int rc = fr_stats_percentile(s, p, &q);
    if (rc != FR_OK) return rc;
    if (!exposure_out) return fail(FR_ERR_INVALID_ARGUMENT, "exposure_out is NULL");
    if (s->escaped == 0) {
        *exposure_out = cfg->exposure;
        return FR_OK;
    }
    if (q < 1u) q = 1u;
    *exposure_out = (double)cfg->iterations / (double)q;
    return FR_OK;
}

} /* extern "C" */
