/*
 * fr_ss_adaptive.h — internal: the call skeleton that ADAPTIVE SUPERSAMPLING (fr_ss_adaptive.hip) and ADAPTIVE SUPERSAMPLED DE
 * (fr_ss_adaptive_de.hip) share on the host ("3.32"): the workspace's layout, the device form behind the domain check
 * and the host form with its row pieces.  Each file keeps its own domain check and its own passes (ssa_render, ssad_render) and
 * hands them in as render(ctx, ya, yb, dst, d_work, stream): rows [ya, yb) into dst with the workspace at d_work, the count left
 * in the workspace's first counter.  Host code only.
 */
#ifndef FR_SS_ADAPTIVE_H
#define FR_SS_ADAPTIVE_H

#include <algorithm>
#include <vector>

#include "fr_ss.h"

namespace fr {

/* The workspace of rows [y0, y1) of cfg (not empty).  de: the probe's z, der and iters of rows [ya, yb) in front; then, for both,
 * the probe's colours of those rows, the list and the two counters.  Without the DE arrays the colours lie at 0. */
struct SsAdaptiveLayout {
    uint32_t ya, yb;
    size_t der_off, iters_off, colour_off, list_off, counters_off, total;
};

constexpr uint64_t ceil8(uint64_t v) { return (v + 7u) & ~7ull; }

/* the two row counts apart, so that the host form can bound a piece before it knows where the piece lies */
inline SsAdaptiveLayout ss_adaptive_offsets(uint32_t width, uint64_t probe_rows, uint64_t rows, bool de) {
    SsAdaptiveLayout l{};
    const uint64_t n = (uint64_t)width * probe_rows, arrays = de ? n : 0;
    l.der_off = (size_t)(16u * arrays);
    l.iters_off = l.der_off + (size_t)(16u * arrays);
    l.colour_off = l.iters_off + (size_t)ceil8(4u * arrays);
    l.list_off = l.colour_off + (size_t)ceil8(3u * n);
    l.counters_off = l.list_off + (size_t)ceil8((uint64_t)4u * width * rows);
    l.total = l.counters_off + 2 * sizeof(unsigned long long);
    return l;
}

inline SsAdaptiveLayout ss_adaptive_layout(const fr_config *cfg, uint32_t y0, uint32_t y1, bool de) {
    const uint32_t ya = y0 > 0 ? y0 - 1 : 0, yb = y1 < cfg->height ? y1 + 1 : cfg->height;
    SsAdaptiveLayout l = ss_adaptive_offsets(cfg->width, yb - ya, y1 - y0, de);
    l.ya = ya;
    l.yb = yb;
    return l;
}

/* fr_ss_adaptive_workspace_bytes and fr_ss_adaptive_de_workspace_bytes */
inline int ss_adaptive_workspace_bytes(const fr_config *cfg, uint32_t s, uint32_t y0, uint32_t y1, bool de, size_t *bytes) {
    SsPlan pl;
    const int rc = ss_plan(cfg, s, y0, y1, pl);
    if (rc != FR_OK) return rc;
    if (!bytes) return fail(FR_ERR_INVALID_ARGUMENT, "bytes is NULL");
    *bytes = (size_t)cfg->width * (size_t)(y1 - y0) == 0 ? 0 : ss_adaptive_layout(cfg, y0, y1, de).total;
    return FR_OK;
}

/* The device form behind the domain check: the no-ops, the buffer rules, then the render and the count into d_refined behind it.
 * too_small names the call that sizes the workspace, misaligned what lies in it.  No host synchronisation, no allocation. */
template <class Render>
int ss_adaptive_device(const fr_config *cfg, bool de, const char *too_small, const char *misaligned, uint32_t y0, uint32_t y1, int channels,
                       void *d_out, size_t out_len, void *d_work, size_t work_len, void *d_refined, void *hip_stream, Render &&render) {
    if (y0 == y1) return FR_OK; /* a no-op: no device, no buffer */
    if (reinterpret_cast<uintptr_t>(d_refined) & 7u) return fail(FR_ERR_INVALID_ARGUMENT, "d_refined must be 8-byte aligned (a uint64)");
    if (cfg->width == 0) { /* no pixels: refined = 0 */
        if (!d_refined) return FR_OK;
        return device_form(hip_stream, [&](Ctx &, hipStream_t stream) -> int {
            HIP_TRY(hipMemsetAsync(d_refined, 0, sizeof(uint64_t), stream));
            return FR_OK;
        });
    }
    const SsAdaptiveLayout l = ss_adaptive_layout(cfg, y0, y1, de);
    if (!d_out) return fail(FR_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (out_len < (size_t)channels * cfg->width * (size_t)(y1 - y0)) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < channels*width*(y1-y0)");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output (d_out) must be 4-byte aligned");
    if (work_len < l.total) return fail(FR_ERR_BUFFER_TOO_SMALL, too_small);
    if (!d_work) return fail(FR_ERR_INVALID_ARGUMENT, "d_work is NULL");
    if (reinterpret_cast<uintptr_t>(d_work) & 7u) return fail(FR_ERR_INVALID_ARGUMENT, misaligned);
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) -> int {
        const int rc = render(ctx, y0, y1, d_out, d_work, stream);
        if (rc != FR_OK || !d_refined) return rc;
        HIP_TRY(hipMemcpyAsync(d_refined, static_cast<const char *>(d_work) + l.counters_off, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
        return FR_OK;
    });
}

/* The host form behind the domain check, through the context's scratch: row pieces whose workspace stays under the host roads'
 * cap (one row at the least; the definition makes them exact; a piece of n rows has a neighbour row on either side at the most),
 * one count a piece read behind it, all summed after the call's single synchronisation. */
template <class Render>
int ss_adaptive_host(const fr_config *cfg, bool de, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len, uint64_t *refined,
                     Render &&render) {
    if (refined) *refined = 0;
    if (y0 == y1 || cfg->width == 0) return FR_OK;
    const auto bound = [&](uint32_t n) { return ss_adaptive_offsets(cfg->width, (uint64_t)n + 2, n, de).total; };
    uint32_t piece = y1 - y0;
    while (piece > 1 && bound(piece) > ss_host_work_cap()) piece = (piece + 1) / 2;
    std::vector<uint64_t> counts(((size_t)(y1 - y0) + piece - 1) / piece, 0);
    const int rc = ss_rows_host(cfg, bound(piece), y0, y1, channels, out, out_len,
                                [&](Ctx &ctx, const fr_kout &ko, void *d_work, size_t, hipStream_t stream) {
                                    size_t k = 0;
                                    for (uint32_t ya = y0; ya < y1; ya += piece, k++) {
                                        const uint32_t yb = (uint32_t)std::min<uint64_t>((uint64_t)ya + piece, y1);
                                        const int rc = render(ctx, ya, yb, ko.rgb + (uint64_t)(ya - y0) * cfg->width * (unsigned)channels, d_work, stream);
                                        if (rc != FR_OK) return rc;
                                        const char *count = static_cast<const char *>(d_work) + ss_adaptive_layout(cfg, ya, yb, de).counters_off;
                                        const hipError_t e = hipMemcpyAsync(&counts[k], count, sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
                                        if (e != hipSuccess) return fail_hip(e, "hipMemcpyAsync(refined)");
                                    }
                                    return (int)FR_OK;
                                });
    if (rc != FR_OK) return rc;
    if (refined)
        for (const uint64_t c : counts) *refined += c;
    return FR_OK;
}

}  // namespace fr

#endif
