/*
 * fr_ss.h — internal: the plan of a supersampled render (fr_ss.hip) — cfg_s, the source rows and the band rule of
 * fr_ss_workspace_bytes — which the supersampled DE roads (fr_ss_de.hip) run at 36 bytes per sample in place of 3.
 */
#ifndef FR_SS_H
#define FR_SS_H

#include "fr_ctx.h"

namespace fr {

constexpr size_t kSsBestCap = (size_t)1 << 30;       /* best_bytes of fr_ss_workspace_bytes and fr_ss_de_workspace_bytes */
constexpr size_t kSsHostWorkCap = (size_t)256 << 20; /* the host roads' workspace: the context keeps it */

struct SsPlan {
    fr_config cfg_s;      /* cfg with width * s, height * s */
    uint64_t src_rows;    /* s * (y1 - y0) */
    uint64_t row_bytes;   /* sample_bytes * s * width: one source row */
    size_t min_bytes, best_bytes;
};

/* The part of the domain that needs no precision — cfg, s, the sizes, the rows — and the workspace of rows [y0, y1):
 * min_bytes = one band of 8 * s source rows (or all the rows, if fewer), best_bytes = the whole range, at most 1 GiB.
 * sample_bytes 3: a band is packed r,g,b, and s = 1 renders straight into the output and needs no workspace; 36: a band is
 * the DE arrays (z, der, iters), which s = 1 needs too. */
int ss_plan(const fr_config *cfg, uint32_t s, uint32_t y0, uint32_t y1, SsPlan &pl, uint32_t sample_bytes = 3);

/* LINEAR-LIGHT SUPERSAMPLING: the `transfer` argument of every _tf call, refused before anything else is looked at */
int check_transfer(int transfer);

/* Source rows per band for a workspace of work_len >= min_bytes: the largest multiple of 8 * s that fits (or all the
 * rows), then evened out — nb = ceil(rows / Bmax) bands of ceil(rows / nb) rows rounded up to 8 * s. */
uint64_t ss_band_rows(const SsPlan &pl, uint32_t s, size_t work_len);

}  // namespace fr

#endif
