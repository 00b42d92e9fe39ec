/*
 * fr_de.h — internal: what the supersampled DE roads (fr_ss_de.hip) take from the DE roads, as fr_bla.h lends BLA-PT's row
 * launch to fr_ss.hip.  Each pair is the domain check the road's own calls run (the file-local de_check / check_bla_de, short of
 * the arrays) and the road's row launch (the file-local de_rows / bla_de_rows), called: rows [y0, y1) of cfg with their
 * derivatives into device arrays on `stream`, between the profiling events.  And what RESUMABLE SCALED DE (fr_de_scaled.hip) takes
 * from RESUMABLE DE (fr_de.hip): the host and device plumbing of a DE state's five arrays, one copy.
 */
#ifndef FR_DE_H
#define FR_DE_H

#include "fr_ctx.h"

namespace fr {

/* the F64 road and PT with a dd or wide centre (fr_de.hip).  wide_call: fr_escape_rows_de_pt_wide's form, centre required. */
int de_domain(const fr_config *cfg, int precision, const Centre &c, bool wide_call, uint32_t y0, uint32_t y1);
int de_render_rows(Ctx &ctx, const fr_config *cfg, int precision, const Centre &c, uint32_t y0, uint32_t y1, double *d_z, uint32_t *d_iters,
                   double *d_der, hipStream_t stream);
/* DE ON BLA-PT (fr_de_bla.hip); bits resolved in place */
int bla_de_domain(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1);
int bla_de_render_rows(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, double *d_z, uint32_t *d_iters,
                       double *d_der, hipStream_t stream);

/* DE ON SCALED PT (fr_de_scaled.hip) for SUPERSAMPLED SCALED DE; bits resolved in place, the centre required */
int scaled_de_domain(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1);
int scaled_de_render_rows(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, uint32_t y0, uint32_t y1, double *d_z,
                          uint32_t *d_iters, double *d_der, hipStream_t stream);

/* The five arrays of a DE state — z, iters, the offset d (PT: dz, SCALED PT: w), m and der — after the road's domain check: the
 * one copy of what fr_escape_rows_de_pt_state / fr_escape_extend_de_pt and their scaled counterparts (fr_de_scaled.hip) do with
 * them (fr_de.hip).  `from` = nullptr: the state render, else the extension from *from.  Both forms check what is left of the
 * calls' domain (the lower cap, NULL and misaligned arrays: texts that name `road` and `d_name`) and return FR_OK without a
 * device where there is nothing to do; the device form then runs `rows` on the caller's stream, the host form keeps z, d and der
 * in the context's z scratch and iters and m in its iters scratch, uploads them first for an extension, and synchronises.  `rows`
 * is a plain function with its arguments behind `self`: nothing is allocated on the call path. */
struct DeStateRows {
    int (*fn)(const void *self, Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_d, uint32_t *d_m, double *d_der, hipStream_t stream);
    const void *self;
};
int de_state_device(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z, void *d_iters, void *d_d, void *d_m,
                    void *d_der, void *hip_stream, const char *road, const char *d_name, const DeStateRows &rows);
int de_state_host(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, double *z, uint32_t *iters, double *d, uint32_t *m,
                  double *der, const char *road, const char *d_name, const DeStateRows &rows);

}  // namespace fr

/* fr_colour_de_rows_device's launch (fr_de.hip: colour_de_rows_kernel) over n stored results; `pixels` and `thickness` as the
 * kernel takes them: (double)height * min(|scale.re|, |scale.im|), and the line's width in those pixels */
hipError_t fr_launch_colour_de_rows(const fr_kparams &p, const double *z, const uint32_t *iters, const double *der, size_t n, double pixels,
                                    double thickness, uint32_t channels, void *out, hipStream_t stream);

/* Colour map + distance shade + box filter over the DE arrays of the s times larger image (fr_ss_de.hip:
 * colour_de_filter_kernel<s>): z, der (2 doubles per sample, 8-byte aligned) and iters hold s * rows rows of s * width samples;
 * dst, bpp as fr_launch_box_filter's; pixels = (double)(s * height) * min|scale| and thickness = T * s, in sample pixels.  The
 * same bytes as fr_launch_colour_de_rows followed by fr_launch_box_filter; s = 1 is the former.  64-bit element offsets. */
hipError_t fr_launch_colour_de_filter(const fr_kparams &p, const double *z, const uint32_t *iters, const double *der, uint32_t width,
                                      uint64_t rows, uint32_t s, double pixels, double thickness, uint32_t bpp, void *dst,
                                      hipStream_t stream, int transfer = 0 /* fr_ss_transfer: LINEAR-LIGHT SUPERSAMPLING */);

#endif
