/*
 * fr_de.h — internal: the one copy of the DE calls' host plumbing, on top of fr_ctx.h's row-call helpers.  A DE road (F64 / PT
 * in fr_de.hip, BLA-PT in fr_de_bla.hip, SCALED PT in fr_de_scaled.hip) gives three things: its domain check short of the
 * arrays, its launch on given kernel parameters, and its refine launch (fr_ss_list.h).  Everything between those and an entry
 * point is here: DE's limit and its three arrays, the device and host form of a three-array row call, the rows between the
 * profiling events over a road's launch (the rows of a strided map: fr_ss_list.h), and the device and host form of a DE state's arrays.
 * The supersampled DE calls (fr_ss_de.hip, fr_ss_adaptive_de.hip) are made of the same pieces.  Callables throughout
 * (lambdas: nothing is allocated on a call path); the order of an entry point's checks and their texts are behaviour
 * (tests/golden/de_call_errors.json).
 */
#ifndef FR_DE_H
#define FR_DE_H

#include "fr_ctx.h"

namespace fr {

/* ---- the roads: the domain short of the arrays (rows, road, centre, bits — resolved in place —, limit) and the launch of the
 * local grid in `p` with its derivatives, arguments already checked; `kname` is the kernel's name for fr_last_kernel_name ---- */

/* the F64 road and PT with a dd or wide centre (fr_de.hip).  wide_call: fr_escape_rows_de_pt_wide's form, centre required. */
int de_domain(const fr_config *cfg, int precision, const Centre &c, bool wide_call, uint32_t y0, uint32_t y1);
int de_launch(Ctx &ctx, const fr_config *cfg, int precision, const Centre &c, const fr_kparams &p, double *d_z, uint32_t *d_iters,
              double *d_der, hipStream_t stream, const char *&kname);
/* DE ON BLA-PT (fr_de_bla.hip) */
int bla_de_domain(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1);
int bla_de_launch(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_kparams &p, double *d_z, uint32_t *d_iters,
                  double *d_der, hipStream_t stream, const char *&kname);
/* DE ON SCALED PT (fr_de_scaled.hip): the centre required; bits < 0: the plain scaled loop, no table */
int scaled_de_domain(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1);
int scaled_de_launch(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_kparams &p, double *d_z, uint32_t *d_iters,
                     double *d_der, hipStream_t stream, const char *&kname);

/* A road's launch on its view, launch(ctx, p, d_z, d_iters, d_der, stream, kname), as the wrappers below take it:
 * de_road(de_launch, cfg, precision, c), de_road(bla_de_launch, cfg, c, bits), de_road(scaled_de_launch, cfg, c, bits). */
template <class Fn, class... View>
auto de_road(Fn *launch, const fr_config *cfg, View... view) {
    return [=](Ctx &ctx, const fr_kparams &p, double *d_z, uint32_t *d_iters, double *d_der, hipStream_t stream, const char *&kname) {
        return launch(ctx, cfg, view..., p, d_z, d_iters, d_der, stream, kname);
    };
}

/* rows(ctx, d_z, d_iters, d_der, stream): rows [y0, y1) of cfg with their derivatives into device arrays as one launch of the
 * road on `stream` between the profiling events; de_render_rows: that, called.  (The rows of a strided map: fr_ss_list.h's
 * de_render_map.) */
template <class Road>
auto de_rows(const fr_config *cfg, uint32_t y0, uint32_t y1, Road road) {
    return [=](Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_der, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, 0, stream,
                             [&](fr_kparams &p, const char *&kname) { return road(ctx, p, d_z, d_iters, d_der, stream, kname); });
    };
}

template <class Road>
int de_render_rows(Ctx &ctx, const fr_config *cfg, uint32_t y0, uint32_t y1, double *d_z, uint32_t *d_iters, double *d_der, hipStream_t stream,
                   Road road) {
    return de_rows(cfg, y0, y1, road)(ctx, d_z, d_iters, d_der, stream);
}

/* ---- DE's own rules ------------------------------------------------------------------------------------------------------ */

int check_de_limit(const fr_config *cfg);
/* the three arrays of a DE call: none NULL (`null_text`: the render's, unless the call has a text of its own), z and der 8-byte
 * aligned, iters 4-byte aligned */
int check_de_arrays(const void *z, const void *iters, const void *der, const char *null_text = nullptr);

/* ---- the two forms of a three-array row call, after the road's domain check: no pixels, nothing to do and no device needed;
 * else the arrays' rules, then rows(ctx, d_z, d_iters, d_der, stream) on the caller's stream, or on the context's with z and der
 * in its z scratch (as the PT state's z and dz are), iters in its iters scratch, copied back behind it, one synchronisation ---- */
template <class Rows>
int de_rows_device(const fr_config *cfg, uint32_t y0, uint32_t y1, void *d_z, void *d_iters, void *d_der, void *hip_stream, Rows &&rows) {
    if ((size_t)cfg->width * (size_t)(y1 - y0) == 0) return FR_OK;
    const int rc = check_de_arrays(d_z, d_iters, d_der);
    if (rc != FR_OK) return rc;
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) {
        return rows(ctx, static_cast<double *>(d_z), static_cast<uint32_t *>(d_iters), static_cast<double *>(d_der), stream);
    });
}

template <class Rows>
int de_rows_host(const fr_config *cfg, uint32_t y0, uint32_t y1, double *z, uint32_t *iters, double *der, Rows &&rows) {
    const size_t npx = (size_t)cfg->width * (size_t)(y1 - y0);
    if (npx == 0) return FR_OK;
    const int rc = check_de_arrays(z, iters, der);
    if (rc != FR_OK) return rc;
    return host_raw(z, npx * 2 * sizeof(double), iters, npx * sizeof(uint32_t), nullptr, nullptr, der, false,
                    [&](Ctx &ctx, double *d_z, uint32_t *d_iters, double *, uint32_t *, double *d_der, hipStream_t stream) {
                        return rows(ctx, d_z, d_iters, d_der, stream);
                    });
}

/* ---- RESUMABLE DE: the arrays of a DE state — z, iters, der, and on a perturbation road the offset d (PT: dz, SCALED PT: w) and m
 * between them — after the road's domain check.  `from` = nullptr: the state render, else the extension from *from.  `road` and
 * `d_name` name the perturbation road and its offset in the texts; road = nullptr: the F64 road's three arrays, d and m NULL.
 * de_state_check is what is left of the calls' domain (check_state's order and its M < N text, fr_ctx.h); *work = false: a legal
 * call with nothing to do (no rows; for an extension also M == N or an algorithm without orbits), no device needed.  The device
 * form then runs rows(ctx, d_z, d_iters, d_d, d_m, d_der, stream) on the caller's stream; the host form keeps z, d and der in
 * the context's z scratch and iters and m in its iters scratch, uploads them first for an extension, and synchronises. ---- */
int de_state_check(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, const void *z, const void *iters, const void *d,
                   const void *m, const void *der, const char *road, const char *d_name, bool *work);

template <class Rows>
int de_state_device(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z, void *d_iters, void *d_d, void *d_m,
                    void *d_der, void *hip_stream, const char *road, const char *d_name, Rows &&rows) {
    bool work;
    const int rc = de_state_check(cfg, y0, y1, from, d_z, d_iters, d_d, d_m, d_der, road, d_name, &work);
    if (rc != FR_OK || !work) return rc;
    return device_form(hip_stream, [&](Ctx &ctx, hipStream_t stream) {
        return rows(ctx, static_cast<double *>(d_z), static_cast<uint32_t *>(d_iters), static_cast<double *>(d_d), static_cast<uint32_t *>(d_m),
                    static_cast<double *>(d_der), stream);
    });
}

template <class Rows>
int de_state_host(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, double *z, uint32_t *iters, double *d, uint32_t *m,
                  double *der, const char *road, const char *d_name, Rows &&rows) {
    bool work;
    const int rc = de_state_check(cfg, y0, y1, from, z, iters, d, m, der, road, d_name, &work);
    if (rc != FR_OK || !work) return rc;
    const size_t npx = (size_t)cfg->width * (size_t)(y1 - y0);
    return host_raw(z, npx * 2 * sizeof(double), iters, npx * sizeof(uint32_t), d, m, der, from != nullptr, rows);
}

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
