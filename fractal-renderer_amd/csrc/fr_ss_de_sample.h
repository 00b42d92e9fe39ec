/*
 * fr_ss_de_sample.h — internal: one sample of ADAPTIVE SUPERSAMPLED DE (include/fractal_hip.h) from its (z, iters, der) to its
 * packed colour, shared by the DE refine kernels (fr_de.hip: ss_refine_de_f64_kernel, ss_refine_de_pt_kernel; fr_de_bla.hip:
 * ss_refine_de_bla_kernel): colour_de_rows_kernel's pixel (fr_de.hip) operation for operation — the colour map on |z|^2, then
 * every byte times s = D / thickness where s < 1, with truncating casts.  Needs fr_colour.h and fr_de_shade.h before it; included
 * INSIDE the including file's anonymous namespace, like them.
 */
__device__ __forceinline__ uint32_t ss_de_sample_colour(const fr_kparams &p, double zr, double zi, double dr, double di, uint32_t it,
                                                        double pixels, double thickness, const double *s_tab) {
    uint8_t rgb[3] = {0, 0, 0};
    const ColourConsts cc = make_colour_consts(p);
    colour_of(cc, zr * zr + zi * zi, it, s_tab, nullptr, rgb);
    uint32_t r = rgb[0], g = rgb[1], b = rgb[2];
    if (it < p.iterations && thickness > 0.0) {
        const double s = de_distance(zr, zi, dr, di, it, p.iterations, pixels, s_tab) / thickness;
        if (s < 1.0) { /* 0 <= byte * s < 255: the cast truncates, nothing saturates */
            r = (uint32_t)((double)r * s);
            g = (uint32_t)((double)g * s);
            b = (uint32_t)((double)b * s);
        }
    }
    return r | (g << 8) | (b << 16);
}
