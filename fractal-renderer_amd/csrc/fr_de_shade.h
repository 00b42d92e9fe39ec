/*
 * fr_de_shade.h — internal: D of "DE" (include/fractal_hip.h), the distance the shading reads, shared by the kernels of
 * fr_de.hip (distance_rows_kernel, colour_de_rows_kernel) and fr_ss_de.hip (colour_de_filter_kernel): one copy of the operation
 * order.  Needs fr_math.h.  Included INSIDE the including file's anonymous namespace, like fr_colour.h.
 */
constexpr double kHalfLn2 = 0x1.62e42fefa39efp-2; /* ln 2 / 2: |z| ln|z| = sqrt(n2) * log2(n2) * (ln 2 / 2) */

/* D of the definition; `pixels` = (double)height * min(|scale.re|, |scale.im|), formed by the host */
__device__ __forceinline__ double de_distance(double zr, double zi, double dr, double di, uint32_t it, uint32_t iterations, double pixels,
                                              const double *lds_tab) {
    if (it == iterations) return 0.0;
    const double n2 = zr * zr + zi * zi, dn2 = dr * dr + di * di;
    const double num = (__builtin_sqrt(n2) * fr_log2_tab(n2, lds_tab)) * kHalfLn2;
    const double D = (num / __builtin_sqrt(dn2)) * pixels;
    return D > 0.0 ? D : 0.0; /* NaN and negatives give 0; +inf stays */
}
