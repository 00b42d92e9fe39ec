// fractal.hpp — C++ host-side mirror of the reference's public surface for the escape-time path,
// over the C ABI of include/fractal_hip.h (libfractal_hip.so, gfx950 kernels).
//
// The reference is a Rust crate and this image has no Rust toolchain, so the host side above the
// C ABI is written in C++ with the reference's names, argument meaning and error behaviour:
//
//   calc::Algo                     calc/src/lib.rs:150-154   fractal::Algo
//   calc::Imaginary                calc/src/lib.rs:79-117    fractal::Imaginary
//   calc::RGB, RGB::new(r, b, g)   calc/src/lib.rs:121-131   fractal::RGB, RGB::make(r, b, g)
//   calc::Config, Config::new      calc/src/lib.rs:21-69     fractal::Config, Config::make(algo)
//   calc::recursive                calc/src/lib.rs:245-257   fractal::recursive
//   calc::get_recursive_pixel      calc/src/lib.rs:199-235   fractal::get_recursive_pixel
//   get_image                      src/lib.rs:253-270        fractal::get_image (one GPU, or the set chosen with use_devices)
//   get_image, BarnsleyFern arm    src/lib.rs:271-319,417-463  fractal::get_image_fern
//
// The reference's functions are infallible and panic on misuse; here a failing C-ABI call throws
// fractal::Error (there is no CPU fallback to fall back to).
#ifndef FRACTAL_HPP
#define FRACTAL_HPP

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fractal_hip.h"

namespace fractal {

class Error : public std::runtime_error {
  public:
    Error(int code, const char *msg) : std::runtime_error(std::string(msg ? msg : "")), code_(code) {}
    int code() const { return code_; }

  private:
    int code_;
};

inline void check(int rc) {
    if (rc != FR_OK) throw Error(rc, fr_last_error());
}

enum class Algo : uint32_t { Mandelbrot = FR_ALGO_MANDELBROT, BarnsleyFern = FR_ALGO_BARNSLEY_FERN, Julia = FR_ALGO_JULIA };

// calc/src/lib.rs:79-82; layout-compatible with fr_imaginary
struct Imaginary {
    double re = 0.0, im = 0.0;
    static constexpr Imaginary zero() { return Imaginary{0.0, 0.0}; }  // Imaginary::ZERO
    fr_imaginary c() const { return fr_imaginary{re, im}; }
};

// calc/src/lib.rs:121-125; layout-compatible with fr_rgb (the STORED fields)
struct RGB {
    uint8_t r = 0, g = 0, b = 0;
    // RGB::new(r, b, g) — calc/src/lib.rs:129-131: the second parameter is BLUE
    static constexpr RGB make(uint8_t r, uint8_t b, uint8_t g) { return RGB{r, g, b}; }
    bool operator==(const RGB &o) const { return r == o.r && g == o.g && b == o.b; }
};
static_assert(sizeof(RGB) == 3 && sizeof(Imaginary) == 16, "must match the C ABI");

// calc::Config (calc/src/lib.rs:21-37); the C struct IS the representation
struct Config : fr_config {
    // Config::new(algo) — calc/src/lib.rs:39-69
    static Config make(Algo algo = Algo::Mandelbrot) {
        Config c;
        fr_config_new(&c, static_cast<uint32_t>(algo));
        return c;
    }
};

// calc::recursive(iterations, start, c, limit) -> (Imaginary, u32) — calc/src/lib.rs:245-257
inline std::pair<Imaginary, uint32_t> recursive(uint32_t iterations, Imaginary start, Imaginary c, double limit) {
    fr_imaginary pos{};
    uint32_t iters = 0;
    check(fr_recursive(iterations, start.c(), c.c(), limit, &pos, &iters));
    return {Imaginary{pos.re, pos.im}, iters};
}

// calc::get_recursive_pixel(&Config, x, y) -> RGB — calc/src/lib.rs:199-235
inline RGB get_recursive_pixel(const Config &config, uint32_t x, uint32_t y) {
    fr_rgb out{};
    check(fr_pixel(&config, x, y, &out));
    return RGB{out.r, out.g, out.b};
}

// Spread get_image over several GPUs (the reference spreads its rows over every core, src/lib.rs:256-258):
// HIP device indices; an index may repeat.  One device (or never calling this) = the single-GPU path.
inline int &multi_devices() {
    static int n = 0;
    return n;
}
inline void use_devices(const std::vector<int> &devices) {
    check(fr_init_devices(devices.data(), static_cast<int>(devices.size())));
    multi_devices() = static_cast<int>(devices.size());
}

// get_image(&Config) -> Vec<RGB> — src/lib.rs:253-270 (Mandelbrot | Julia arm).
// get_image(config, FR_PRECISION_DD) renders a deep zoom in double-double arithmetic (include/fractal_hip.h,
// fr_precision) on one GPU, whatever use_devices chose; a view centre off the f64 grid needs its low halves:
// fr_render_rows_dd(&config, &pos_lo, 0, config.height, 3, out, out_len).  FR_PRECISION_PT (perturbation: the same deep
// views, far cheaper on long orbits) renders on one GPU the same way; its low halves go through fr_render_rows_pt.
inline std::vector<RGB> get_image(const Config &config, int precision = FR_PRECISION_F64) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    uint8_t *out = reinterpret_cast<uint8_t *>(image.data());
    if (multi_devices() > 1 && precision != FR_PRECISION_DD && precision != FR_PRECISION_PT)
        check(fr_render_rgb8_multi(&config, precision, 0, out, image.size() * sizeof(RGB)));
    else
        check(fr_render_rows_rgb8(&config, precision, 0, config.height, out, image.size() * sizeof(RGB)));
    return image;
}

// In which space the s x s samples of a supersampled form are averaged (include/fractal_hip.h, "LINEAR-LIGHT SUPERSAMPLING"):
// Bytes, the display-encoded values as they are, or Srgb, linear light — decoded, averaged, encoded again, exactly, in integers —
// which keeps the light of a bright thread on a dark ground.  The last, defaulted argument of every supersampled form below.
enum class Transfer : int { Bytes = FR_SS_TRANSFER_BYTES, Srgb = FR_SS_TRANSFER_SRGB };

// get_image anti-aliased: supersample x supersample samples per pixel, box-filtered on the device (include/fractal_hip.h,
// "supersampled rendering"; 1 <= supersample <= FR_SS_MAX).  Only the width x height result crosses PCIe.  One GPU,
// whatever use_devices chose; supersample = 1 is get_image(config, precision) on that GPU, byte for byte.
inline std::vector<RGB> get_image(const Config &config, int precision, uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_tf(&config, precision, nullptr, supersample, static_cast<int>(transfer), 0, config.height, 3,
                               reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB), nullptr));
    return image;
}

// get_image's Algo::BarnsleyFern arm — src/lib.rs:271-319 + fern() :417-463.  threads = what
// rayon::current_num_threads() is on the machine being stood in for (the reference returns ONE thread's image of
// iterations / threads points); seed replaces SmallRng::from_entropy() (src/lib.rs:428).
inline std::vector<RGB> get_image_fern(const Config &config, uint32_t threads, uint64_t seed) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_fern_rgb8(&config, threads, seed, 0, reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB)));
    return image;
}

// ---- a view kept on the device (include/fractal_hip.h, "a view kept on the device"): thin wrappers ----------------
// A GUI keeps (z, iters) of the current view in device memory (20 bytes per pixel, 36 for FR_PRECISION_DD with its low
// parts): escape_rows_device once per view, extend_rows_device on an iterations change, colour_rows_device on every
// control that only feeds the colour map.  Device pointers and a hipStream_t, all asynchronous.
inline void escape_rows_device(const Config &config, void *d_z, void *d_iters, void *hip_stream = nullptr,
                               int precision = FR_PRECISION_F64, const fr_imaginary *pos_lo = nullptr, int z_width = 2) {
    check(fr_escape_rows_device(&config, precision, pos_lo, 0, config.height, z_width, d_z, d_iters, hip_stream, nullptr));
}
// config.iterations is the new cap; the arrays hold the same view at from_iterations (the library cannot check that)
inline void extend_rows_device(const Config &config, uint32_t from_iterations, void *d_z, void *d_iters, void *hip_stream = nullptr,
                               int precision = FR_PRECISION_F64, const fr_imaginary *pos_lo = nullptr, int z_width = 2) {
    check(fr_escape_extend_device(&config, precision, pos_lo, 0, config.height, from_iterations, z_width, d_z, d_iters, hip_stream,
                                  nullptr));
}
// the same over host vectors as fr_escape_rows filled them (z: 2 doubles per pixel), in the f64 arithmetic fr_escape_rows
// used; FR_PRECISION_DD state is four doubles per pixel and goes through fr_escape_extend itself
inline void extend_rows(const Config &config, uint32_t from_iterations, std::vector<double> &z, std::vector<uint32_t> &iters) {
    const size_t n = static_cast<size_t>(config.width) * config.height;
    if (z.size() != 2 * n || iters.size() != n) throw Error(FR_ERR_INVALID_ARGUMENT, "extend_rows: z needs 2 * width * height doubles, iters width * height");
    check(fr_escape_extend(&config, FR_PRECISION_F64, nullptr, 0, config.height, from_iterations, 2, z.data(), iters.data()));
}
// channels 3 (r,g,b) or 4 (r,g,b,255; d_out 4-byte aligned) over the whole stored view
inline void colour_rows_device(const Config &config, const void *d_z, const void *d_iters, void *d_out, int channels = 4,
                               void *hip_stream = nullptr, int z_width = 2) {
    const size_t n = static_cast<size_t>(config.width) * config.height;
    check(fr_colour_rows_device(&config, d_z, z_width, d_iters, n, channels, d_out, static_cast<size_t>(channels) * n, hip_stream));
}


// ---- resumable perturbation (include/fractal_hip.h, "resumable perturbation"): thin wrappers ----------------------
// A deep view kept on the device in FR_PRECISION_PT is (z, iters, dz, m), 40 bytes per pixel: pt_state_rows_device once per
// view, extend_pt_rows_device on an iterations change (config.iterations is the new cap; the arrays hold the same view at
// from_iterations, which the library cannot check), colour_rows_device over (d_z, d_iters) with z_width 2.
inline void pt_state_rows_device(const Config &config, void *d_z, void *d_iters, void *d_dz, void *d_m, void *hip_stream = nullptr,
                                 const fr_imaginary *pos_lo = nullptr) {
    check(fr_escape_rows_pt_state_device(&config, pos_lo, 0, config.height, d_z, d_iters, d_dz, d_m, hip_stream));
}
inline void extend_pt_rows_device(const Config &config, uint32_t from_iterations, void *d_z, void *d_iters, void *d_dz, void *d_m,
                                  void *hip_stream = nullptr, const fr_imaginary *pos_lo = nullptr) {
    check(fr_escape_extend_pt_device(&config, pos_lo, 0, config.height, from_iterations, d_z, d_iters, d_dz, d_m, hip_stream));
}
// ---- WIDE PT (include/fractal_hip.h, "WIDE PT"): a fixed-point view centre of up to 1016 bits ------------------------
// FR_PRECISION_PT past a scale of 10^30: the centre is words x 64 bits per axis instead of (pos, pos_lo); config.pos is not
// read.  A GUI pans with add() and hands the view back to (pos, pos_lo) at shallow scales with to_double().
struct WideCentre {
    std::vector<uint64_t> re, im;  // little-endian words, two's complement, value I / 2^(64 words - 8)
    explicit WideCentre(uint32_t words = 2) : re(words, 0), im(words, 0) {}
    // the smallest word count of the domain rule F >= e + 64, where max |scale| = f 2^e with 0.5 <= f < 1
    static uint32_t words_for_scale(double scale_re, double scale_im) {
        int e = 0;
        (void)std::frexp(std::fmax(std::fabs(scale_re), std::fabs(scale_im)), &e);
        const int n = (e + 72 + 63) / 64;
        return static_cast<uint32_t>(n < 2 ? 2 : n);
    }
    // decimal strings of any length, each component the floor of the string's exact value (fr_wide_from_decimal)
    static WideCentre from_decimal(const std::string &re_text, const std::string &im_text, uint32_t words) {
        WideCentre c(words);
        check(fr_wide_from_decimal(re_text.c_str(), c.re.data(), words));
        check(fr_wide_from_decimal(im_text.c_str(), c.im.data(), words));
        return c;
    }
    uint32_t words() const { return static_cast<uint32_t>(re.size()); }
    void add(double dre, double dim) {
        check(fr_wide_add_double(re.data(), words(), dre));
        check(fr_wide_add_double(im.data(), words(), dim));
    }
    // (pos, pos_lo): the nearest f64 per axis and the nearest f64 to the rest
    std::pair<Imaginary, Imaginary> to_double() const {
        Imaginary hi, lo;
        check(fr_wide_to_double(re.data(), words(), &hi.re, &lo.re));
        check(fr_wide_to_double(im.data(), words(), &hi.im, &lo.im));
        return {hi, lo};
    }
    fr_wide_centre c() const { return fr_wide_centre{words(), re.data(), im.data()}; }  // points into this object
};

// get_image in FR_PRECISION_PT centred on a wide centre (one GPU, whatever use_devices chose)
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_pt_wide(&config, &centre, 0, config.height, 3, reinterpret_cast<uint8_t *>(image.data()),
                                 image.size() * sizeof(RGB)));
    return image;
}
// the resumable state of such a view and its cap raised in place: pt_state_rows_device / extend_pt_rows_device above
inline void pt_state_rows_device(const Config &config, const fr_wide_centre &centre, void *d_z, void *d_iters, void *d_dz, void *d_m,
                                 void *hip_stream = nullptr) {
    check(fr_escape_rows_pt_wide_state_device(&config, &centre, 0, config.height, d_z, d_iters, d_dz, d_m, hip_stream));
}
inline void extend_pt_rows_device(const Config &config, const fr_wide_centre &centre, uint32_t from_iterations, void *d_z,
                                  void *d_iters, void *d_dz, void *d_m, void *hip_stream = nullptr) {
    check(fr_escape_extend_pt_wide_device(&config, &centre, 0, config.height, from_iterations, d_z, d_iters, d_dz, d_m, hip_stream));
}

// ---- BLA-PT (include/fractal_hip.h, "BLA-PT"): FR_PRECISION_PT that skips iterations in bulk ------------------------------
// An approximation of PT, defined exactly; bits = 0 takes FR_BLA_DEFAULT_BITS, else 24 .. 53.  One GPU.
struct Bla {
    int bits = 0;
};
// get_image in BLA-PT centred on (config.pos, pos_lo)
inline std::vector<RGB> get_image(const Config &config, Bla bla, const fr_imaginary *pos_lo = nullptr) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_pt_bla(&config, pos_lo, nullptr, bla.bits, 0, config.height, 3, reinterpret_cast<uint8_t *>(image.data()),
                                image.size() * sizeof(RGB)));
    return image;
}
// ... and centred on a wide centre
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, Bla bla) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_pt_bla(&config, nullptr, &centre, bla.bits, 0, config.height, 3, reinterpret_cast<uint8_t *>(image.data()),
                                image.size() * sizeof(RGB)));
    return image;
}
// (z, iters) of the whole view into device arrays, for colour_rows_device; centre may be null
inline void escape_rows_device(const Config &config, Bla bla, void *d_z, void *d_iters, void *hip_stream = nullptr,
                               const fr_imaginary *pos_lo = nullptr, const fr_wide_centre *centre = nullptr) {
    check(fr_escape_rows_pt_bla_device(&config, pos_lo, centre, bla.bits, 0, config.height, d_z, d_iters, hip_stream));
}

// ---- SCALED PT (include/fractal_hip.h, "SCALED PT"): the wide-centre roads past a scale of 2^440, up to just under 2^952 ------
// bits = -1: the plain scaled loop (WIDE PT's results wherever WIDE PT renders); 0 or 24 .. 53: with BLA-PT's skips.  One GPU.
struct Scaled {
    int bits = -1;
};
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, Scaled scaled) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_pt_scaled(&config, &centre, scaled.bits, 0, config.height, 3, reinterpret_cast<uint8_t *>(image.data()),
                                   image.size() * sizeof(RGB)));
    return image;
}
// (z, iters) of the whole view into device arrays, for colour_rows_device
inline void escape_rows_device(const Config &config, const fr_wide_centre &centre, Scaled scaled, void *d_z, void *d_iters,
                               void *hip_stream = nullptr) {
    check(fr_escape_rows_pt_scaled_device(&config, &centre, scaled.bits, 0, config.height, d_z, d_iters, hip_stream));
}
// A view past 2^440 kept on the device is (z, iters, w, m), 40 bytes per pixel ("RESUMABLE SCALED PT"): the scaled counterparts
// of pt_state_rows_device / extend_pt_rows_device above.  The plain loop's (scaled.bits must be -1: the table form has no state);
// d_w holds the scaled offset w, so only the scaled extension continues what the scaled state render wrote.
inline void pt_state_rows_device(const Config &config, const fr_wide_centre &centre, Scaled scaled, void *d_z, void *d_iters, void *d_w,
                                 void *d_m, void *hip_stream = nullptr) {
    if (scaled.bits != -1) throw std::invalid_argument("SCALED PT: only the plain loop (bits = -1) has a resumable state");
    check(fr_escape_rows_pt_scaled_state_device(&config, &centre, 0, config.height, d_z, d_iters, d_w, d_m, hip_stream));
}
inline void extend_pt_rows_device(const Config &config, const fr_wide_centre &centre, Scaled scaled, uint32_t from_iterations, void *d_z,
                                  void *d_iters, void *d_w, void *d_m, void *hip_stream = nullptr) {
    if (scaled.bits != -1) throw std::invalid_argument("SCALED PT: only the plain loop (bits = -1) has a resumable state");
    check(fr_escape_extend_pt_scaled_device(&config, &centre, 0, config.height, from_iterations, d_z, d_iters, d_w, d_m, hip_stream));
}


// ---- anti-aliased deep views (include/fractal_hip.h, "supersampled rendering on the deep roads") ------------------------------
// get_image on a deep road with supersample x supersample samples per pixel, box-filtered on the device: the forms above with a
// supersample factor behind them (1 .. FR_SS_MAX; 1 is the form without it, byte for byte).  One GPU.
inline std::vector<RGB> get_image_ss_pt(const Config &config, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                                        uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_pt_tf(&config, pos_lo, centre, road, bits, supersample, static_cast<int>(transfer), 0, config.height, 3,
                                  reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB)));
    return image;
}
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_pt(config, nullptr, &centre, FR_PT_ROAD_PLAIN, 0, supersample, transfer);
}
inline std::vector<RGB> get_image(const Config &config, Bla bla, const fr_imaginary *pos_lo, uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_pt(config, pos_lo, nullptr, FR_PT_ROAD_BLA, bla.bits, supersample, transfer);
}
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, Bla bla, uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_pt(config, nullptr, &centre, FR_PT_ROAD_BLA, bla.bits, supersample, transfer);
}
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, Scaled scaled, uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_pt(config, nullptr, &centre, FR_PT_ROAD_SCALED, scaled.bits, supersample, transfer);
}
// ---- adaptive supersampling (include/fractal_hip.h, "ADAPTIVE SUPERSAMPLING") --------------------------------------------------
// The supersampled forms above with an Adaptive behind them: all supersample x supersample samples only at EDGE pixels — those
// whose probe sample differs from a neighbour's by more than `threshold` (0 .. 255; -1: every pixel, the supersampled render's
// bytes; 255: none) in some channel — and the probe sample everywhere else.  *refined (may be null) receives the number of edge
// pixels.  The F64 road and every FR_PRECISION_PT road; one GPU.
struct Adaptive {
    int threshold = 8;
    uint64_t *refined = nullptr;
};
inline std::vector<RGB> get_image_ss_adaptive(const Config &config, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                              int road, int bits, uint32_t supersample, Adaptive adaptive, Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_adaptive_tf(&config, precision, pos_lo, centre, road, bits, supersample, static_cast<int>(transfer), adaptive.threshold, 0,
                                        config.height, 3, reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB),
                                        adaptive.refined));
    return image;
}
inline std::vector<RGB> get_image(const Config &config, int precision, uint32_t supersample, Adaptive adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive(config, precision, nullptr, nullptr, FR_PT_ROAD_PLAIN, 0, supersample, adaptive, transfer);
}
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, uint32_t supersample, Adaptive adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive(config, FR_PRECISION_PT, nullptr, &centre, FR_PT_ROAD_PLAIN, 0, supersample, adaptive, transfer);
}
inline std::vector<RGB> get_image(const Config &config, Bla bla, const fr_imaginary *pos_lo, uint32_t supersample, Adaptive adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive(config, FR_PRECISION_PT, pos_lo, nullptr, FR_PT_ROAD_BLA, bla.bits, supersample, adaptive, transfer);
}
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, Bla bla, uint32_t supersample, Adaptive adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive(config, FR_PRECISION_PT, nullptr, &centre, FR_PT_ROAD_BLA, bla.bits, supersample, adaptive, transfer);
}
inline std::vector<RGB> get_image(const Config &config, const fr_wide_centre &centre, Scaled scaled, uint32_t supersample, Adaptive adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive(config, FR_PRECISION_PT, nullptr, &centre, FR_PT_ROAD_SCALED, scaled.bits, supersample, adaptive, transfer);
}
// A kept anti-aliased view is a kept view of the config with width and height times supersample: the escape / state / extend
// wrappers above on that config, and this to colour it — colour map and box filter in one kernel, no RGB workspace.
// channels 3 (r,g,b) or 4 (r,g,b,255; d_out 4-byte aligned); config is the OUTPUT's (width x height).
inline void colour_rows_ss_device(const Config &config, const void *d_z, const void *d_iters, uint32_t supersample, void *d_out,
                                  int channels = 4, void *hip_stream = nullptr, int z_width = 2, Transfer transfer = Transfer::Bytes) {
    check(fr_colour_rows_ss_tf_device(&config, d_z, z_width, d_iters, config.width, config.height, supersample, static_cast<int>(transfer), channels,
                                      d_out, static_cast<size_t>(channels) * config.width * config.height, hip_stream));
}

// ---- auto-exposure (include/fractal_hip.h, "statistics of a kept view") ------------------------------------------------------
// The exposure a view's own escape indices call for: its (z, iters) reduced on the device to the 8 KB fr_view_stats record,
// a percentile of the escaped pixels' indices taken from it on the host, and the exposure that gives a pixel there the full
// primary colour.  The image stays the reference's colour map at that exposure.  (The record is `struct fr_view_stats`: the
// C call that fills it bears the same name.)
using ViewStats = struct fr_view_stats;
// over host vectors as fr_escape_rows & co fill them: z_width doubles per pixel (4: DD with its low parts, read on the hi parts)
inline ViewStats view_stats(const Config &config, const std::vector<double> &z, const std::vector<uint32_t> &iters, int z_width = 2) {
    if (z_width < 1 || z.size() != static_cast<size_t>(z_width) * iters.size())
        throw Error(FR_ERR_INVALID_ARGUMENT, "view_stats: z needs z_width doubles per entry of iters");
    ViewStats out;
    check(fr_view_stats(&config, z.data(), z_width, iters.data(), iters.size(), &out));
    return out;
}
// device arrays into a device record (sizeof(ViewStats) bytes, 8-byte aligned), asynchronous on hip_stream: once per new view
// or cap of a kept view; the GUI then copies the record back and recolours with auto_exposure's answer
inline void view_stats_device(const Config &config, const void *d_z, const void *d_iters, size_t n, void *d_stats,
                              void *hip_stream = nullptr, int z_width = 2) {
    check(fr_view_stats_device(&config, d_z, z_width, d_iters, n, d_stats, hip_stream));
}
inline uint32_t stats_percentile(const ViewStats &stats, double p) {
    uint32_t out = 0;
    check(fr_stats_percentile(&stats, p, &out));
    return out;
}
// 0.99 is a presentation default: a lone pixel beside a minibrot should not darken the frame; 1.0 takes the maximum
inline double auto_exposure(const Config &config, const ViewStats &stats, double percentile = 0.99) {
    double out = 0.0;
    check(fr_auto_exposure(&config, &stats, percentile, &out));
    return out;
}
// get_image at that exposure, on any single-device road: escape(cfg_s, z, iters) fills 2 doubles and one index per pixel of
// cfg_s = config with width and height times supersample (fr_escape_rows, fr_escape_rows_pt_wide, ...); the result is the
// road's render (supersampled render) of config with `exposure` set to *exposure_out, byte for byte.
template <class Escape>
std::vector<RGB> get_image_auto(const Config &config, uint32_t supersample, double percentile, double *exposure_out, Escape &&escape,
                                Transfer transfer = Transfer::Bytes) {
    if (supersample < 1 || supersample > FR_SS_MAX) throw Error(FR_ERR_INVALID_ARGUMENT, "get_image_auto: supersample is 1 .. FR_SS_MAX");
    Config big = config;
    big.width *= supersample;
    big.height *= supersample;
    const size_t n = static_cast<size_t>(big.width) * big.height;
    std::vector<double> z(2 * n);
    std::vector<uint32_t> iters(n);
    escape(big, z.data(), iters.data());
    Config shown = config;
    shown.exposure = auto_exposure(config, view_stats(big, z, iters), percentile);
    if (exposure_out) *exposure_out = shown.exposure;
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_colour_ss_rgb8_tf(&shown, z.data(), 2, iters.data(), config.width, config.height, supersample, static_cast<int>(transfer), 3,
                               reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB)));
    return image;
}
// ... in the arithmetic of `precision` (FR_PRECISION_F64, FR_PRECISION_F32; the deep precisions with pos_lo = 0)
inline std::vector<RGB> get_image_auto(const Config &config, int precision = FR_PRECISION_F64, double percentile = 0.99,
                                       uint32_t supersample = 1, double *exposure_out = nullptr, Transfer transfer = Transfer::Bytes) {
    return get_image_auto(config, supersample, percentile, exposure_out, [&](const Config &big, double *z, uint32_t *iters) {
        check(fr_escape_rows(&big, precision, 0, big.height, z, iters));
    }, transfer);
}

// ---- distance estimation (include/fractal_hip.h, "DE") ------------------------------------------------------------------------
// get_image with distance shading: the road's escape results WITH the orbit's derivative, then the colour map with every byte
// of an escaped pixel closer than `thickness` pixels to the set scaled by distance / thickness — filaments thinner than a
// pixel stay visible.  escape(config, z, iters, der) fills 2 + 2 doubles and one index per pixel (fr_escape_rows_de,
// fr_escape_rows_de_pt_wide).  thickness 0 is get_image's bytes.
template <class Escape>
std::vector<RGB> get_image_de(const Config &config, double thickness, Escape &&escape) {
    const size_t n = static_cast<size_t>(config.width) * config.height;
    std::vector<double> z(2 * n), der(2 * n);
    std::vector<uint32_t> iters(n);
    escape(config, z.data(), iters.data(), der.data());
    std::vector<RGB> image(n);
    check(fr_colour_de_rgb8(&config, z.data(), iters.data(), der.data(), n, thickness, reinterpret_cast<uint8_t *>(image.data()),
                            image.size() * sizeof(RGB)));
    return image;
}
// Anti-aliased (include/fractal_hip.h, "SUPERSAMPLED DE"): supersample x supersample samples per pixel, each shaded with the
// thickness thickness * supersample in sample pixels — the line stays `thickness` output pixels wide — and box-filtered on the
// device; the larger DE arrays exist only a band at a time.  road FR_PT_ROAD_PLAIN or FR_PT_ROAD_BLA.  The overloads below take
// it as their last argument; 1 is the form without it, byte for byte.
inline std::vector<RGB> get_image_ss_de(const Config &config, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                        int road, int bits, double thickness, uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_de_tf(&config, precision, pos_lo, centre, road, bits, thickness, supersample, static_cast<int>(transfer), 0, config.height, 3,
                                  reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB)));
    return image;
}
// ... on the F64 road, or on PT with a dd centre (precision FR_PRECISION_PT; pos_lo may be null)
inline std::vector<RGB> get_image_de(const Config &config, double thickness = 1.0, int precision = FR_PRECISION_F64,
                                     const fr_imaginary *pos_lo = nullptr, uint32_t supersample = 1, Transfer transfer = Transfer::Bytes) {
    if (supersample != 1) return get_image_ss_de(config, precision, pos_lo, nullptr, FR_PT_ROAD_PLAIN, 0, thickness, supersample, transfer);
    return get_image_de(config, thickness, [&](const Config &c, double *z, uint32_t *iters, double *der) {
        check(fr_escape_rows_de(&c, precision, pos_lo, 0, c.height, z, iters, der));
    });
}
// ... on PT with a wide centre
inline std::vector<RGB> get_image_de(const Config &config, const fr_wide_centre &centre, double thickness = 1.0, uint32_t supersample = 1,
                                     Transfer transfer = Transfer::Bytes) {
    if (supersample != 1) return get_image_ss_de(config, FR_PRECISION_PT, nullptr, &centre, FR_PT_ROAD_PLAIN, 0, thickness, supersample, transfer);
    return get_image_de(config, thickness, [&](const Config &c, double *z, uint32_t *iters, double *der) {
        check(fr_escape_rows_de_pt_wide(&c, &centre, 0, c.height, z, iters, der));
    });
}
// ... on BLA-PT (include/fractal_hip.h, "DE ON BLA-PT"): the derivative goes through the table's skips; a dd centre
// (config.pos, pos_lo; pos_lo may be null) or a wide centre, never both
inline std::vector<RGB> get_image_de(const Config &config, Bla bla, double thickness = 1.0, const fr_imaginary *pos_lo = nullptr,
                                     const fr_wide_centre *centre = nullptr, uint32_t supersample = 1, Transfer transfer = Transfer::Bytes) {
    if (supersample != 1)
        return get_image_ss_de(config, FR_PRECISION_PT, pos_lo, centre, FR_PT_ROAD_BLA, bla.bits, thickness, supersample, transfer);
    return get_image_de(config, thickness, [&](const Config &c, double *z, uint32_t *iters, double *der) {
        check(fr_escape_rows_de_pt_bla(&c, pos_lo, centre, bla.bits, 0, c.height, z, iters, der));
    });
}
// ... past a scale of 2^440, on SCALED PT (include/fractal_hip.h, "DE ON SCALED PT"): der holds the scaled derivative u = d 2^-e,
// and the shading is DE's own on the scaled view that fr_de_scaled_view writes.  One sample per pixel.
inline std::vector<RGB> get_image_de(const Config &config, Scaled scaled, const fr_wide_centre &centre, double thickness = 1.0) {
    const size_t n = static_cast<size_t>(config.width) * config.height;
    std::vector<double> z(2 * n), der(2 * n);
    std::vector<uint32_t> iters(n);
    check(fr_escape_rows_de_pt_scaled(&config, &centre, scaled.bits, 0, config.height, z.data(), iters.data(), der.data()));
    Config view = config;
    check(fr_de_scaled_view(&config, &view));
    std::vector<RGB> image(n);
    check(fr_colour_de_rgb8(&view, z.data(), iters.data(), der.data(), n, thickness, reinterpret_cast<uint8_t *>(image.data()),
                            image.size() * sizeof(RGB)));
    return image;
}
// ... anti-aliased (include/fractal_hip.h, "SUPERSAMPLED SCALED DE"): supersample x supersample samples per pixel, each shaded on
// the scaled view with thickness * supersample in sample pixels, box-filtered on the device; supersample = 1 is the call above.
inline std::vector<RGB> get_image_de(const Config &config, Scaled scaled, const fr_wide_centre &centre, double thickness,
                                     uint32_t supersample, Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_de_pt_scaled_tf(&config, &centre, scaled.bits, thickness, supersample, static_cast<int>(transfer), 0, config.height, 3,
                                            reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB)));
    return image;
}
// the same into device memory through a workspace the caller lends (fr_ss_de_workspace_bytes), asynchronous on hip_stream
inline void get_image_de_device(const Config &config, Scaled scaled, const fr_wide_centre &centre, double thickness, uint32_t supersample,
                                void *d_out, void *d_work, size_t work_len, int channels = 4, void *hip_stream = nullptr, Transfer transfer = Transfer::Bytes) {
    check(fr_render_rows_ss_de_pt_scaled_tf_device(&config, &centre, scaled.bits, thickness, supersample, static_cast<int>(transfer), 0, config.height,
                                                   channels, d_out, static_cast<size_t>(channels) * config.width * config.height, d_work,
                                                   work_len, hip_stream));
}
// ---- adaptive anti-aliased distance estimation (include/fractal_hip.h, "ADAPTIVE SUPERSAMPLED DE") -----------------------------
// get_image_de's supersampled forms with an AdaptiveDe behind them: the distance-shaded supersample x supersample samples only at
// EDGE pixels — those whose shaded probe differs from a neighbour's by more than `threshold` in some channel (-1: every pixel, the
// supersampled DE render's bytes, for which that form is faster) and those whose probe lies closer to the set than `reach` output
// pixels by its own distance estimate (0: the colour rule alone) — and the probe sample everywhere else.  *refined (may be null)
// receives the number of edge pixels.  The F64 road, PT with a dd or a wide centre, and BLA-PT; one GPU.
struct AdaptiveDe {
    int threshold = 8;
    double reach = 2.0;
    uint64_t *refined = nullptr;
};
inline std::vector<RGB> get_image_ss_adaptive_de(const Config &config, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                                 int road, int bits, double thickness, uint32_t supersample, AdaptiveDe adaptive,
                                                 Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_adaptive_de_tf(&config, precision, pos_lo, centre, road, bits, thickness, supersample, static_cast<int>(transfer),
                                           adaptive.threshold, adaptive.reach, 0, config.height, 3,
                                           reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB), adaptive.refined));
    return image;
}
// ... on the F64 road, or on PT with a dd centre (precision FR_PRECISION_PT; pos_lo may be null)
inline std::vector<RGB> get_image_de(const Config &config, double thickness, int precision, const fr_imaginary *pos_lo, uint32_t supersample,
                                     AdaptiveDe adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive_de(config, precision, pos_lo, nullptr, FR_PT_ROAD_PLAIN, 0, thickness, supersample, adaptive, transfer);
}
// ... on PT with a wide centre
inline std::vector<RGB> get_image_de(const Config &config, const fr_wide_centre &centre, double thickness, uint32_t supersample,
                                     AdaptiveDe adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive_de(config, FR_PRECISION_PT, nullptr, &centre, FR_PT_ROAD_PLAIN, 0, thickness, supersample, adaptive, transfer);
}
// ... on BLA-PT: a dd centre (config.pos, pos_lo; pos_lo may be null) or a wide centre, never both
inline std::vector<RGB> get_image_de(const Config &config, Bla bla, double thickness, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                     uint32_t supersample, AdaptiveDe adaptive, Transfer transfer = Transfer::Bytes) {
    return get_image_ss_adaptive_de(config, FR_PRECISION_PT, pos_lo, centre, FR_PT_ROAD_BLA, bla.bits, thickness, supersample, adaptive, transfer);
}
// ... past a scale of 2^440, on SCALED PT (include/fractal_hip.h, "ADAPTIVE SUPERSAMPLED SCALED DE"): the probe and the samples are
// those of the supersampled scaled form above, shaded on the scaled view
inline std::vector<RGB> get_image_de(const Config &config, Scaled scaled, const fr_wide_centre &centre, double thickness, uint32_t supersample,
                                     AdaptiveDe adaptive, Transfer transfer = Transfer::Bytes) {
    std::vector<RGB> image(static_cast<size_t>(config.width) * config.height);
    check(fr_render_rows_ss_adaptive_de_pt_scaled_tf(&config, &centre, scaled.bits, thickness, supersample, static_cast<int>(transfer),
                                                     adaptive.threshold, adaptive.reach, 0, config.height, 3,
                                                     reinterpret_cast<uint8_t *>(image.data()), image.size() * sizeof(RGB), adaptive.refined));
    return image;
}
// A DE view past 2^440 kept on the device is (z, iters, w, m, der), 56 bytes per pixel ("RESUMABLE SCALED DE"): the state render and
// the extension that raises its cap in place, scaled derivative included.  The plain loop's (scaled.bits must be -1: the table
// form has no state).  Recolour with colour_de_rows_device / colour_de_rows_ss_device on the view fr_de_scaled_view writes.
inline void de_state_rows_device(const Config &config, const fr_wide_centre &centre, Scaled scaled, void *d_z, void *d_iters, void *d_w,
                                 void *d_m, void *d_der, void *hip_stream = nullptr) {
    if (scaled.bits != -1) throw std::invalid_argument("SCALED PT: only the plain loop (bits = -1) has a resumable state");
    check(fr_escape_rows_de_pt_scaled_state_device(&config, &centre, 0, config.height, d_z, d_iters, d_w, d_m, d_der, hip_stream));
}
inline void extend_de_rows_device(const Config &config, const fr_wide_centre &centre, Scaled scaled, uint32_t from_iterations, void *d_z,
                                  void *d_iters, void *d_w, void *d_m, void *d_der, void *hip_stream = nullptr) {
    if (scaled.bits != -1) throw std::invalid_argument("SCALED PT: only the plain loop (bits = -1) has a resumable state");
    check(fr_escape_extend_de_pt_scaled_device(&config, &centre, 0, config.height, from_iterations, d_z, d_iters, d_w, d_m, d_der, hip_stream));
}
// a kept view's recolour at another thickness, device arrays, asynchronous on hip_stream: no orbit is run
inline void colour_de_rows_device(const Config &config, const void *d_z, const void *d_iters, const void *d_der, double thickness,
                                  void *d_out, int channels = 4, void *hip_stream = nullptr) {
    const size_t n = static_cast<size_t>(config.width) * config.height;
    check(fr_colour_de_rows_device(&config, d_z, d_iters, d_der, n, thickness, channels, d_out, hip_stream));
}
// A kept anti-aliased DE view is a kept DE view of the config with width and height times supersample (36 * supersample^2 bytes
// per output pixel): this colours, shades and box-filters it in one kernel.  config is the OUTPUT's; thickness in output pixels.
inline void colour_de_rows_ss_device(const Config &config, const void *d_z, const void *d_iters, const void *d_der, uint32_t supersample,
                                     double thickness, void *d_out, int channels = 4, void *hip_stream = nullptr, Transfer transfer = Transfer::Bytes) {
    check(fr_colour_de_rows_ss_tf_device(&config, d_z, d_iters, d_der, config.width, config.height, supersample, static_cast<int>(transfer), thickness,
                                         channels, d_out, static_cast<size_t>(channels) * config.width * config.height, hip_stream));
}

}  // namespace fractal
#endif
