// fractal_cli — command line over libfractal_hip.so with the reference's flags and defaults
// (clap builder at src/lib.rs:32-164, extraction at :168-226), so a user of the reference binary can
// run the same command lines on an MI355X.  It writes a binary PPM (P6) of the Vec<RGB> bytes: the
// AVIF encoder (src/lib.rs:323-367) is out of scope and stays the reference's.
//
//   g++ -std=c++17 -Iinclude -Ifractal-renderer_amd/host fractal-renderer_amd/cli/fractal_cli.cpp
//       -Lfractal-renderer_amd -lfractal_hip -Wl,-rpath,$PWD/fractal-renderer_amd -o fractal_cli
//   ./fractal_cli 3000 3000 -i 1024 -s 1000000 -x -0.7436447860 -y 0.1318252536 -o zoom
//
// Extensions (no counterpart upstream): --f32; --devices 0,1,... (spread the image over several GPUs);
// --perturbation (deep zooms: FR_PRECISION_PT on a wide centre; -x / -y are then read as decimal strings of any length, at
// the word count the scale asks for, and scales up to 2^440 render — include/fractal_hip.h, "WIDE PT");
// --bla or --bla=BITS beside --perturbation (BLA-PT: the same view with iterations skipped in bulk, an approximation defined
// in include/fractal_hip.h, "BLA-PT"; BITS is 24 .. 53, default 40);
// --scaled beside --perturbation (SCALED PT: the pixel loop that carries its offsets scaled by the view's exponent, so scales
// past 2^440 render, up to just under 2^952; it combines with --bla — include/fractal_hip.h, "SCALED PT");
// --supersample N (N x N samples per pixel, box-filtered on the device; with --perturbation, --bla and --scaled too);
// --adaptive or --adaptive=T beside --supersample (adaptive supersampling: all N x N samples only at edge pixels, those whose
// probe sample differs from a neighbour's by more than T, 0 .. 255, default 8, in some channel; -1 refines every pixel — written
// with '=': a bare number after --adaptive is <width>; include/fractal_hip.h, "ADAPTIVE SUPERSAMPLING"; with --perturbation, --bla
// and --scaled too, not with --distance-shade, --auto-exposure, --f32, --devices or -a fern; the refined share is printed unless
// --quiet);
// --linear-light beside --supersample above 1 (the N x N samples are averaged as linear light — decoded from sRGB, averaged and
// encoded again, exactly — so a thin bright line keeps its light; include/fractal_hip.h, "LINEAR-LIGHT SUPERSAMPLING"; with
// --adaptive, --perturbation, --bla, --scaled and --auto-exposure too);
// --auto-exposure [P] (the exposure is chosen from the view's own escape indices: the one at which an escaped pixel at
// percentile P of them, default 0.99, gets the full primary colour — include/fractal_hip.h, "statistics of a kept view"; a
// following number within [0, 1] written with a '.' or an exponent is P (0.5, 1.0 — a bare 0 or 1 is a <width>), or write
// --auto-exposure=P; every single-device road above, not with -e, more than
// one device or -a fern; the chosen exposure is printed unless --quiet);
// --distance-shade T (distance estimation: an escaped pixel closer than T pixels to the set is darkened by distance / T, so
// filaments thinner than a pixel stay visible — include/fractal_hip.h, "DE"; the F64 road, or --perturbation; not with --bla,
// --scaled, --supersample above 1, --f32, --devices, --auto-exposure or -a fern);
// for -a fern: --threads N (the rayon thread count being stood in for; default: this machine's hardware
// threads, what rayon would use) and --seed N (default: from the OS, as the reference seeds from entropy).
// Not handled here (by design): --gui, --open.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "fractal.hpp"

namespace {

[[noreturn]] void die(const std::string &msg) {
    std::fprintf(stderr, "error: %s\n", msg.c_str());
    std::exit(2);
}

// parse_hex_rgb (src/lib.rs:22-29): "RRGGBB" -> RGB::new(r, g, b); RGB::new's parameters are
// (r, b, g) (calc/src/lib.rs:129-131), so that call stores {r: r, g: b, b: g}.
fractal::RGB parse_hex_rgb(const std::string &s) {
    if (s.size() != 6) die("failed to parse hex color");
    auto byte = [&](int i) {
        char *end = nullptr;
        const std::string part = s.substr(i, 2);
        long v = std::strtol(part.c_str(), &end, 16);
        if (*end != '\0') die("failed to parse hex color");
        return static_cast<uint8_t>(v);
    };
    return fractal::RGB::make(byte(0), byte(2), byte(4));
}

double to_f64(const std::string &s, const char *what) {
    char *end = nullptr;
    double v = std::strtod(s.c_str(), &end);
    if (end == s.c_str() || *end != '\0') die(std::string("invalid value for ") + what + ": " + s);
    return v;
}

uint32_t to_u32(const std::string &s, const char *what) {
    char *end = nullptr;
    unsigned long long v = std::strtoull(s.c_str(), &end, 10);
    if (end == s.c_str() || *end != '\0' || v > 0xFFFFFFFFull) die(std::string("invalid value for ") + what + ": " + s);
    return static_cast<uint32_t>(v);
}

}  // namespace

int main(int argc, char **argv) {
    using namespace fractal;
    // defaults: src/lib.rs:34-164
    std::string width = "750", height = "500", limit = "65536", stable_limit = "2", pos_y = "0", scale = "0.4",
                exposure = "5", filename = "output", algo_s = "mandelbrot", color_weight = "0.01";
    std::optional<std::string> iterations, pos_x, scale_x, scale_y, primary, secondary, julia_re, julia_im, devices, threads_s,
        seed_s, supersample_s;
    bool disable_inside = false, unsmooth = false, f32 = false, quiet = false, perturbation = false, bla = false, scaled = false;
    bool exposure_given = false, auto_exposure_on = false;
    std::optional<std::string> distance_shade;
    bool adaptive = false;
    bool linear_light = false;
    int adaptive_t = 8;
    double auto_p = 0.99;
    int bla_bits = 0;
    std::vector<std::string> positionals;

    auto value = [&](int &i, const char *flag) -> std::string {
        if (i + 1 >= argc) die(std::string("missing value for ") + flag);
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-i" || a == "--iterations") iterations = value(i, "-i");
        else if (a == "-l" || a == "--limit") limit = value(i, "-l");
        else if (a == "--stable-limit") stable_limit = value(i, "--stable-limit");
        else if (a == "-x") pos_x = value(i, "-x");
        else if (a == "-y") pos_y = value(i, "-y");
        else if (a == "--scale-x") scale_x = value(i, "--scale-x");
        else if (a == "--scale-y") scale_y = value(i, "--scale-y");
        else if (a == "-s" || a == "--scale") scale = value(i, "-s");
        else if (a == "-e" || a == "--exposure") {
            exposure = value(i, "-e");
            exposure_given = true;
        }
        else if (a == "--auto-exposure") { // a following 0.5 or 1.0 is the percentile; a bare integer is a <width>
            auto_exposure_on = true;
            if (i + 1 < argc && std::strpbrk(argv[i + 1], ".eE")) {
                char *end = nullptr;
                const double v = std::strtod(argv[i + 1], &end);
                if (end != argv[i + 1] && *end == '\0' && v >= 0.0 && v <= 1.0) {
                    auto_p = v;
                    i++;
                }
            }
        }
        else if (a.rfind("--auto-exposure=", 0) == 0) {
            auto_exposure_on = true;
            auto_p = to_f64(a.substr(16), "--auto-exposure");
            if (!(auto_p >= 0.0 && auto_p <= 1.0)) die("--auto-exposure takes a percentile within [0, 1]");
        }
        else if (a == "--distance-shade") distance_shade = value(i, "--distance-shade");
        else if (a == "--primary-color") primary = value(i, "--primary-color");
        else if (a == "--secondary-color") secondary = value(i, "--secondary-color");
        else if (a == "-d" || a == "--disable-inside") disable_inside = true;
        else if (a == "-u" || a == "--unsmooth") unsmooth = true;
        else if (a == "-o" || a == "--output") filename = value(i, "-o");
        else if (a == "-a" || a == "--algorithm") algo_s = value(i, "-a");
        else if (a == "--julia-real") julia_re = value(i, "--julia-real");
        else if (a == "--julia-imaginary") julia_im = value(i, "--julia-imaginary");
        else if (a == "-w" || a == "--color-weight") color_weight = value(i, "-w");
        else if (a == "--f32") f32 = true;       // this build's extension (no counterpart upstream)
        else if (a == "--perturbation") perturbation = true; // this build's extension: deep zooms on a wide centre
        else if (a == "--scaled") scaled = true; // SCALED PT: views past 2^440
        else if (a == "--bla") bla = true; // BLA-PT at the default bits
        else if (a.rfind("--bla=", 0) == 0) { // ... or at 24 .. 53 (written with '=': a bare number after --bla is <width>)
            bla = true;
            bla_bits = static_cast<int>(to_u32(a.substr(6), "--bla"));
            if (bla_bits < 24 || bla_bits > 53) die("--bla takes 24 .. 53 bits");
        }
        else if (a == "--adaptive") adaptive = true; // adaptive supersampling at the default threshold
        else if (a.rfind("--adaptive=", 0) == 0) { // ... or at -1 .. 255 (written with '=': a bare number after --adaptive is <width>)
            adaptive = true;
            char *end = nullptr;
            const long v = std::strtol(a.c_str() + 11, &end, 10);
            if (end == a.c_str() + 11 || *end != '\0' || v < -1 || v > 255) die("--adaptive takes a threshold of -1 .. 255");
            adaptive_t = static_cast<int>(v);
        }
        else if (a == "--linear-light") linear_light = true; // the samples are averaged as linear light
        else if (a == "--supersample") supersample_s = value(i, "--supersample"); // N x N samples per pixel, box-filtered on the device
        else if (a == "--devices") devices = value(i, "--devices");
        else if (a == "--threads") threads_s = value(i, "--threads");
        else if (a == "--seed") seed_s = value(i, "--seed");
        else if (a == "--quiet") quiet = true;
        else if (a == "--open" || a == "-g" || a == "--gui") die(a + " is not supported by this front end");
        else if (a.size() > 1 && a[0] == '-' && !(a[1] >= '0' && a[1] <= '9') && a[1] != '.') die("unknown flag " + a);
        else positionals.push_back(a);
    }
    if (positionals.size() > 2) die("too many positional arguments (expected <width> <height>)");
    if (!positionals.empty()) width = positionals[0];
    if (positionals.size() > 1) height = positionals[1];

    // Algo::from_str (calc/src/lib.rs:165-179): case-insensitive
    std::string al = algo_s;
    for (char &c : al) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
    Algo algo;
    if (al == "mandelbrot") algo = Algo::Mandelbrot;
    else if (al == "julia") algo = Algo::Julia;
    else if (al == "fern" || al == "barnsleyfern") algo = Algo::BarnsleyFern;
    else die("invalid algorithm name");
    if (algo == Algo::Julia && (!julia_re || !julia_im)) die("--julia-real and --julia-imaginary are required with -a julia");
    if ((scale_x || scale_y) && scale != "0.4") die("--scale conflicts with --scale-x/--scale-y");
    if (perturbation && (f32 || devices || algo == Algo::BarnsleyFern))
        die("--perturbation does not combine with --f32, --devices or -a fern");
    if (bla && !perturbation) die("--bla needs --perturbation");
    if (scaled && !perturbation) die("--scaled needs --perturbation");
    if (auto_exposure_on && exposure_given) die("--auto-exposure chooses the exposure: it does not combine with -e / --exposure");
    if (auto_exposure_on && algo == Algo::BarnsleyFern) die("--auto-exposure does not apply to -a fern: the fern has no escape indices");
    if (auto_exposure_on && devices && devices->find(',') != std::string::npos)
        die("--auto-exposure runs on one device: the statistics cover one array, not the pieces of --devices");
    if (adaptive) {
        if (!supersample_s) die("--adaptive needs --supersample: it chooses where the N x N samples are taken");
        if (distance_shade) die("--adaptive does not combine with --distance-shade");
        if (auto_exposure_on) die("--adaptive does not combine with --auto-exposure");
        if (f32) die("--adaptive does not combine with --f32: adaptive supersampling is defined on the f64 road and on --perturbation");
        if (devices) die("--adaptive does not combine with --devices: adaptive supersampling runs on one device");
        if (algo == Algo::BarnsleyFern) die("--adaptive does not apply to -a fern");
    }
    if (linear_light) {
        if (!supersample_s || to_u32(*supersample_s, "--supersample") <= 1)
            die("--linear-light needs --supersample above 1: it chooses how the N x N samples are averaged");
        if (algo == Algo::BarnsleyFern) die("--linear-light does not apply to -a fern");
    }
    if (distance_shade) {
        const uint32_t ss = supersample_s ? to_u32(*supersample_s, "--supersample") : 1;
        if (bla) die("--distance-shade does not combine with --bla: a skipped block has no per-step derivative");
        if (scaled) die("--distance-shade does not combine with --scaled: distance estimation is not defined on SCALED PT");
        if (ss > 1) die("--distance-shade does not combine with --supersample above 1");
        if (f32) die("--distance-shade does not combine with --f32: distance estimation is defined on the f64 road and on --perturbation");
        if (devices) die("--distance-shade does not combine with --devices: distance estimation runs on one device");
        if (auto_exposure_on) die("--distance-shade does not combine with --auto-exposure");
        if (algo == Algo::BarnsleyFern) die("--distance-shade does not apply to -a fern: the fern has no orbit derivative");
    }

    // src/lib.rs:207-226
    Config cfg = Config::make(algo);
    cfg.width = to_u32(width, "width");
    cfg.height = to_u32(height, "height");
    if (iterations) cfg.iterations = to_u32(*iterations, "iterations");
    cfg.limit = to_f64(limit, "limit");
    cfg.stable_limit = to_f64(stable_limit, "stable-limit");
    const std::string pos_x_s = pos_x ? *pos_x : (algo == Algo::Julia ? "0" : "-0.6"); /* src/lib.rs:66-72: 0 only for julia, so -0.6 for the fern too */
    cfg.pos.re = to_f64(pos_x_s, "-x");
    cfg.pos.im = to_f64(pos_y, "-y");
    cfg.scale.re = to_f64(scale_x ? *scale_x : scale, "scale");
    cfg.scale.im = to_f64(scale_y ? *scale_y : scale, "scale");
    cfg.exposure = to_f64(exposure, "exposure");
    cfg.inside = !disable_inside;
    cfg.smooth = !unsmooth;
    if (primary) {
        RGB c = parse_hex_rgb(*primary);
        cfg.primary_color = fr_rgb{c.r, c.g, c.b};
    }
    if (secondary) {
        RGB c = parse_hex_rgb(*secondary);
        cfg.secondary_color = fr_rgb{c.r, c.g, c.b};
    }
    cfg.color_weight = to_f64(color_weight, "color-weight");
    if (algo == Algo::Julia) {
        cfg.julia_set.re = to_f64(*julia_re, "--julia-real");
        cfg.julia_set.im = to_f64(*julia_im, "--julia-imaginary");
    }

    try {
        if (devices) {
            std::vector<int> list;
            size_t pos = 0;
            while (pos <= devices->size()) {
                const size_t comma = devices->find(',', pos);
                const std::string part = devices->substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
                list.push_back(static_cast<int>(to_u32(part, "--devices")));
                if (comma == std::string::npos) break;
                pos = comma + 1;
            }
            use_devices(list);
        }
        std::vector<RGB> image;
        const Transfer tf = linear_light ? Transfer::Srgb : Transfer::Bytes;
        uint64_t refined = 0; // --adaptive: the number of edge pixels
        const auto t0 = std::chrono::steady_clock::now();
        if (algo == Algo::BarnsleyFern) {
            uint32_t threads = threads_s ? to_u32(*threads_s, "--threads") : std::thread::hardware_concurrency();
            if (threads == 0) threads = 1;
            uint64_t seed = 0;
            if (seed_s) {
                char *end = nullptr;
                seed = std::strtoull(seed_s->c_str(), &end, 10);
                if (end == seed_s->c_str() || *end != '\0') die("invalid value for --seed: " + *seed_s);
            } else {
                std::random_device rd;
                seed = (static_cast<uint64_t>(rd()) << 32) | rd();
            }
            image = get_image_fern(cfg, threads, seed);
        } else if (distance_shade) {
            const double thickness = to_f64(*distance_shade, "--distance-shade");
            if (perturbation) {
                const WideCentre centre = WideCentre::from_decimal(pos_x_s, pos_y, WideCentre::words_for_scale(cfg.scale.re, cfg.scale.im));
                image = get_image_de(cfg, centre.c(), thickness);
            } else {
                image = get_image_de(cfg, thickness);
            }
        } else if (auto_exposure_on) {
            // the road's escape indices, their statistics on the device, then the colour map at the exposure they call for
            const uint32_t ss = supersample_s ? to_u32(*supersample_s, "--supersample") : 1;
            double chosen = 0.0;
            if (perturbation) {
                const WideCentre centre = WideCentre::from_decimal(pos_x_s, pos_y, WideCentre::words_for_scale(cfg.scale.re, cfg.scale.im));
                const fr_wide_centre wc = centre.c();
                image = get_image_auto(cfg, ss, auto_p, &chosen, [&](const Config &big, double *z, uint32_t *iters) {
                    if (scaled) check(fr_escape_rows_pt_scaled(&big, &wc, bla ? bla_bits : -1, 0, big.height, z, iters));
                    else if (bla) check(fr_escape_rows_pt_bla(&big, nullptr, &wc, bla_bits, 0, big.height, z, iters));
                    else check(fr_escape_rows_pt_wide(&big, &wc, 0, big.height, z, iters));
                }, tf);
            } else {
                image = get_image_auto(cfg, f32 ? FR_PRECISION_F32 : FR_PRECISION_F64, auto_p, ss, &chosen, tf);
            }
            if (!quiet) std::printf("auto-exposure %.17g (percentile %g of the escape indices)\n", chosen, auto_p);
        } else if (perturbation) {
            // the centre keeps every digit of -x / -y; cfg.pos (their f64 roundings) is not read
            const WideCentre centre = WideCentre::from_decimal(pos_x_s, pos_y, WideCentre::words_for_scale(cfg.scale.re, cfg.scale.im));
            if (adaptive) { // anti-aliased where the image has edges
                const uint32_t ss = to_u32(*supersample_s, "--supersample");
                const Adaptive ad{adaptive_t, &refined};
                if (scaled) image = get_image(cfg, centre.c(), Scaled{bla ? bla_bits : -1}, ss, ad, tf);
                else image = bla ? get_image(cfg, centre.c(), Bla{bla_bits}, ss, ad, tf) : get_image(cfg, centre.c(), ss, ad, tf);
            } else if (supersample_s) { // anti-aliased: the same road, N x N samples per pixel
                const uint32_t ss = to_u32(*supersample_s, "--supersample");
                if (scaled) image = get_image(cfg, centre.c(), Scaled{bla ? bla_bits : -1}, ss, tf);
                else image = bla ? get_image(cfg, centre.c(), Bla{bla_bits}, ss, tf) : get_image(cfg, centre.c(), ss, tf);
            } else if (scaled) image = get_image(cfg, centre.c(), Scaled{bla ? bla_bits : -1});
            else image = bla ? get_image(cfg, centre.c(), Bla{bla_bits}) : get_image(cfg, centre.c());
        } else {
            const int precision = f32 ? FR_PRECISION_F32 : FR_PRECISION_F64;
            if (adaptive) image = get_image(cfg, precision, to_u32(*supersample_s, "--supersample"), Adaptive{adaptive_t, &refined}, tf);
            else image = supersample_s ? get_image(cfg, precision, to_u32(*supersample_s, "--supersample"), tf) : get_image(cfg, precision);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const std::string path = filename + ".ppm";  // the reference appends ".avif" (src/lib.rs:192-195)
        std::FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) die("cannot open " + path);
        std::fprintf(f, "P6\n%u %u\n255\n", cfg.width, cfg.height);
        std::fwrite(image.data(), 3, image.size(), f);
        std::fclose(f);
        if (adaptive && !quiet) {
            const uint64_t npx = static_cast<uint64_t>(cfg.width) * cfg.height;
            std::printf("refined %llu of %llu pixels (%.1f%%) at threshold %d\n", static_cast<unsigned long long>(refined),
                        static_cast<unsigned long long>(npx), npx ? 100.0 * static_cast<double>(refined) / static_cast<double>(npx) : 0.0, adaptive_t);
        }
        if (!quiet) std::printf("rendered %ux%u in %.2f ms -> %s\n", cfg.width, cfg.height, ms, path.c_str());
    } catch (const Error &e) {
        std::fprintf(stderr, "fractal_hip error %d: %s\n", e.code(), e.what());
        return 1;
    }
    return 0;
}
