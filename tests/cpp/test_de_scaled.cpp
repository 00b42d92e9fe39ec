// The C++ overload for DE ON SCALED PT (fractal-renderer_amd/host/fractal.hpp): a view past 2^440 centred on two decimal strings is
// rendered through fractal::get_image_de(config, Scaled{bits}, centre, thickness) and written as raw r,g,b bytes;
// tests/test_gpu_de_scaled.py compares them with the C calls'.  Usage: test_de_scaled RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS
// THICKNESS OUT
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fractal.hpp"

#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

int main(int argc, char **argv) {
    using namespace fractal;
    if (argc != 10) {
        std::fprintf(stderr, "usage: %s RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS THICKNESS OUT\n", argv[0]);
        return 2;
    }
    try {
        Config cfg = Config::make(Algo::Mandelbrot);
        cfg.scale.re = cfg.scale.im = std::ldexp(1.0, std::atoi(argv[3]));
        cfg.width = static_cast<uint32_t>(std::atoi(argv[4]));
        cfg.height = static_cast<uint32_t>(std::atoi(argv[5]));
        cfg.iterations = static_cast<uint32_t>(std::atoi(argv[6]));
        cfg.limit = 2.0;
        const WideCentre centre = WideCentre::from_decimal(argv[1], argv[2], WideCentre::words_for_scale(cfg.scale.re, cfg.scale.im));
        const fr_wide_centre c = centre.c();
        bool threw = false;
        try {
            get_image_de(cfg, Scaled{23}, c, 1.0);
        } catch (const Error &e) {
            threw = e.code() == FR_ERR_INVALID_ARGUMENT;
        }
        EXPECT(threw);
        // the scaled view: 2^k = 0.5 * 2^(k+1)
        Config view = cfg;
        EXPECT(fr_de_scaled_view(&cfg, &view) == FR_OK);
        EXPECT(view.scale.re == 0.5 && view.scale.im == 0.5 && view.height == cfg.height && view.iterations == cfg.iterations);
        const std::vector<RGB> image = get_image_de(cfg, Scaled{std::atoi(argv[7])}, c, std::atof(argv[8]));
        EXPECT(image.size() == static_cast<size_t>(cfg.width) * cfg.height);
        // thickness 0 is the road's unshaded render
        const std::vector<RGB> flat = get_image_de(cfg, Scaled{std::atoi(argv[7])}, c, 0.0);
        const std::vector<RGB> render = get_image(cfg, c, Scaled{std::atoi(argv[7])});
        EXPECT(std::memcmp(flat.data(), render.data(), flat.size() * sizeof(RGB)) == 0);
        std::FILE *f = std::fopen(argv[9], "wb");
        EXPECT(f != nullptr);
        EXPECT(std::fwrite(image.data(), 3, image.size(), f) == image.size());
        std::fclose(f);
    } catch (const Error &e) {
        std::fprintf(stderr, "fractal_hip error %d: %s\n", e.code(), e.what());
        return 1;
    }
    return 0;
}
