// The C++ overload for DE ON BLA-PT (fractal-renderer_amd/host/fractal.hpp): a view centred on two decimal strings is rendered
// through fractal::get_image_de(config, Bla{bits}, thickness, nullptr, &centre) and written as raw r,g,b bytes;
// tests/test_gpu_de_bla.py compares them with the C calls'.  Usage: test_de_bla RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS
// THICKNESS OUT
#include <cmath>
#include <cstdio>
#include <cstdlib>

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
            get_image_de(cfg, Bla{54}, 1.0, nullptr, &c);
        } catch (const Error &e) {
            threw = e.code() == FR_ERR_INVALID_ARGUMENT;
        }
        EXPECT(threw);
        const std::vector<RGB> image = get_image_de(cfg, Bla{std::atoi(argv[7])}, std::atof(argv[8]), nullptr, &c);
        // the (pos, pos_lo) road: a shallow view, the size alone is checked here
        Config shallow = Config::make(Algo::Mandelbrot);
        shallow.width = 24, shallow.height = 16, shallow.iterations = 200;
        EXPECT(get_image_de(shallow, Bla{}).size() == 24u * 16u);
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
