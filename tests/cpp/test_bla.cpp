// The C++ overloads for BLA-PT (fractal-renderer_amd/host/fractal.hpp): a view centred on two decimal strings is rendered
// through fractal::get_image(config, centre, Bla{bits}) and written as raw r,g,b bytes; tests/test_gpu_bla.py compares them
// with the C call's.  Usage: test_bla RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS OUT
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
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS OUT\n", argv[0]);
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
        bool threw = false;
        try {
            get_image(cfg, centre.c(), Bla{23});
        } catch (const Error &e) {
            threw = e.code() == FR_ERR_INVALID_ARGUMENT;
        }
        EXPECT(threw);
        const std::vector<RGB> image = get_image(cfg, centre.c(), Bla{std::atoi(argv[7])});
        // the (pos, pos_lo) road: a shallow view, the size alone is checked here
        Config shallow = Config::make(Algo::Mandelbrot);
        shallow.width = 24, shallow.height = 16, shallow.iterations = 200;
        EXPECT(get_image(shallow, Bla{}).size() == 24u * 16u);
        std::FILE *f = std::fopen(argv[8], "wb");
        EXPECT(f != nullptr);
        EXPECT(std::fwrite(image.data(), 3, image.size(), f) == image.size());
        std::fclose(f);
    } catch (const Error &e) {
        std::fprintf(stderr, "fractal_hip error %d: %s\n", e.code(), e.what());
        return 1;
    }
    return 0;
}
