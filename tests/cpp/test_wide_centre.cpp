// The C++ overloads for WIDE PT (fractal-renderer_amd/host/fractal.hpp): a view centred on two decimal strings is rendered
// through fractal::get_image(config, centre) and written as raw r,g,b bytes; tests/test_gpu_pt_wide.py compares them with
// the library's image.  Usage: test_wide_centre RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS OUT
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
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS OUT\n", argv[0]);
        return 2;
    }
    try {
        Config cfg = Config::make(Algo::Mandelbrot);
        cfg.scale.re = cfg.scale.im = std::ldexp(1.0, std::atoi(argv[3]));
        cfg.width = static_cast<uint32_t>(std::atoi(argv[4]));
        cfg.height = static_cast<uint32_t>(std::atoi(argv[5]));
        cfg.iterations = static_cast<uint32_t>(std::atoi(argv[6]));
        cfg.limit = 2.0;
        const uint32_t words = WideCentre::words_for_scale(cfg.scale.re, cfg.scale.im);
        EXPECT(WideCentre::words_for_scale(std::ldexp(1.0, 200), 1.0) == 5 && WideCentre::words_for_scale(1.0, std::ldexp(1.0, 440)) == 9);
        EXPECT(WideCentre::words_for_scale(0.4, 0.4) == 2);
        WideCentre centre = WideCentre::from_decimal(argv[1], argv[2], words);
        // a pan step there and back leaves the words as they were; the hand-over pair is the nearest f64 and the rest
        const WideCentre before = centre;
        const double step = 3.0 / cfg.scale.re;
        centre.add(step, -step);
        EXPECT(centre.re != before.re && centre.im != before.im);
        centre.add(-step, step);
        EXPECT(centre.re == before.re && centre.im == before.im);
        const auto pair = centre.to_double();
        EXPECT(pair.first.re == std::strtod(argv[1], nullptr) && pair.first.im == std::strtod(argv[2], nullptr));
        EXPECT(std::fabs(pair.second.re) <= std::fabs(pair.first.re) * 0x1p-53);
        bool threw = false;
        try {
            WideCentre::from_decimal("2.5", "0", words);
        } catch (const Error &e) {
            threw = e.code() == FR_ERR_INVALID_ARGUMENT;
        }
        EXPECT(threw);
        const std::vector<RGB> image = get_image(cfg, centre.c());
        std::FILE *f = std::fopen(argv[7], "wb");
        EXPECT(f != nullptr);
        EXPECT(std::fwrite(image.data(), 3, image.size(), f) == image.size());
        std::fclose(f);
    } catch (const Error &e) {
        std::fprintf(stderr, "fractal_hip error %d: %s\n", e.code(), e.what());
        return 1;
    }
    return 0;
}
