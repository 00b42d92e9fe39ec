// The C++ overload for ADAPTIVE SUPERSAMPLED SCALED DE (fractal-renderer_amd/host/fractal.hpp): a view past 2^440 centred on two
// decimal strings is rendered through fractal::get_image_de(config, Scaled{bits}, centre, thickness, supersample, AdaptiveDe{...})
// and written as raw r,g,b bytes, the refined count printed; tests/test_gpu_ss_adaptive_de_scaled.py compares both with the C
// call's.  Usage: test_de_adaptive_scaled RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS THICKNESS SUPERSAMPLE THRESHOLD REACH TRANSFER OUT
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
    if (argc != 14) {
        std::fprintf(stderr, "usage: %s RE IM SCALE_LOG2 WIDTH HEIGHT ITERATIONS BITS THICKNESS SUPERSAMPLE THRESHOLD REACH TRANSFER OUT\n", argv[0]);
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
        const Scaled scaled{std::atoi(argv[7])};
        const double thickness = std::atof(argv[8]);
        const uint32_t s = static_cast<uint32_t>(std::atoi(argv[9]));
        const Transfer transfer = std::atoi(argv[12]) ? Transfer::Srgb : Transfer::Bytes;
        bool threw = false;
        try {
            get_image_de(cfg, scaled, c, thickness, s, AdaptiveDe{8, -1.0, nullptr});
        } catch (const Error &e) {
            threw = e.code() == FR_ERR_INVALID_ARGUMENT;
        }
        EXPECT(threw);
        uint64_t refined = ~0ull;
        AdaptiveDe adaptive;
        adaptive.threshold = std::atoi(argv[10]);
        adaptive.reach = std::atof(argv[11]);
        adaptive.refined = &refined;
        const std::vector<RGB> image = get_image_de(cfg, scaled, c, thickness, s, adaptive, transfer);
        EXPECT(image.size() == static_cast<size_t>(cfg.width) * cfg.height);
        // threshold -1 refines every pixel: the supersampled scaled form's bytes, whatever the reach
        uint64_t all = 0;
        const std::vector<RGB> every = get_image_de(cfg, scaled, c, thickness, s, AdaptiveDe{-1, 0.0, &all}, transfer);
        const std::vector<RGB> full = get_image_de(cfg, scaled, c, thickness, s, transfer);
        EXPECT(all == image.size() && std::memcmp(every.data(), full.data(), full.size() * sizeof(RGB)) == 0);
        std::FILE *f = std::fopen(argv[13], "wb");
        EXPECT(f != nullptr);
        EXPECT(std::fwrite(image.data(), 3, image.size(), f) == image.size());
        std::fclose(f);
        std::printf("refined %llu\n", static_cast<unsigned long long>(refined));
    } catch (const Error &e) {
        std::fprintf(stderr, "fractal_hip error %d: %s\n", e.code(), e.what());
        return 1;
    }
    return 0;
}
