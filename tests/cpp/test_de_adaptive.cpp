// The C++ overload for ADAPTIVE SUPERSAMPLED DE on the F64 road (fractal-renderer_amd/host/fractal.hpp): the default Mandelbrot
// view is rendered through fractal::get_image_de(config, thickness, FR_PRECISION_F64, nullptr, supersample, AdaptiveDe{...}) and
// written as raw r,g,b bytes, the refined count printed; tests/test_gpu_ss_adaptive_de.py compares both with the C call's.
// Usage: test_de_adaptive WIDTH HEIGHT ITERATIONS THICKNESS SUPERSAMPLE THRESHOLD REACH OUT
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
        std::fprintf(stderr, "usage: %s WIDTH HEIGHT ITERATIONS THICKNESS SUPERSAMPLE THRESHOLD REACH OUT\n", argv[0]);
        return 2;
    }
    try {
        Config cfg = Config::make(Algo::Mandelbrot);
        cfg.width = static_cast<uint32_t>(std::atoi(argv[1]));
        cfg.height = static_cast<uint32_t>(std::atoi(argv[2]));
        cfg.iterations = static_cast<uint32_t>(std::atoi(argv[3]));
        const double thickness = std::atof(argv[4]);
        const uint32_t s = static_cast<uint32_t>(std::atoi(argv[5]));
        bool threw = false;
        try {
            get_image_de(cfg, thickness, FR_PRECISION_F64, nullptr, s, AdaptiveDe{8, -1.0, nullptr});
        } catch (const Error &e) {
            threw = e.code() == FR_ERR_INVALID_ARGUMENT;
        }
        EXPECT(threw);
        uint64_t refined = ~0ull;
        AdaptiveDe adaptive;
        EXPECT(adaptive.threshold == 8 && adaptive.reach == 2.0 && adaptive.refined == nullptr);
        adaptive.threshold = std::atoi(argv[6]);
        adaptive.reach = std::atof(argv[7]);
        adaptive.refined = &refined;
        const std::vector<RGB> image = get_image_de(cfg, thickness, FR_PRECISION_F64, nullptr, s, adaptive);
        EXPECT(image.size() == static_cast<size_t>(cfg.width) * cfg.height);
        // the BLA form on the (pos, pos_lo) road: the size alone is checked here
        EXPECT(get_image_de(cfg, Bla{}, thickness, nullptr, nullptr, s, AdaptiveDe{}).size() == image.size());
        std::FILE *f = std::fopen(argv[8], "wb");
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
