// fractal.hpp's Transfer argument (include/fractal_hip.h, "LINEAR-LIGHT SUPERSAMPLING"): writes the raw r,g,b bytes of four
// renders of the default view at 67 x 35, 200 iterations, supersample 2, one after another, into the file named by argv[1]:
// get_image with Transfer::Srgb, with Transfer::Bytes, without the argument, and the adaptive form at threshold 8 with
// Transfer::Srgb.  tests/test_gpu_ss_linear.py compares them with the model.
#include <cstdio>

#include "fractal.hpp"

int main(int argc, char **argv) {
    using namespace fractal;
    if (argc != 2) return 2;
    try {
        Config cfg = Config::make(Algo::Mandelbrot);
        cfg.width = 67;
        cfg.height = 35;
        cfg.iterations = 200;
        uint64_t refined = 0;
        const std::vector<RGB> images[4] = {get_image(cfg, FR_PRECISION_F64, 2, Transfer::Srgb), get_image(cfg, FR_PRECISION_F64, 2, Transfer::Bytes),
                                            get_image(cfg, FR_PRECISION_F64, 2),
                                            get_image(cfg, FR_PRECISION_F64, 2, Adaptive{8, &refined}, Transfer::Srgb)};
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        for (const std::vector<RGB> &image : images) std::fwrite(image.data(), sizeof(RGB), image.size(), f);
        std::fclose(f);
        std::printf("refined %llu\n", static_cast<unsigned long long>(refined));
    } catch (const Error &e) {
        std::fprintf(stderr, "fractal_hip error %d: %s\n", e.code(), e.what());
        return 1;
    }
    return 0;
}
