// gp_floor_sim.cpp - stand-alone host program that runs gpfloor::variance_floor (sl_gp_floor.h, the
// routine sl_gp_set_head calls) on a factor written by the Python side.
//
//   gp_floor_sim <file>     the file holds doubles: n, panel height, stages, prior variance, then the
//                           row-major Linv[n][n]
//
// Prints the `stages` constants, one per line with 17 digits; exit status 1 with a message on a
// malformed file.  (tests/test_gp_floor_host.py builds it with -fsanitize=address,undefined.)
#include <cstdio>
#include <vector>

#include "sl_gp_floor.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: gp_floor_sim <file>\n");
        return 1;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "gp_floor_sim: cannot open %s\n", argv[1]);
        return 1;
    }
    double head[4];
    if (std::fread(head, sizeof(double), 4, f) != 4) {
        std::fprintf(stderr, "gp_floor_sim: short header\n");
        std::fclose(f);
        return 1;
    }
    const int n = (int)head[0], rp = (int)head[1], stages = (int)head[2];
    if (n < 1 || n > 8192 || rp < 1 || stages < 1 || stages != (n + rp - 1) / rp) {
        std::fprintf(stderr, "gp_floor_sim: bad sizes n=%d rp=%d stages=%d\n", n, rp, stages);
        std::fclose(f);
        return 1;
    }
    std::vector<double> linv((size_t)n * n);
    const size_t got = std::fread(linv.data(), sizeof(double), linv.size(), f);
    std::fclose(f);
    if (got != linv.size()) {
        std::fprintf(stderr, "gp_floor_sim: short factor\n");
        return 1;
    }
    std::vector<double> c((size_t)stages, -1.0);
    gpfloor::variance_floor(linv.data(), n, rp, stages, head[3], c.data());
    for (int s = 0; s < stages; ++s) std::printf("%.17g\n", c[s]);
    return 0;
}
