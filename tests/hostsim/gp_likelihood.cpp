// gp_likelihood.cpp - TEST-ONLY host run of the per-element arithmetic and the tile / slot reduction of
// safe_learning_amd/csrc/sl_gp_likelihood.h (k_lml_grad and k_lml_reduce of sl_gp_likelihood.hip).
//
// A stand-alone program (run under the address and undefined-behaviour sanitizers where the toolchain has them):
//     gp_likelihood IN OUT
// IN:  int64 n, int64 p, int64 dout, the sl_gp_kernel description (its bytes), X [n][p], B [n][dout], K^-1 [n][n].
// OUT: double nslots, grad_variance [8][8], grad_inv_ls [8][8], grad_noise.
// The lanes of a wavefront are a loop here and the butterfly of the device is done on an array of 64; the order of
// every sum is the device's.  tests/test_gp_likelihood_host.py compares the result with the NumPy restatement
// (tests/np_gp_likelihood.py).  Never imported by the product package.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sl_gp_likelihood.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t shape[3];
    if (std::fread(shape, sizeof(int64_t), 3, in) != 3) return 4;
    const int64_t n = shape[0];
    const int p = (int)shape[1], dout = (int)shape[2];
    if (n < 1 || n > 4096 || p < 1 || p > SL_MAX_INPUT_DIM || dout < 1 || dout > 64) return 5;
    sl_gp_kernel ks;
    if (std::fread(&ks, sizeof(ks), 1, in) != 1) return 6;
    if (ks.nfactors < 1 || ks.nfactors > SL_KERNEL_MAX_FACTORS) return 7;
    std::vector<double> X((size_t)(n * p)), B((size_t)(n * dout)), kinv((size_t)(n * n));
    if (std::fread(X.data(), sizeof(double), X.size(), in) != X.size()) return 8;
    if (std::fread(B.data(), sizeof(double), B.size(), in) != B.size()) return 9;
    if (std::fread(kinv.data(), sizeof(double), kinv.size(), in) != kinv.size()) return 10;
    std::fclose(in);

    sl_lml_slots sl;
    if (sl_lml_compile_slots(ks, p, &sl) > SL_LML_MAX_SLOTS) return 11;
    const int nacc = sl.nslots + 1, nb = (int)((n + SL_LML_TILE - 1) / SL_LML_TILE);
    std::vector<double> partial((size_t)sl_lml_tiles(n) * nacc, 0.0);
    for (int I = 0; I < nb; ++I)
        for (int J = 0; J <= I; ++J) {
            double red[SL_LML_THREADS / 64][SL_LML_MAX_ACC] = {};
            for (int wave = 0; wave < SL_LML_THREADS / 64; ++wave)
                for (int e = 0; e < SL_LML_TILE / 4; ++e) {
                    const int64_t row = sl_lml_visit_row(n, I, wave, e);
                    if (row < 0) continue;
                    std::vector<sl_lml_entry> ent(64);
                    double coeff[64];
                    for (int lane = 0; lane < 64; ++lane)
                        coeff[lane] = sl_lml_lane(ks, n, p, dout, X.data(), B.data(), kinv.data(), row, J, lane, ent[lane]);
                    std::vector<double> terms((size_t)nacc * 64, 0.0);
                    for (int lane = 0; lane < 64; ++lane) {
                        int walked = 0;
                        sl_lml_walk(ks, p, ent[lane], [&](int s, double term) {
                            terms[(size_t)s * 64 + lane] = coeff[lane] * term;
                            ++walked;
                        });
                        if (walked != sl.nslots) return 13;
                        terms[(size_t)sl.nslots * 64 + lane] = (int64_t)J * SL_LML_TILE + lane == row ? coeff[lane] : 0.0;
                    }
                    for (int s = 0; s < nacc; ++s) {
                        double* v = &terms[(size_t)s * 64];
                        double w[64];
                        for (int off = 32; off >= 1; off >>= 1) {
                            for (int lane = 0; lane < 64; ++lane) w[lane] = v[lane] + v[lane ^ off];
                            for (int lane = 0; lane < 64; ++lane) v[lane] = w[lane];
                        }
                        red[wave][s] = red[wave][s] + v[0];
                    }
                }
            for (int s = 0; s < nacc; ++s) {
                double v = red[0][s];
                for (int w = 1; w < SL_LML_THREADS / 64; ++w) v = v + red[w][s];
                partial[(size_t)sl_lml_tile_index(I, J) * nacc + s] = v;
            }
        }
    std::vector<double> out(2 + 2 * 64, 0.0);
    out[0] = sl.nslots;
    for (int s = 0; s < nacc; ++s) {
        double v = 0.0;
        for (int t = 0; t < sl_lml_tiles(n); ++t) v = v + partial[(size_t)t * nacc + s];
        if (s == sl.nslots) out[1 + 128] = v;
        else out[1 + (sl.slot[s].what == SL_LML_INV_LS ? 64 : 0) + sl.slot[s].factor * 8 + sl.slot[s].q] = v;
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 12;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return 0;
}
