// poly_value.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_poly_value.h.
//
// As a shared library tests/test_polynomial_value_host.py compares it bit for bit with the NumPy restatement
// (tests/np_polynomial_value.py); as a program (its own main, run under the address and undefined-behaviour
// sanitizers) it checks the table builder: the caps, exponents past the inputs, the gradient rows, an empty
// table, the last entry of a full table.  Never imported by the product package.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sl_model.h"

extern "C" {

// the table as sl_value_polynomial_set would store it; msg [240]
int polyv_build(int d, int nterms, const double* coef, const uint8_t* expo, int normalize, const double* tx,
                int32_t* row_start /* [SL_MAX_STATE_DIM + 2] */, double* out_coef /* [256] */,
                uint64_t* out_expo /* [256] */, char* msg) {
    SlPolyValue t;
    char local[240];
    const int rc = sl_polyv_build(&t, d, nterms, coef, expo, normalize, tx, msg ? msg : local, 240);
    if (rc != SL_OK) return rc;
    for (int i = 0; i < SL_MAX_STATE_DIM + 2; ++i) row_start[i] = t.row_start[i];
    std::memcpy(out_coef, t.coef, sizeof(t.coef));
    std::memcpy(out_expo, t.expo, sizeof(t.expo));
    return SL_OK;
}

// V and dV/dx of n states
int polyv_eval(int d, int nterms, const double* coef, const uint8_t* expo, int normalize, const double* tx,
               int negate, int64_t n, const double* states, double* value /* [n] */, double* grad /* [n][d] */) {
    SlPolyValue t;
    char msg[240];
    const int rc = sl_polyv_build(&t, d, nterms, coef, expo, normalize, tx, msg, sizeof(msg));
    if (rc != SL_OK) return rc;
    for (int64_t i = 0; i < n; ++i) {
        double x[SL_D] = {}, g[SL_D] = {};
        for (int k = 0; k < d; ++k) x[k] = states[i * d + k];
        value[i] = sl_polyv_value(t, d, negate, x);
        sl_polyv_gradient(t, d, negate, x, g);
        for (int k = 0; k < d; ++k) grad[i * d + k] = g[k];
    }
    return SL_OK;
}

}  // extern "C"

// ---- the program -------------------------------------------------------------------------------------------
static int g_failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
    } while (0)

static void expo_row(std::vector<uint8_t>& e, std::initializer_list<int> v) {
    int q = 0;
    for (int x : v) e.push_back((uint8_t)x), ++q;
    for (; q < SL_MAX_STATE_DIM; ++q) e.push_back(0);
}

int main() {
    SlPolyValue t;
    char msg[240];
    // V = 2 x^2 y - 3 y + 5 (a constant term) in two variables
    std::vector<double> coef = {2.0, -3.0, 5.0};
    std::vector<uint8_t> expo;
    expo_row(expo, {2, 1}); expo_row(expo, {0, 1}); expo_row(expo, {0, 0});
    CHECK(sl_polyv_build(&t, 2, 3, coef.data(), expo.data(), 0, nullptr, msg, sizeof(msg)) == SL_OK);
    // rows: value [0, 3), d/dx [3, 4) = 4 x y, d/dy [4, 6) = 2 x^2, -3; the others empty
    CHECK(t.row_start[0] == 0 && t.row_start[1] == 3 && t.row_start[2] == 4 && t.row_start[3] == 6);
    CHECK(t.row_start[4] == 6 && t.row_start[SL_MAX_STATE_DIM + 1] == 6 && t.nentries == 6 && t.nterms == 3);
    CHECK(t.coef[3] == 4.0 && t.expo[3] == 0x101u);
    CHECK(t.coef[4] == 2.0 && t.expo[4] == 0x002u && t.coef[5] == -3.0 && t.expo[5] == 0x0u);
    const double x[SL_D] = {0.5, -1.5};
    double g[SL_D];
    double acc = 0.0 + ((2.0 * 0.5) * 0.5) * -1.5;
    acc = acc + (-3.0 * -1.5);
    acc = acc + 5.0;
    CHECK(sl_polyv_value(t, 2, 0, x) == acc && sl_polyv_value(t, 2, 1, x) == acc * -1.0);
    sl_polyv_gradient(t, 2, 0, x, g);
    CHECK(g[0] == 0.0 + (4.0 * 0.5) * -1.5 && g[1] == (0.0 + (2.0 * 0.5) * 0.5) + -3.0);
    // normalised: z = x * T, the gradient carries T_k
    const double tx[SL_MAX_STATE_DIM] = {2.0, 4.0, 1.0, 1.0, 1.0, 1.0};
    CHECK(sl_polyv_build(&t, 2, 3, coef.data(), expo.data(), 1, tx, msg, sizeof(msg)) == SL_OK);
    double accn = 0.0 + ((2.0 * 1.0) * 1.0) * -6.0;
    accn = accn + (-3.0 * -6.0);
    accn = accn + 5.0;
    CHECK(sl_polyv_value(t, 2, 0, x) == accn);
    sl_polyv_gradient(t, 2, 1, x, g);
    CHECK(g[0] == (((0.0 + (4.0 * 1.0) * -6.0)) * 2.0) * -1.0);
    CHECK(sl_polyv_build(&t, 2, 3, coef.data(), expo.data(), 1, nullptr, msg, sizeof(msg)) == SL_ERR_INVALID);
    // an empty table: V = +0.0, the gradient +0.0; negated -0.0
    CHECK(sl_polyv_build(&t, 3, 0, nullptr, nullptr, 0, nullptr, msg, sizeof(msg)) == SL_OK);
    const double x3[SL_D] = {NAN, INFINITY, -1.0};
    CHECK(sl_polyv_value(t, 3, 0, x3) == 0.0 && !std::signbit(sl_polyv_value(t, 3, 0, x3)));
    CHECK(std::signbit(sl_polyv_value(t, 3, 1, x3)));
    sl_polyv_gradient(t, 3, 0, x3, g);
    CHECK(g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0);
    // the caps: degree, entries (value row + gradient rows), dimension, exponent past the inputs
    std::vector<double> ones(SL_POLYV_MAX_ENTRIES + 1, 1.0);
    std::vector<uint8_t> flat((SL_POLYV_MAX_ENTRIES + 1) * SL_MAX_STATE_DIM, 0);
    CHECK(sl_polyv_build(&t, 2, SL_POLYV_MAX_ENTRIES, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_OK);
    CHECK(t.row_start[1] == SL_POLYV_MAX_ENTRIES && t.row_start[SL_MAX_STATE_DIM + 1] == SL_POLYV_MAX_ENTRIES);
    const double x2[SL_D] = {1.0, 1.0};
    CHECK(sl_polyv_value(t, 2, 0, x2) == (double)SL_POLYV_MAX_ENTRIES);          // the last entry is read
    CHECK(sl_polyv_build(&t, 2, SL_POLYV_MAX_ENTRIES + 1, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_ERR_INVALID);
    CHECK(std::strstr(msg, "SL_POLYV_MAX_ENTRIES") != nullptr);
    flat[0] = 1;                                                  // one more entry in the row of d/dx
    CHECK(sl_polyv_build(&t, 2, SL_POLYV_MAX_ENTRIES, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_ERR_INVALID);
    CHECK(std::strstr(msg, "SL_POLYV_MAX_ENTRIES") != nullptr);
    CHECK(sl_polyv_build(&t, 2, SL_POLYV_MAX_ENTRIES - 1, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_OK);
    CHECK(t.row_start[1] == SL_POLYV_MAX_ENTRIES - 1 && t.row_start[2] == SL_POLYV_MAX_ENTRIES);
    flat[0] = SL_POLY_MAX_DEGREE;
    CHECK(sl_polyv_build(&t, 2, 1, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_OK);
    CHECK(t.coef[1] == (double)SL_POLY_MAX_DEGREE && t.expo[1] == (uint64_t)(SL_POLY_MAX_DEGREE - 1));
    flat[1] = 1;
    CHECK(sl_polyv_build(&t, 2, 1, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_ERR_INVALID);
    CHECK(std::strstr(msg, "SL_POLY_MAX_DEGREE") != nullptr);
    flat[0] = flat[1] = 0;
    flat[2] = 1;
    CHECK(sl_polyv_build(&t, 2, 1, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_ERR_INVALID);
    CHECK(sl_polyv_build(&t, 3, 1, ones.data(), flat.data(), 0, nullptr, msg, 240) == SL_OK);
    flat[2] = 0;
    CHECK(sl_polyv_build(&t, 0, 0, nullptr, nullptr, 0, nullptr, msg, 240) == SL_ERR_INVALID);
    CHECK(sl_polyv_build(&t, SL_MAX_STATE_DIM + 1, 0, nullptr, nullptr, 0, nullptr, msg, 240) == SL_ERR_INVALID);
    CHECK(sl_polyv_build(&t, 2, 1, nullptr, flat.data(), 0, nullptr, msg, 240) == SL_ERR_INVALID);
    // the widest table: six states, every variable in some term
    std::vector<double> wide_coef;
    std::vector<uint8_t> wide_expo;
    for (int k = 0; k < 36; ++k) {
        wide_coef.push_back(0.01 * (k + 1));
        for (int q = 0; q < SL_MAX_STATE_DIM; ++q) wide_expo.push_back((q == k % 6 ? 2 : 0) + (q == (k / 6) ? 1 : 0));
    }
    CHECK(sl_polyv_build(&t, SL_MAX_STATE_DIM, 36, wide_coef.data(), wide_expo.data(), 1, tx, msg, 240) == SL_OK);
    const double x6[SL_D] = {0.9, -0.8, 0.7, -0.6, 0.5, -0.4};
    CHECK(std::isfinite(sl_polyv_value(t, SL_MAX_STATE_DIM, 0, x6)));
    sl_polyv_gradient(t, SL_MAX_STATE_DIM, 0, x6, g);
    for (int k = 0; k < SL_MAX_STATE_DIM; ++k) CHECK(std::isfinite(g[k]) && g[k] != 0.0);
    std::printf(g_failures ? "%d check(s) failed\n" : "poly_value: all checks passed\n", g_failures);
    return g_failures ? 1 : 0;
}
