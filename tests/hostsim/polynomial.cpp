// polynomial.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_polynomial.h (through sl_model.h's
// sl_dynamics_det, the way the kernels reach it).
//
// As a shared library tests/test_polynomial_host.py compares it bit for bit with the NumPy restatement
// (tests/np_polynomial.py); as a program (its own main, run under the address and undefined-behaviour
// sanitizers) it checks the table builder: the caps, rows out of range, exponents past the inputs, empty
// rows, no terms at all, the stable sort by row.  Never imported by the product package.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sl_model.h"

extern "C" {

// the table as sl_dynamics_polynomial_set would store it; msg [200]
int poly_build(int d, int m, int nterms, const int32_t* rows, const double* coef, const uint8_t* expo, int substeps,
               double h, int32_t* row_start /* [8] */, double* out_coef /* [64] */, uint64_t* out_expo /* [64] */,
               char* msg) {
    SlPolyTable t;
    char local[200];
    const int rc = sl_poly_build(&t, d, m, nterms, rows, coef, expo, substeps, h, msg ? msg : local, 200);
    if (rc != SL_OK) return rc;
    for (int i = 0; i < SL_MAX_STATE_DIM + 2; ++i) row_start[i] = t.row_start[i];
    std::memcpy(out_coef, t.coef, sizeof(t.coef));
    std::memcpy(out_expo, t.expo, sizeof(t.expo));
    return SL_OK;
}

// x+ of n (state, action) rows under the description's normalisation; fixed_dims != 0: d and m as the
// kernels compiled for fixed dimensions pass them (the same code: they are plain arguments)
int poly_eval(const sl_dynamics_desc* desc, int d, int m, int nterms, const int32_t* rows, const double* coef,
              const uint8_t* expo, int substeps, double h, int64_t n, const double* states, const double* actions,
              double* out) {
    SlPolyTable t;
    char msg[200];
    const int rc = sl_poly_build(&t, d, m, nterms, rows, coef, expo, substeps, h, msg, sizeof(msg));
    if (rc != SL_OK) return rc;
    SlDevModel M;
    std::memset(&M, 0, sizeof(M));
    M.m.dynamics = *desc;
    M.m.grid.d = d;
    M.m.policy.m = m;
    M.in_dim = d + m;
    M.poly = &t;
    const SlDims nd = sl_dims<0, 0>(M);
    for (int64_t i = 0; i < n; ++i) {
        double z[SL_P] = {}, u[SL_M] = {}, nxt[SL_D];
        for (int k = 0; k < d; ++k) z[k] = states[i * d + k];
        for (int a = 0; a < m; ++a) u[a] = actions[i * m + a];
        sl_append_action(nd, u, z);
        sl_dynamics_det<0>(M, nd, z, nxt);
        for (int k = 0; k < d; ++k) out[i * d + k] = nxt[k];
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
    for (; q < SL_MAX_INPUT_DIM; ++q) e.push_back(0);
}

int main() {
    SlPolyTable t;
    char msg[200];
    // Van der Pol, the terms given out of row order: sorted by row, the caller's order kept within a row
    std::vector<int32_t> rows = {1, 0, 1, 1};
    std::vector<double> coef = {1.0, -1.0, 0.5, -0.5};
    std::vector<uint8_t> expo;
    expo_row(expo, {1, 0, 0}); expo_row(expo, {0, 1, 0}); expo_row(expo, {2, 1, 0}); expo_row(expo, {0, 1, 0});
    CHECK(sl_poly_build(&t, 2, 1, 4, rows.data(), coef.data(), expo.data(), 10, 0.01, msg, sizeof(msg)) == SL_OK);
    CHECK(t.row_start[0] == 0 && t.row_start[1] == 1 && t.row_start[2] == 4 && t.row_start[7] == 4);
    CHECK(t.coef[0] == -1.0 && t.coef[1] == 1.0 && t.coef[2] == 0.5 && t.coef[3] == -0.5);
    CHECK(t.expo[0] == 0x100u && t.expo[1] == 0x1u && t.expo[2] == 0x102u && t.expo[3] == 0x100u);
    CHECK(t.d == 2 && t.m == 1 && t.nterms == 4 && t.substeps == 10 && t.h == 0.01);
    // one sub-step by hand, in the documented order
    sl_dynamics_desc f;
    std::memset(&f, 0, sizeof(f));
    t.substeps = 1;
    const double z[SL_P] = {0.3, -0.7, 123.0};
    double nxt[SL_D];
    sl_polynomial(f, t, 2, 1, z, nxt);
    const double a0 = 0.0 + (-1.0 * -0.7);
    double a1 = 0.0 + (1.0 * 0.3);
    a1 = a1 + (((0.5 * 0.3) * 0.3) * -0.7);
    a1 = a1 + (-0.5 * -0.7);
    CHECK(nxt[0] == 0.3 + 0.01 * a0 && nxt[1] == -0.7 + 0.01 * a1);
    // a map (substeps = 0) with an empty row: that row's next state is +0.0; a NaN passes through
    t.substeps = 0;
    t.row_start[1] = t.row_start[2] = 1;                          // row 1 has no term
    const double zn[SL_P] = {NAN, 2.0, 0.0};
    sl_polynomial(f, t, 2, 1, zn, nxt);
    CHECK(nxt[0] == 2.0 * -1.0 && nxt[1] == 0.0 && !std::signbit(nxt[1]));
    const double zi[SL_P] = {1.0, INFINITY, 0.0};
    sl_polynomial(f, t, 2, 1, zi, nxt);
    CHECK(nxt[0] == -INFINITY);
    // no terms at all: the zero field (a state stays), the zero map
    CHECK(sl_poly_build(&t, 3, 2, 0, nullptr, nullptr, nullptr, 4, 0.5, msg, sizeof(msg)) == SL_OK);
    CHECK(t.row_start[0] == 0 && t.row_start[3] == 0 && t.nterms == 0);
    const double z3[SL_P] = {1.5, -2.5, 3.5, 9.0, 9.0};
    sl_polynomial(f, t, 3, 2, z3, nxt);
    CHECK(nxt[0] == 1.5 && nxt[1] == -2.5 && nxt[2] == 3.5);
    // the caps
    std::vector<int32_t> many(SL_POLY_MAX_TERMS + 1, 0);
    std::vector<double> ones(SL_POLY_MAX_TERMS + 1, 1.0);
    std::vector<uint8_t> flat((SL_POLY_MAX_TERMS + 1) * SL_MAX_INPUT_DIM, 0);
    CHECK(sl_poly_build(&t, 2, 1, SL_POLY_MAX_TERMS, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_OK);
    CHECK(t.row_start[1] == SL_POLY_MAX_TERMS && t.row_start[2] == SL_POLY_MAX_TERMS);
    CHECK(sl_poly_build(&t, 2, 1, SL_POLY_MAX_TERMS + 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) ==
          SL_ERR_INVALID);
    CHECK(std::strstr(msg, "SL_POLY_MAX_TERMS") != nullptr);
    flat[0] = SL_POLY_MAX_DEGREE - 1; flat[2] = 1;
    CHECK(sl_poly_build(&t, 2, 1, 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_OK);
    flat[1] = 1;
    CHECK(sl_poly_build(&t, 2, 1, 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(std::strstr(msg, "SL_POLY_MAX_DEGREE") != nullptr);
    flat[0] = flat[1] = flat[2] = 0;
    // a row out of range, an exponent past the d + m inputs, bad dimensions, negative sub-steps, NULL arrays
    many[0] = 2;
    CHECK(sl_poly_build(&t, 2, 1, 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_ERR_INVALID);
    many[0] = -1;
    CHECK(sl_poly_build(&t, 2, 1, 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_ERR_INVALID);
    many[0] = 0;
    flat[3] = 1;
    CHECK(sl_poly_build(&t, 2, 1, 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(sl_poly_build(&t, 2, 2, 1, many.data(), ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_OK);
    flat[3] = 0;
    CHECK(sl_poly_build(&t, 0, 1, 0, nullptr, nullptr, nullptr, 1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(sl_poly_build(&t, SL_MAX_STATE_DIM + 1, 1, 0, nullptr, nullptr, nullptr, 1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(sl_poly_build(&t, 2, 0, 0, nullptr, nullptr, nullptr, 1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(sl_poly_build(&t, 2, SL_MAX_ACTION_DIM + 1, 0, nullptr, nullptr, nullptr, 1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(sl_poly_build(&t, 2, 1, 0, nullptr, nullptr, nullptr, -1, 1.0, msg, 200) == SL_ERR_INVALID);
    CHECK(sl_poly_build(&t, 2, 1, 1, nullptr, ones.data(), flat.data(), 1, 1.0, msg, 200) == SL_ERR_INVALID);
    // the widest model: every state row and every input used, the last term of the table read
    std::vector<int32_t> wide_rows;
    std::vector<double> wide_coef;
    std::vector<uint8_t> wide_expo;
    for (int k = 0; k < SL_POLY_MAX_TERMS; ++k) {
        wide_rows.push_back(k % SL_MAX_STATE_DIM);
        wide_coef.push_back(0.01 * (k + 1));
        for (int q = 0; q < SL_MAX_INPUT_DIM; ++q) wide_expo.push_back(q == k % SL_MAX_INPUT_DIM ? SL_POLY_MAX_DEGREE : 0);
    }
    CHECK(sl_poly_build(&t, SL_MAX_STATE_DIM, SL_MAX_ACTION_DIM, SL_POLY_MAX_TERMS, wide_rows.data(), wide_coef.data(),
                        wide_expo.data(), 3, 0.1, msg, 200) == SL_OK);
    CHECK(t.row_start[SL_MAX_STATE_DIM] == SL_POLY_MAX_TERMS);
    const double z8[SL_P] = {0.9, -0.8, 0.7, -0.6, 0.5, -0.4, 0.3, -0.2};
    sl_polynomial(f, t, SL_MAX_STATE_DIM, SL_MAX_ACTION_DIM, z8, nxt);
    for (int k = 0; k < SL_MAX_STATE_DIM; ++k) CHECK(std::isfinite(nxt[k]) && nxt[k] != z8[k]);
    std::printf(g_failures ? "%d check(s) failed\n" : "polynomial: all checks passed\n", g_failures);
    return g_failures ? 1 : 0;
}
