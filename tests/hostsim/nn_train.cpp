// nn_train.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_nn_train.h.
//
// The per-sample arithmetic of k_nn_loss, compiled with g++ from the same header, over arrays of
// network values, so that tests/test_lyapunov_training_host.py can compare every term and
// coefficient with the NumPy reference (tests/np_lyapunov_training.py) bit for bit without a GPU.
// The test loads it as a shared library; built as a program, main() checks a few hand-worked samples.  Never imported by the product package.
#include <cstdint>
#include <cstdio>
#include "sl_nn_train.h"

extern "C" {

// out [5][m]: classifier, decrease, objective, coeff_x, coeff_next
int nt_roa(int64_t m, const double* v, const double* v_next, const double* labels, const double* weights,
           double safe_level, double lagrange, double eps, double* out) {
    for (int64_t i = 0; i < m; ++i) {
        const SlNnLossSample s = sl_nn_loss_roa(v[i], v_next[i], labels[i], weights[i], safe_level, lagrange, eps,
                                                (double)m);
        out[i] = s.classifier;
        out[m + i] = s.decrease;
        out[2 * m + i] = s.objective;
        out[3 * m + i] = s.coeff_x;
        out[4 * m + i] = s.coeff_next;
    }
    return 0;
}

int nt_abs(int64_t m, const double* v, const double* targets, double* out) {
    for (int64_t i = 0; i < m; ++i) {
        const SlNnLossSample s = sl_nn_loss_abs(v[i], targets[i], (double)m);
        out[i] = s.classifier;
        out[m + i] = s.decrease;
        out[2 * m + i] = s.objective;
        out[3 * m + i] = s.coeff_x;
        out[4 * m + i] = s.coeff_next;
    }
    return 0;
}

}  // extern "C"

static int expect(const char* what, double got, double want) {
    if (got == want) return 0;
    std::printf("%s: got %.17g, expected %.17g\n", what, got, want);
    return 1;
}

int main() {
    int bad = 0;
    // inside the level set, labelled inside, decreasing: nothing to pay, nothing to push
    SlNnLossSample s = sl_nn_loss_roa(0.5, 0.25, 1.0, 2.0, 1.0, 10.0, 0.0, 4.0);
    bad += expect("inactive objective", s.objective, 0.0) + expect("inactive coeff_x", s.coeff_x, 0.0) +
           expect("inactive coeff_next", s.coeff_next, 0.0);
    // outside, labelled inside, increasing: hinge 0.5 * weight 2, decrease 0.5 / 1.5 * 3
    s = sl_nn_loss_roa(1.5, 2.0, 1.0, 2.0, 1.0, 3.0, 0.0, 4.0);
    bad += expect("classifier", s.classifier, 1.0) + expect("decrease", s.decrease, 0.5 / 1.5) +
           expect("coeff_x", s.coeff_x, (2.0 - 3.0 * (1.0 / 1.5)) / 4.0) +
           expect("coeff_next", s.coeff_next, 3.0 * (1.0 / 1.5) / 4.0);
    // labelled outside: the decrease term is switched off, the hinge pushes V up
    s = sl_nn_loss_roa(0.5, 2.0, 0.0, 1.0, 1.0, 3.0, 0.0, 2.0);
    bad += expect("outside classifier", s.classifier, 0.5) + expect("outside decrease", s.decrease, 0.0) +
           expect("outside coeff_x", s.coeff_x, -0.5) + expect("outside coeff_next", s.coeff_next, 0.0);
    // the kinks: derivative 0
    s = sl_nn_loss_roa(1.0, 1.0, 1.0, 1.0, 1.0, 3.0, 0.0, 1.0);
    bad += expect("kink coeff_x", s.coeff_x, 0.0) + expect("kink coeff_next", s.coeff_next, 0.0);
    s = sl_nn_loss_abs(0.25, 0.25, 8.0);
    bad += expect("abs kink", s.coeff_x, 0.0) + expect("abs kink loss", s.objective, 0.0);
    s = sl_nn_loss_abs(0.25, 0.75, 8.0);
    bad += expect("abs", s.objective, 0.5) + expect("abs coeff", s.coeff_x, -0.125);
    std::printf(bad ? "nn_train: %d mismatches\n" : "nn_train: ok\n", bad);
    return bad ? 1 : 0;
}
