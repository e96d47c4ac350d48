// sl_nn_train.h - per-sample arithmetic of the two training losses of
// examples/lyapunov_function_learning.ipynb (cells 25 and 30), shared by the kernel (k_nn_loss,
// sl_nn.hip) and the host tests.
//
// A loss is a mean over the batch of per-sample terms that are scalar functions of V at the state
// (and at its successor).  What training needs from a sample is the term itself and its derivative
// with respect to those values: the coefficient with which dV/dtheta of the point enters the
// gradient (sl_nn_param_grad sums coefficient * dV/dK over the points).  Every max(., 0) and |.| has
// derivative 0 at its kink, as TensorFlow's gradients of tf.maximum / tf.abs have, and the
// denominator of the decrease term is a constant of the differentiation (tf.stop_gradient).
//
// One rounding per operation, in the order written here (the library is built without
// contraction): the NumPy oracle of the tests repeats the lines and is compared bit for bit.
//
// Plain C++ on scalars: g++ compiles it for the tests.
#pragma once

#include "sl_model.h"

struct SlNnLossSample {
    double classifier;      // ROA: w * max(-(2 l - 1)(c - V(x)), 0);  ABS: |V(x) - target|
    double decrease;        // ROA: l * max(V(x+) - V(x), 0) / (V(x) + eps);  ABS: 0
    double objective;       // ROA: classifier + lambda * decrease;  ABS: classifier
    double coeff_x;         // d objective / d V(x), divided by the batch size
    double coeff_next;      // d objective / d V(x+), divided by the batch size (ABS: 0)
};

// SL_NN_LOSS_ROA, one sample: v = V(x), v_next = V(x+), label in {0, 1}, class weight w.
SL_HD SlNnLossSample sl_nn_loss_roa(double v, double v_next, double label, double weight, double safe_level,
                                    double lagrange, double eps, double batch) {
    SlNnLossSample s;
    const double sign = 2.0 * label - 1.0;
    const double hinge = -sign * (safe_level - v);              // -(2 l - 1)(c - V)
    const bool hinge_on = hinge > 0.0;
    s.classifier = weight * (hinge_on ? hinge : 0.0);
    const double dv = v_next - v;
    const bool dec_on = dv > 0.0;
    const double denom = v + eps;
    s.decrease = label * (dec_on ? dv : 0.0) / denom;
    s.objective = s.classifier + lagrange * s.decrease;
    // d hinge / d V = sign;  d decrease / d V(x+) = l / denom = -d decrease / d V(x)
    const double d_cls = hinge_on ? weight * sign : 0.0;
    const double d_dec = dec_on ? lagrange * (label / denom) : 0.0;
    s.coeff_x = (d_cls - d_dec) / batch;
    s.coeff_next = d_dec / batch;
    return s;
}

// SL_NN_LOSS_ABS, one sample: |V(x) - target|, coefficient sign(V(x) - target) / batch, sign(0) = 0.
SL_HD SlNnLossSample sl_nn_loss_abs(double v, double target, double batch) {
    SlNnLossSample s;
    const double diff = v - target;
    s.classifier = fabs(diff);
    s.decrease = 0.0;
    s.objective = s.classifier;
    const double sign = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
    s.coeff_x = sign / batch;
    s.coeff_next = 0.0;
    return s;
}
