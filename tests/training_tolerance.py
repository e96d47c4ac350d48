"""The tolerance rule of the training-gradient tests (np_lyapunov_training, np_policy_training,
np_safe_policy_training and the host and GPU tests on them).

A gradient is compared with its float64 NumPy reference as ``|g - g_ref| <= tol * A``: ``A`` is the
reference's error companion (the same pass on absolute values) and ``tol`` is FACTOR times the
reference's OWN error - float64 against the same pass in long double, as a multiple of UNIT * A -
recorded per batch in the REFERENCE_RATIO table of the reference's module, or measured once.  Why 32
is enough room for what each kernel does differently stands with the ``tolerance`` of that module.
"""

import numpy as np

LONG = np.longdouble
UNIT = 2.0 ** -53
FACTOR = 32.0


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def ratio_to_companion(got, ref, comp, rows=None):
    """max |got - ref| / A in units of 2^-53 over arrays or lists of arrays (entries with A = 0 must agree
    exactly); ``rows``: a mask of the leading axis (points that are compared)."""
    worst = 0.0
    for g, r, a in zip(_as_list(got), _as_list(ref), _as_list(comp)):
        g, r, a = (np.asarray(v, dtype=LONG) for v in (g, r, a))
        if rows is not None:
            g, r, a = g[rows], r[rows], a[rows]
        diff = np.abs(g - r)
        assert np.all(diff[a == 0] == 0)
        if (a > 0).any():
            worst = max(worst, float((diff[a > 0] / a[a > 0]).max()))
    return worst * 2.0 ** 53


def recorded_or_measured(table, key, measure):
    """The recorded figure ``table[key]``; a key without one is measured (``measure(key)``) once and kept."""
    if key not in table:
        table[key] = measure(key)
    return table[key]


def tolerance(ratio):
    """FACTOR times a reference's own error ``ratio`` (in units of 2^-53 of A), as a multiple of A."""
    return FACTOR * ratio * UNIT
