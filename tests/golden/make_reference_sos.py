"""The sum-of-squares Lyapunov candidate of ``examples/lyapunov_function_learning.ipynb`` (cell 17), run from
a checkout of the reference (``numpy_tf.REFERENCE_ROOT``, or the directory given as the first argument): the
reference's ``monomials`` / ``derivative_monomials`` (``examples/utilities.py:753-811``) behind the NumPy stand-in for TensorFlow (``numpy_tf``, like the other
``make_reference_*`` scripts), and the cell's two functions ``lyapunov_sos`` / ``lyapunov_sos_derivative``
and its matrix ``Q``, executed from the notebook's own text at generation time (the part of the cell in
front of its first use of the notebook's grid).  Nothing of that text is copied here.

* the column order of ``monomials(x, 3)``, recovered numerically (the exponents of every column);
* ``V`` and ``dV/d(state_norm * x)`` on 500 seeded states in [-1, 1]^2 and on a 41^2 grid, with the
  notebook's ``state_norm`` (cell 7: 180 and 360 degrees in radians).

Output ``reference_sos.npz``.  Data only.

    python tests/golden/make_reference_sos.py [REFERENCE_CHECKOUT]
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy_tf                                         # noqa: E402

OUT = os.path.join(HERE, "reference_sos.npz")
NUM_POINTS, SAMPLES, SEED = 41, 500, 17


def cell_17(namespace):
    """Executes the definitions of the notebook's SOS cell (everything in front of ``values_sos``)."""
    NOTEBOOK = os.path.join(numpy_tf.REFERENCE_ROOT, "examples", "lyapunov_function_learning.ipynb")
    with open(NOTEBOOK) as handle:
        cells = json.load(handle)["cells"]
    sources = ["".join(c["source"]) for c in cells if c["cell_type"] == "code"]
    (text,) = [s for s in sources if "def lyapunov_sos(" in s]
    head = text.split("\nvalues_sos", 1)[0]
    assert "lyapunov_sos_derivative" in head and "Q = np.array" in head
    exec(compile(head, NOTEBOOK + ":cell17", "exec"), namespace)


def column_exponents(monomials):
    """The exponents (a, b) of every column of ``monomials(x, 3)``: column(2, 1) = 2^a, column(1, 2) = 2^b."""
    a = np.log2(monomials(np.array([[2.0, 1.0]]), 3)[0])
    b = np.log2(monomials(np.array([[1.0, 2.0]]), 3)[0])
    exps = np.stack([a, b], axis=1)
    assert np.array_equal(exps, np.round(exps))
    probe = np.array([[1.5, -0.75]])
    assert np.array_equal(monomials(probe, 3)[0], np.prod(probe ** exps, axis=1))
    return exps.astype(np.int64)


def main():
    if len(sys.argv) > 1:
        numpy_tf.REFERENCE_ROOT = os.path.abspath(sys.argv[1])
    ref = numpy_tf.load_reference(examples=True)
    E = ref.examples
    state_norm = (np.deg2rad(180), np.deg2rad(360))                 # cell 7
    namespace = dict(np=np, monomials=E.monomials, derivative_monomials=E.derivative_monomials,
                     state_norm=state_norm)
    cell_17(namespace)
    Q = np.asarray(namespace["Q"], dtype=np.float64)
    value, derivative = namespace["lyapunov_sos"], namespace["lyapunov_sos_derivative"]
    rng = np.random.default_rng(SEED)
    states = rng.uniform(-1.0, 1.0, size=(SAMPLES, 2))
    axis = np.linspace(-1.0, 1.0, NUM_POINTS)
    grid = np.stack(np.meshgrid(axis, axis, indexing="ij"), axis=-1).reshape(-1, 2)
    out = dict(Q=Q, state_norm=np.asarray(state_norm, dtype=np.float64), degree=np.int64(3),
               exponents=column_exponents(E.monomials), states=states, grid_num_points=np.int64(NUM_POINTS),
               grid_points=grid)
    for key, pts in (("states", states), ("grid", grid)):
        out["value_" + key] = np.asarray(value(pts, Q, state_norm), dtype=np.float64).reshape(len(pts), 1)
        # the derivative with respect to the de-normalised argument z = state_norm * x
        out["dvdz_" + key] = np.asarray(derivative(pts, Q, state_norm), dtype=np.float64).reshape(len(pts), 2)
        assert np.isfinite(out["value_" + key]).all() and np.isfinite(out["dvdz_" + key]).all()
    print("Q: smallest eigenvalue %.4g, asymmetry %.3g" % (np.linalg.eigvalsh((Q + Q.T) / 2).min(), np.abs(Q - Q.T).max()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 292226


if __name__ == "__main__":
    main()
