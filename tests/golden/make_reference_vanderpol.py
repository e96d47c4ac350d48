"""The reference's own ``VanDerPol`` (``examples/utilities.py:440-519``) and ``compute_roa``
(``:654-686``), run unmodified from ``/root/reference`` behind the NumPy stand-in for TensorFlow
(``numpy_tf``), like ``make_reference_roa.py`` (build container only).

The stand-in's ``Lazy`` has no ``**`` (``x ** 2`` of the reference's ``ode``): it is added here, at run
time, as ``np.power`` - NumPy squares an integer exponent 2 as ``x * x``.

* one step of ``VanDerPol(1, dt=0.1)`` with ``normalization=[3, 3]`` and without, on seeded states
  of magnitude <= 1 (normalised);
* ``linearize()`` of both;
* the normalised system on ``GridWorld([[-1, 1]] * 2, 41)``, horizon 300, tol 0.01: mask, end
  states and the first steps of every trajectory.

Output ``reference_vanderpol.npz``.  Data only.

    python tests/golden/make_reference_vanderpol.py          (needs /root/reference)
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy_tf                                         # noqa: E402

OUT = os.path.join(HERE, "reference_vanderpol.npz")
DAMPING, DT, NORMALIZATION = 1, 0.1, [3, 3]
NUM_POINTS, HORIZON, TOL, TRAJ_STEPS = 41, 300, 0.01, 12


def main():
    numpy_tf.Lazy.__pow__ = lambda self, o: self._binary(o, np.power)
    ref = numpy_tf.load_reference(examples=True)
    tf = sys.modules["tensorflow"]
    numpy_tf.install_test_extras(tf)
    F, E = ref.functions, ref.examples
    rng = np.random.default_rng(20)
    states = rng.uniform(-1.0, 1.0, size=(500, 2))
    out = dict(damping=np.float64(DAMPING), dt=np.float64(DT), normalization=np.asarray(NORMALIZATION, dtype=np.float64),
               step_states=states)
    for key, norm in (("norm", NORMALIZATION), ("plain", None)):
        dynamics = E.VanDerPol(DAMPING, DT, norm)
        tf_states = tf.placeholder(ref.config.dtype, [None, 2], name="states")
        tf_actions = tf.placeholder(ref.config.dtype, [None, 1], name="actions")
        tf_next = dynamics(tf_states, tf_actions)
        out["step_" + key] = np.asarray(tf_next.eval({tf_states: states, tf_actions: np.zeros((len(states), 1))}))
        out["linearize_" + key] = np.asarray(dynamics.linearize())
        if norm is None:
            continue
        grid = F.GridWorld([[-1, 1]] * 2, NUM_POINTS)

        def closed_loop(x, _node=tf_next, _states=tf_states, _actions=tf_actions):
            with np.errstate(all="ignore"):                # trajectories outside the region blow up
                return np.asarray(_node.eval({_states: np.asarray(x), _actions: np.zeros((len(x), 1))}))

        roa, traj = E.compute_roa(grid, closed_loop, horizon=HORIZON, tol=TOL, no_traj=False)
        end = traj[:, :, -1]
        with np.errstate(all="ignore"):
            dist = np.linalg.norm(end, axis=1)
        band = (dist > TOL / 10) & (dist < 10 * TOL)
        print("vdp: %d cells, %d inside, %d non-finite, %d within a decade of tol, largest inside distance %.3g"
              % (grid.nindex, roa.sum(), (~np.isfinite(end).all(axis=1)).sum(), band.sum(), dist[roa].max()))
        assert roa.any() and not roa.all() and not band.any()
        out.update(roa_num_points=np.int64(NUM_POINTS), roa_horizon=np.int64(HORIZON), roa_tol=np.float64(TOL),
                   roa_points=np.asarray(grid.all_points), roa=np.asarray(roa, dtype=bool), roa_end=np.asarray(end),
                   roa_traj=np.asarray(traj[:, :, :TRAJ_STEPS]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
