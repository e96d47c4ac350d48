"""Discounted returns computed BY THE REFERENCE'S OWN ``reward_rollout`` (build container only).

``examples/utilities.py:522-545`` runs unmodified from ``/root/reference`` behind the NumPy stand-in
for TensorFlow (``numpy_tf``), on closed loops built from the reference's own classes:
``examples/utilities.py`` ``InvertedPendulum`` / ``CartPole`` and ``functions.py`` ``LinearSystem`` /
``Saturation`` / ``QuadraticFunction``.  The callables are what the notebooks hand to it
(``reinforcement_learning_pendulum.ipynb:397``): the graphs ``dynamics(states, policy(states))`` and
``reward(states, policy(states))`` evaluated with the states fed.

* pendulum, 41 x 41 grid, Q = diag(1, 2), R = 1.2; cart-pole, 7^4 grid, Q = R = 0.1 I: saturated LQR
  on the Euler models (the parameters of ``safe_learning_amd.benchmarks.make_case``), discount 0.98,
  horizon 1000, tol 1e-2; inputs, sums and the step count the reference prints.

Output ``reference_reward_rollout.npz``.  Data only.

    python tests/golden/make_reference_reward_rollout.py          (needs /root/reference)
"""

import contextlib
import io
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy_tf                                         # noqa: E402

OUT = os.path.join(HERE, "reference_reward_rollout.npz")
SCENARIOS = {"pendulum": dict(num_points=41, Q=np.diag([1.0, 2.0]), R=np.array([[1.2]])),
             "cartpole": dict(num_points=7, Q=0.1 * np.eye(4), R=np.array([[0.1]]))}
DISCOUNT, HORIZON, TOL = 0.98, 1000, 1e-2


def main():
    import scipy.linalg
    from safe_learning_amd.benchmarks import make_case
    ref = numpy_tf.load_reference(examples=True)
    tf = sys.modules["tensorflow"]
    numpy_tf.install_test_extras(tf)
    F, E = ref.functions, ref.examples
    out = {"discount": np.float64(DISCOUNT), "horizon": np.int64(HORIZON), "tol": np.float64(TOL)}
    for name, s in SCENARIOS.items():
        case = make_case(name, num_points=s["num_points"], dynamics="analytic")
        dyn = case["dynamics"]
        if name == "pendulum":
            dynamics = E.InvertedPendulum(dyn["mass"], dyn["length"], dyn["friction"], dyn["dt"],
                                          dyn["normalization"])
        else:
            dynamics = E.CartPole(dyn["pendulum_mass"], dyn["cart_mass"], dyn["length"], dyn["rot_friction"],
                                  dyn["dt"], dyn["normalization"])
        policy = F.Saturation(F.LinearSystem((case["K"],)), *case["saturate"])
        matrix = scipy.linalg.block_diag(-s["Q"], -s["R"])
        reward = F.QuadraticFunction(matrix)
        grid = F.GridWorld(case["limits"], case["num_points"])
        tf_states = tf.placeholder(ref.config.dtype, [None, case["d"]], name="states")
        tf_actions = policy(tf_states)
        tf_next = dynamics(tf_states, tf_actions)
        tf_reward = reward(tf_states, tf_actions)

        def closed_loop(x, _node=tf_next, _states=tf_states):
            return np.asarray(_node.eval({_states: np.asarray(x)}))

        def reward_eval(x, _node=tf_reward, _states=tf_states):
            return np.asarray(_node.eval({_states: np.asarray(x)}))

        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            rollout = E.reward_rollout(grid, closed_loop, reward_eval, DISCOUNT, horizon=HORIZON, tol=TOL)
        said = printed.getvalue().strip()
        steps = int(re.search(r"converged after (\d+) steps", said).group(1))
        print("%s: %d cells, reference says %r, minimum %.16g" % (name, grid.nindex, said, rollout.min()))
        out[name + "_limits"] = np.asarray(case["limits"], dtype=np.float64)
        out[name + "_num_points"] = np.asarray(case["num_points"], dtype=np.int64)
        out[name + "_reward_matrix"] = np.asarray(matrix, dtype=np.float64)
        out[name + "_points"] = np.asarray(grid.all_points)
        out[name + "_rollout"] = np.asarray(rollout, dtype=np.float64)
        out[name + "_steps"] = np.int64(steps)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
