"""Build ORACLE objects (test infrastructure) from the parameter dicts of
``safe_learning_amd.benchmarks.make_case`` - the same numbers the HIP engine gets."""

import numpy as np

import oracle
from safe_learning_amd.benchmarks import initial_safe_mask, make_case  # noqa: F401


ORACLE_KERNEL_LEAVES = {'rbf': oracle.np_functions.SlicedRBF, 'matern32': oracle.np_functions.Matern32,
                        'linear': oracle.np_functions.Linear}


def oracle_specs(case):
    if 'policy_table' in case:
        tab = case['policy_table']
        policy = oracle.Triangulation(oracle.GridWorld(case['limits'], tab['num_points']),
                                      tab['values'])
    else:
        policy = oracle.LinearSystem((case['K'],))
    if case['saturate'] is not None:
        policy = oracle.Saturation(policy, *case['saturate'])
    dyn = case['dynamics']
    if dyn['kind'] == 'linear':
        dynamics = oracle.LinearSystem((dyn['matrix'],))
    elif dyn['kind'] == 'pendulum':
        dynamics = oracle.InvertedPendulum(dyn['mass'], dyn['length'], dyn['friction'], dyn['dt'],
                                           dyn['normalization'])
    elif dyn['kind'] == 'cartpole':
        dynamics = oracle.CartPole(dyn['pendulum_mass'], dyn['cart_mass'], dyn['length'],
                                   dyn['rot_friction'], dyn['dt'], dyn['normalization'])
    else:
        d = case['d']
        if case['stack']:
            heads = []
            for k in range(d):
                if 'kernels' in dyn:
                    from safe_learning_amd.benchmarks import kernel_from_products
                    kern = kernel_from_products(dyn['kernels'][k], ORACLE_KERNEL_LEAVES)
                else:
                    kern = oracle.RBF(d + case['m'], dyn['variance'], dyn['lengthscales'][k], ARD=True)
                gp = oracle.GPRCached(dyn['X'], dyn['Y'][:, [k]], kern,
                                      oracle.LinearSystem((dyn['prior'][[k], :],)),
                                      likelihood_variance=dyn['noise_variance'])
                heads.append(oracle.GaussianProcess(gp, dyn['beta']))
            dynamics = oracle.FunctionStack(heads)
        else:
            kern = oracle.RBF(d + case['m'], dyn['variance'], dyn['lengthscales'], ARD=True)
            gp = oracle.GPRCached(dyn['X'], dyn['Y'], kern, oracle.LinearSystem((dyn['prior'],)),
                                  likelihood_variance=dyn['noise_variance'])
            dynamics = oracle.GaussianProcess(gp, dyn['beta'])
    vspec = case.get('V', {'kind': 'quadratic'})
    if vspec['kind'] == 'quadratic':
        value = oracle.QuadraticFunction(case['P'])
        gradient = None
    elif vspec['kind'] == 'network':
        value = oracle.LyapunovNetwork(case['d'], vspec['layer_dims'], vspec['activations'],
                                       vspec['eps'], vspec['weights'])
        gradient = value.gradient
    else:
        value = oracle.Triangulation(oracle.GridWorld(case['limits'],
                                                      vspec.get('num_points', case['num_points'])),
                                     vspec['values'], project=vspec.get('project', False))
        gradient = value.gradient
    kind, arg = (case['lv'] + (None,))[:2]
    if kind == 'const':
        lv = arg
    elif kind == 'abs_linear':
        lv = oracle.AbsFunction(oracle.LinearSystem((arg,)))
    elif kind == 'norm_linear':
        lv = oracle.Norm1Function(oracle.LinearSystem((arg,)))
    elif kind == 'abs_grad':
        lv = oracle.AbsFunction(gradient)
    else:
        lv = oracle.Norm1Function(gradient)
    return policy, dynamics, value, lv


def make_case_3d(num_points=(9, 10, 16), dynamics='linear', n_gp=300, seed=0, tau_scale=0.0,
                 signal_std=0.03, noise_std=0.0005, lengthscale=1.5, initial_radius=0.3):
    """A three-state case in ``make_case``'s format (test-only: the benchmark families are 1-D, 2-D
    and 4-D, the kernels are also compiled for d = 3).  A discrete chain of integrators with a
    little damping, x1' = x1 + h x2, x2' = x2 + h x3, x3' = x3 + h (u - 0.5 x3), under its saturated
    LQR law; V = x^T P x with P normalised, L_v = |2 P x|.  ``dynamics``: 'linear' or 'gp' (one RBF
    head over [x, u] trained on noisy samples of the chain, prior: the chain without damping)."""
    from safe_learning_amd.utilities import dlqr
    h = 0.1
    A = np.array([[1., h, 0.], [0., 1., h], [0., 0., 1. - 0.5 * h]])
    B = np.array([[0.], [0.], [h]])
    K, P = dlqr(A, B, np.eye(3), np.eye(1))
    P = P / np.abs(P).max()
    num_points = [int(n) for n in np.broadcast_to(num_points, (3,))]
    unit = 2.0 / (np.array(num_points) - 1)
    case = dict(name='chain3', stack=False, d=3, m=1, limits=[[-1., 1.]] * 3, num_points=num_points,
                K=-K, saturate=(-1., 1.), P=P, lv=('abs_linear', 2 * P),
                lf=float(np.linalg.norm(A, 1) + np.linalg.norm(B, 1) * np.linalg.norm(-K, 1)),
                tau=float(np.sum(unit) / 2) * tau_scale, initial_radius=initial_radius, A_true=A, B_true=B)
    if dynamics == 'linear':
        case['dynamics'] = {'kind': 'linear', 'matrix': np.hstack((A, B))}
    elif dynamics == 'gp':
        X = np.random.default_rng(seed).uniform(-1, 1, (n_gp, 4))
        Y = X @ np.hstack((A, B)).T + np.random.default_rng(seed + 1).normal(0, noise_std, (n_gp, 3))
        A_prior = A.copy()
        A_prior[2, 2] = 1.0
        case['dynamics'] = {'kind': 'gp', 'X': X, 'Y': Y, 'variance': signal_std ** 2,
                            'lengthscales': np.full(4, lengthscale), 'noise_variance': noise_std ** 2,
                            'prior': np.hstack((A_prior, B)), 'beta': 2.0}
    else:
        raise ValueError(dynamics)
    return case


class _LyapunovWithoutValues(oracle.Lyapunov):
    """For timing samples of huge grids: skip the all_points value table (8.6 GB at 128^4)."""

    def update_values(self):
        self.values = None


def oracle_lyapunov(case, compute_values=True, dynamics=None):
    """``dynamics``: a model to use instead of the case's own (kernel cases of gp_cases.py)."""
    grid = oracle.GridWorld(case['limits'], case['num_points'])
    policy, own_dynamics, value, lv = oracle_specs(case)
    dynamics = own_dynamics if dynamics is None else dynamics
    cls = oracle.Lyapunov if compute_values else _LyapunovWithoutValues
    return cls(grid, value, dynamics, case['lf'], lv, case['tau'], policy,
               initial_set=initial_safe_mask(case) if compute_values else None)


def oracle_cell_records(lyap, indices):
    """Per-cell [decrease, threshold, mean[d], err[d]] of the oracle (same layout as the
    engine's debug records)."""
    states = lyap.discretization.index_to_state(indices)
    actions = lyap.policy(states)
    nxt = lyap.dynamics(states, actions)
    decrease = lyap.v_decrease_bound(states, nxt)
    threshold = lyap.threshold(states, lyap.tau)
    if isinstance(nxt, tuple):
        mean, err = nxt
    else:
        mean, err = nxt, np.zeros_like(nxt)
    threshold = np.broadcast_to(threshold, decrease.shape)
    return np.hstack((decrease, threshold, mean, err))


def lyapunov_like_network_weights(P, layer_dims, scale=0.5, eps=1e-8):
    """LyapunovNetwork weights whose V is close to ``scale^2 x^T P x`` near the origin (a network
    that IS a Lyapunov candidate, unlike a randomly initialised one): the first layer's kernel
    ``W^T W + eps I`` equals ``scale^2 P`` and the remaining kernels pass the leading components
    through.  Variable order of ``examples/utilities.py:95-99``."""
    P = np.asarray(P, dtype=np.float64)
    d = len(P)
    weights, in_dim = [], d
    for i, out_dim in enumerate(layer_dims):
        hidden = int(np.ceil((in_dim + 1) / 2))
        W = np.zeros((hidden, in_dim))
        if i == 0:
            assert hidden >= d
            W[:d, :d] = np.linalg.cholesky(scale ** 2 * P - eps * np.eye(d)).T
        else:
            k = min(hidden, in_dim)
            W[:k, :k] = np.eye(k)
        weights.append(W)
        if out_dim > in_dim:
            weights.append(np.zeros((out_dim - in_dim, in_dim)))
        in_dim = out_dim
    return weights
