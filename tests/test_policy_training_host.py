"""CPU checks of the policy-gradient path (PolicyIteration.action_gradient / policy_gradient,
NeuralNetwork.parameter_gradient, Triangulation.parameter_gradient, training.policy_improvement_step):
the NumPy reference the GPU tests compare with (tests/np_policy_training.py) is itself checked here, and so is
everything of the feature that runs without a GPU.

Measured here (printed by the tests; float64 on x86-64 with glibc):

* the reference against torch.autograd in float64 on the same graph (dense chain, GP mean with every kernel
  family, quadratic reward, the table as a gather with fixed simplices and a clamp): the largest |difference| / A
  stays below the reference's own error against long double on every case (ratios printed per case);
* the reference in float64 against the same evaluation in np.longdouble, max |g64 - g80| / A in units of 2^-53:
  action gradient (explicit actions / through the policy) lqr 1.12 / 2.07, pendulum 0.57 / 1.89, cartpole
  0.69 / 1.58, linear22 1.09 / 3.31; network parameter gradients per batch size 1 / 15 / 16 / 17 / 1000:
  [32, 32, 1] 47.5 / 114 / 16.7 / 37.2 / 134, [64, 64, 2] 8.42 / 3.3 / 2.33 / 3.2 / 1.16, [1] 1.75 / 0.30 /
  0.081 / 0.58 / 0.13, [17, 5, 1] 2.81 / 4.31 / 2.23 / 2.37 / 1.23; table gradients 0.32 ... 1.14; the steps of
  the two loops 0.12 ... 0.71 (1-D LQR) and 0.29 ... 3.73 (notebook shape).
  np_policy_training.REFERENCE_RATIO holds these figures rounded up; a GPU tolerance is 32 times its figure.
"""

import ctypes as C
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import hostsim_build
import np_policy_training as T
from oracle import np_functions as onp

EXTENDED = np.finfo(np.longdouble).eps < 1e-18


# ---- 1. the reference against torch autograd ------------------------------
def _torch_kernel(kern, X, Z):
    import torch
    if isinstance(kern, onp.Prod):
        out = _torch_kernel(kern.kern_list[0], X, Z)
        for member in kern.kern_list[1:]:
            out = out * _torch_kernel(member, X, Z)
        return out
    if isinstance(kern, onp.Add):
        return sum(_torch_kernel(member, X, Z) for member in kern.kern_list)
    active = list(range(kern.input_dim)) if isinstance(kern, onp.RBF) else [int(v) for v in kern.active_dims]
    Xa, Za = X[:, active], Z[:, active]
    if isinstance(kern, onp.Linear):
        return (Xa * torch.from_numpy(kern.variance)) @ Za.T
    ls = torch.from_numpy(np.asarray(kern.lengthscales, dtype=np.float64))
    r2 = (((Xa[:, None, :] - Za[None, :, :]) / ls) ** 2).sum(dim=2)
    if isinstance(kern, onp.Matern32):
        s = np.sqrt(3.0) * torch.sqrt(r2 + 1e-12)
        return kern.variance * (1 + s) * torch.exp(-s)
    return kern.variance * torch.exp(-r2 / 2)


def _torch_table(tri, points, params):
    """The table as TensorFlow differentiates it: a gather with the simplices the reference finds (fixed) and
    a clamp of the points."""
    import torch
    pts64 = points.detach().numpy()
    ids = tri.find_simplex(pts64)
    simplices = tri.simplices(ids)
    origins = torch.from_numpy(tri.discretization.index_to_state(simplices[:, 0]))
    H = torch.from_numpy(tri.hyperplanes[ids % tri.triangulation.nsimplex])
    if tri.project:
        lim = tri.discretization.limits
        points = torch.minimum(torch.maximum(points, torch.from_numpy(lim[:, 0].copy())),
                               torch.from_numpy(lim[:, 1].copy()))
    w1 = ((points - origins)[:, :, None] * H).sum(dim=1)
    w = torch.cat((1 - w1.sum(dim=1, keepdim=True), w1), dim=1)
    return (w[:, :, None] * params[torch.from_numpy(simplices)]).sum(dim=1)


def _torch_future_values(orl, x, u):
    import torch
    import scipy.linalg
    z = torch.cat((x, u), dim=1)
    d = x.shape[1]
    if isinstance(orl.dynamics, onp.LinearSystem):
        mean = z @ torch.from_numpy(orl.dynamics.matrix).T
    else:
        cols = []
        for gp, _ in T._gp_members(orl.dynamics):
            alpha = torch.from_numpy(scipy.linalg.solve_triangular(gp.cholesky.T, gp.alpha, lower=False))
            K = _torch_kernel(gp.kern, torch.from_numpy(gp.X), z)
            cols.append(K.T @ alpha + z @ torch.from_numpy(gp.mean_function.matrix).T)
        mean = torch.cat(cols, dim=1)
    assert mean.shape[1] == d
    P = torch.from_numpy(np.asarray(orl.reward_function.matrix, dtype=np.float64))
    reward = ((z @ P) * z).sum(dim=1)
    value = _torch_table(orl.value_function, mean, torch.from_numpy(orl.value_function.parameters))[:, 0]
    return reward + orl.gamma * value


def _torch_network(net, x, params):
    import torch
    acts = {None: lambda v: v, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}
    it, h = iter(params), x
    for l, name in enumerate(net.nonlinearities):
        h = h @ next(it)
        if net.use_bias and l < len(net.layers) - 1:
            h = h + next(it)
        h = acts[name](h)
    return h * net.output_scale


@pytest.mark.parametrize("explicit", [True, False], ids=["actions", "policy"])
@pytest.mark.parametrize("name", T.SYSTEMS)
def test_reference_action_gradient_matches_autograd(name, explicit):
    import torch
    orl, _ = T.system_pair(name)
    states, actions = T.system_states(name, 1000)
    u64 = actions if explicit else T.policy_actions(orl.policy, states)
    ok = T.comparable(orl, states, u64)
    print("%s: %.3f of the points left out" % (name, 1 - ok.mean()))
    assert 1 - ok.mean() <= T.MAX_EXCLUDED
    ref = T.action_gradient(orl, states, u64)
    u = torch.from_numpy(np.ascontiguousarray(u64)).requires_grad_(True)
    q = _torch_future_values(orl, torch.from_numpy(states), u)
    q.sum().backward()
    ratio = T.ratio_to_companion(u.grad.numpy(), ref["grad"], ref["A"], ok)
    print("%s (%s): autograd vs reference %.3f x 2^-53 of A (reference vs long double: %.3f)" % (
        name, "explicit actions" if explicit else "policy", ratio, T.REFERENCE_RATIO["action", name, explicit]))
    assert ratio * 2.0 ** -53 <= T.tolerance("action", name, explicit)
    assert_allclose(q.detach().numpy(), ref["q"], rtol=1e-12, atol=1e-13)
    assert_allclose(ref["q"], orl.future_values(states, actions=u64)[:, 0], rtol=1e-12, atol=1e-13)
    if orl.value_function.project:
        nxt = ref["next"]
        assert ((nxt < -1) | (nxt > 1)).any(axis=1)[ok].any(), "no successor outside the table: the mask is idle"


@pytest.mark.parametrize("key", sorted(T.NETWORKS))
def test_reference_network_gradient_matches_autograd(key):
    import torch
    onet, _ = T.make_network(key)
    for n in (1, 15, 16, 17, 1000):
        points, coeff = T.make_batch(key, n)
        ok = T.relu_margin(onet, points) > 1e-9
        assert 1 - ok.mean() <= T.MAX_EXCLUDED and (ok.all() or n > 50)
        points, coeff = points[ok], coeff[ok]
        assert (coeff == 0).all(axis=1).any() or n < 3
        ref, comp = T.network_parameter_gradient(onet, points, coeff)
        assert [g.shape for g in ref] == [p.shape for p in onet.parameters] == [a.shape for a in comp]
        params = [torch.from_numpy(p.copy()).requires_grad_(True) for p in onet.parameters]
        out = _torch_network(onet, torch.from_numpy(points), params)
        assert_allclose(out.detach().numpy(), onet(points), rtol=1e-12, atol=1e-15)
        (torch.from_numpy(coeff) * out).sum().backward()
        ratio = T.ratio_to_companion([p.grad.numpy() for p in params], ref, comp)
        print("%s, n = %d: autograd vs reference %.3f x 2^-53 of A (reference vs long double: %.3f)" % (
            key, n, ratio, T.REFERENCE_RATIO["network", key, n]))
        assert ratio * 2.0 ** -53 <= T.tolerance("network", key, n)
        assert all((a >= np.abs(g)).all() for g, a in zip(ref, comp))


@pytest.mark.parametrize("key", sorted(T.TABLES))
def test_reference_table_gradient_matches_autograd(key):
    import torch
    tri, points, coeff = T.table_case(key)
    ref, comp = T.table_parameter_gradient(tri, points, coeff)
    params = torch.from_numpy(tri.parameters.copy()).requires_grad_(True)
    out = _torch_table(tri, torch.from_numpy(points), params)
    assert_allclose(out.detach().numpy(), tri(points), rtol=1e-12, atol=1e-14)
    (torch.from_numpy(coeff) * out).sum().backward()
    ratio = T.ratio_to_companion(params.grad.numpy(), ref, comp)
    print("%s: autograd vs reference %.3f x 2^-53 of A (reference vs long double: %.3f)" % (
        key, ratio, T.REFERENCE_RATIO["table", key]))
    assert ratio * 2.0 ** -53 <= T.tolerance("table", key)
    lim = tri.discretization.limits
    assert ((points < lim[:, 0]) | (points > lim[:, 1])).any() and (ref != 0).all(axis=1).any()


@pytest.mark.parametrize("kind", ["steps-lqr", "steps-notebook"])
def test_reference_policy_gradient_matches_autograd(kind):
    """The whole chain - policy, dynamics, reward, table - differentiated with respect to the policy's
    parameters, at the initial parameters of the two step loops."""
    import torch
    if kind == "steps-lqr":
        orl, _ = T.lqr_pair(value_sweeps=1)
        states, reduction = orl.state_space, T.LQR_LOOP["reduction"]
        params = [torch.from_numpy(orl.policy.parameters.copy()).requires_grad_(True)]
        u = _torch_table(orl.policy, torch.from_numpy(states), params[0])
    else:
        orl, _ = T.system_pair("pendulum")
        states, reduction = T.notebook_states(orl), T.NOTEBOOK_LOOP["reduction"]
        params = [torch.from_numpy(p.copy()).requires_grad_(True) for p in orl.policy.parameters]
        u = _torch_network(orl.policy, torch.from_numpy(states), params)
    q = _torch_future_values(orl, torch.from_numpy(states), u)
    objective = q.sum() if reduction == 'sum' else q.mean()
    objective.backward()
    ref_objective, ref, comp = T.policy_gradient(orl, states, reduction)
    assert float(objective.detach()) == pytest.approx(float(ref_objective), rel=1e-12)
    got = [p.grad.numpy() for p in params]
    ratio = T.ratio_to_companion(got if isinstance(ref, list) else got[0], ref, comp)
    print("%s: autograd vs reference %.3f x 2^-53 of A" % (kind, ratio))
    assert ratio * 2.0 ** -53 <= T.tolerance(kind, 0 if kind == "steps-notebook" else 5)


def test_kernel_values_are_the_oracles():
    """kernel_terms evaluates the oracle's kernel classes: its K equals their ``K``."""
    for name in ("pendulum", "cartpole"):
        orl, _ = T.system_pair(name)
        states, actions = T.system_states(name, 50)
        z = np.hstack((states, actions))
        for gp, _ in T._gp_members(orl.dynamics):
            K = T.kernel_terms(gp.kern, gp.X, z, [states.shape[1]])[0]
            assert_allclose(K, gp.kern.K(gp.X, z), rtol=1e-12, atol=1e-18)
        mean = T.dynamics_terms(orl.dynamics, z, states.shape[1])[0]
        assert_allclose(mean, orl.dynamics(states, actions)[0], rtol=1e-10, atol=1e-13)


# ---- the recorded figures ------------------------------
def test_recorded_reference_ratios():
    """Every recorded figure is re-measured: it bounds the measurement and is not slack by more than 4."""
    # (the 131 149-point batches take up to half a minute each in long double: measured once with the same
    # function, 35.97, 0.1049, 0.01360 and 0.6192)
    keys = [k for k in T.REFERENCE_RATIO if k[0] in ("action", "network", "table") and k[-1] != 131149]
    measured = {k: T.measure_reference_ratio(k) for k in keys}
    for kind in ("steps-lqr", "steps-notebook"):
        for step, ratio in enumerate(T.measure_step_ratios(kind)):
            measured[kind, step] = ratio
    assert sorted(measured) == sorted(k for k in T.REFERENCE_RATIO if k[-1] != 131149)
    for key in sorted(measured):
        print("%s: float64 vs long double %.3f x 2^-53 of A (recorded %.3g)" % (key, measured[key],
                                                                                T.REFERENCE_RATIO[key]))
        if EXTENDED:
            assert 0.25 * T.REFERENCE_RATIO[key] <= measured[key] <= T.REFERENCE_RATIO[key], key


# ---- 2. + 3. the per-point arithmetic, compiled for the host ------------------------------
class _Head(C.Structure):
    """SlPgHead of safe_learning_amd/csrc/sl_policy_grad.h."""
    _fields_ = [("n", C.c_int), ("n_pad", C.c_int), ("dout", C.c_int), ("col0", C.c_int), ("variance", C.c_double),
                ("inv_ls", C.c_void_p), ("xs", C.c_void_p), ("alpha", C.c_void_p), ("kernel", C.c_void_p)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("policy_grad")
    exe = hostsim_build.program("policy_grad.cpp", out, hostsim_build.SHIM_FLAGS)
    assert subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.strip() == "policy_grad: ok"
    lib = hostsim_build.shared("policy_grad.cpp", out, hostsim_build.SHIM_FLAGS)
    lib.pg_dact.restype = C.c_double
    lib.pg_dact.argtypes = [C.c_int, C.c_double]
    return lib


def test_header_under_sanitizers(tmp_path_factory):
    """The stand-alone program of tests/hostsim/policy_grad.cpp under AddressSanitizer and UBSan, on its own."""
    exe = hostsim_build.program("policy_grad.cpp", tmp_path_factory.mktemp("policy_grad_san"),
                                hostsim_build.SHIM_FLAGS + ["-g"], sanitize=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "policy_grad: ok", run.stdout


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _tri_args(tri):
    grid = tri.discretization
    keep = [grid._desc(), np.ascontiguousarray(tri.unit_simplex_codes, dtype=np.int32),
            np.ascontiguousarray(tri.hyperplanes), np.ascontiguousarray(np.concatenate(grid.discrete_points))]
    return keep, [C.byref(keep[0]), len(keep[1]), _p(keep[1]), _p(keep[2]), _p(keep[3]), int(tri.project)]


def _shim_action_gradient(shim, name, states, actions):
    """The header on the product's own description of the system (no engine involved)."""
    import safe_learning_amd as sl
    from safe_learning_amd import _hip
    from safe_learning_amd.functions import _gp_heads, _is_plain_rbf
    import scipy.linalg
    orl, _ = T.system_pair(name)
    if name == "lqr":
        c = T.lqr_case()
        dynamics = sl.LinearSystem((c["a"], c["b"]))
    else:
        from safe_learning_amd.benchmarks import build_specs
        case = T.system_case(name)["case"]
        _, dynamics, _, _ = build_specs(dict(case, K=np.zeros((case["m"], case["d"])), saturate=None))
    d, m = states.shape[1], actions.shape[1]
    p = d + m
    vgrid = sl.GridWorld(orl.value_function.discretization.limits, orl.value_function.discretization.num_points)
    vf = sl.Triangulation(vgrid, orl.value_function.parameters.copy(), project=orl.value_function.project)
    keep, tri_args = _tri_args(vf)
    table = np.ascontiguousarray(vf.parameters)
    dyn, reward, value = _hip.DynamicsDesc(), _hip.ValueDesc(), _hip.ValueDesc()
    sl.QuadraticFunction(orl.reward_function.matrix)._write_value(reward)
    value.kind = _hip.V_TRI
    heads = (_Head * 6)()
    nheads = 0
    if isinstance(dynamics, sl.LinearSystem):
        dyn.kind = _hip.DYN_LINEAR
        for i in range(d):
            for j in range(p):
                dyn.matrix[i][j] = float(dynamics.matrix[i, j])
    else:
        dyn.kind = _hip.DYN_GP
        gps, _ = _gp_heads(dynamics)
        for gp, _, col0 in gps:
            mat = gp.mean_function.matrix
            for r in range(mat.shape[0]):
                for j in range(p):
                    dyn.matrix[col0 + r][j] = float(mat[r, j])
            alpha = np.ascontiguousarray(gp.cholesky_inverse.T.dot(gp.alpha))         # alpha' = Linv^T alpha
            h = heads[nheads]
            h.n = h.n_pad = len(gp.X)
            h.dout, h.col0 = alpha.shape[1], col0
            if _is_plain_rbf(gp.kern, p):
                ls = np.broadcast_to(np.asarray(gp.kern.lengthscales, dtype=np.float64), (p,))
                inv_ls, xs = np.ascontiguousarray(1.0 / ls), np.ascontiguousarray((gp.X / ls).T)
                h.variance, kernel = float(gp.kern.variance), None
            else:
                inv_ls, xs = np.ones(p), np.ascontiguousarray(gp.X.T)
                kernel = _hip.GpKernel()
                factors = gp.kern._factors(p)
                kernel.nfactors = len(factors)
                for f, (kind, product, variance, inv) in enumerate(factors):
                    kernel.factor[f].kind, kernel.factor[f].product = int(kind), int(product)
                    for q in range(p):
                        kernel.factor[f].variance[q] = float(variance[q])
                        kernel.factor[f].inv_lengthscales[q] = float(inv[q])
                h.kernel = C.cast(C.pointer(kernel), C.c_void_p)
            h.inv_ls, h.xs, h.alpha = _p(inv_ls).value, _p(xs).value, _p(alpha).value
            keep += [alpha, inv_ls, xs, kernel]
            nheads += 1
    n = len(states)
    states, actions = np.ascontiguousarray(states), np.ascontiguousarray(actions)
    grad, q, nxt = np.zeros((n, m)), np.zeros(n), np.zeros((n, d))
    rc = shim.pg_action_gradient(*tri_args, _p(table), C.byref(dyn), C.byref(reward), C.byref(value),
                                 C.c_double(orl.gamma), nheads, heads, d, m, C.c_int64(n), _p(states), _p(actions),
                                 _p(grad), _p(q), _p(nxt))
    assert rc == 0
    return orl, grad, q, nxt


@pytest.mark.parametrize("name", T.SYSTEMS)
def test_header_action_gradient_matches_reference(shim, name):
    states, actions = T.system_states(name, 1000)
    orl, grad, q, nxt = _shim_action_gradient(shim, name, states, actions)
    ok = T.comparable(orl, states, actions)
    assert 1 - ok.mean() <= T.MAX_EXCLUDED
    ref = T.action_gradient(orl, states, actions)
    ratio = T.ratio_to_companion(grad, ref["grad"], ref["A"], ok)
    print("%s: header vs reference %.3f x 2^-53 of A (tolerance %.1f)" % (
        name, ratio, 32 * T.REFERENCE_RATIO["action", name, True]))
    assert ratio * 2.0 ** -53 <= T.tolerance("action", name, True)
    assert_allclose(nxt, ref["next"], rtol=1e-12, atol=1e-14)
    assert_allclose(q[ok], ref["q"][ok], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("key", sorted(T.TABLES))
def test_header_table_pairs_match_reference(shim, key):
    import safe_learning_amd as sl
    tri, points, coeff = T.table_case(key)
    grid = sl.GridWorld(tri.discretization.limits, tri.discretization.num_points)
    stri = sl.Triangulation(grid, tri.parameters.copy(), project=tri.project)
    keep, tri_args = _tri_args(stri)
    n, k1 = len(points), grid.ndim + 1
    pts = np.ascontiguousarray(points)
    vert, w = np.zeros((n, k1), dtype=np.int64), np.zeros((n, k1))
    assert shim.pg_tri_locate(*tri_args, C.c_int64(n), _p(pts), _p(vert), _p(w)) == 0
    ref_w, ref_simplices, _ = T.table_weights(tri, points)
    # the same interpolant: the pairs give the table's values and the reference's gradient
    assert_allclose(np.sum(w[:, :, None] * tri.parameters[vert], axis=1), tri(points), rtol=1e-12, atol=1e-14)
    grad = np.zeros_like(tri.parameters)
    for i in range(n):
        for k in range(k1):
            grad[vert[i, k]] += coeff[i] * w[i, k]
    ref, comp = T.table_parameter_gradient(tri, points, coeff)
    ratio = T.ratio_to_companion(grad, ref, comp)
    print("%s: header pairs vs reference %.3f x 2^-53 of A" % (key, ratio))
    assert ratio * 2.0 ** -53 <= T.tolerance("table", key)


def test_header_activation_derivatives(shim):
    for code, name in ((0, None), (1, 'tanh'), (2, 'relu'), (3, 'sigmoid')):
        pre = np.array([-1.5, -1e-300, 0.0, 1e-300, 0.3, 2.0])
        post = T._act(name, pre)
        want = T._dact(name, pre, post)
        got = np.array([shim.pg_dact(code, float(v)) for v in post])
        if name == 'relu':
            assert_array_equal(got, want)                        # 1 for a pre-activation > 0, else 0
        else:
            assert_allclose(got, want, rtol=1e-15, atol=0)


# ---- 4. the reference's known answer ------------------------------
def test_reference_policy_iteration_known_answer():
    """safe_learning/tests/test_rl.py:29-77 with the module's step function: 10 x (one value-iteration sweep +
    5 gradient steps on the 5-vertex policy from -k/2 x) ends within the fixture's atol of the DLQR solution."""
    import oracle
    c = T.lqr_case()
    g = c["g"]
    orl, _ = T.lqr_pair(value_sweeps=0)
    objectives = []
    for _ in range(g["outer_iterations"]):
        orl.value_iteration()
        for _ in range(g["gd_steps"]):
            objectives.append(T.policy_improvement_step(orl, None, g["learning_rate"], 'sum')[0])
    true_value = oracle.QuadraticFunction(-c["p"])
    assert_allclose(orl.value_function.parameters, true_value(orl.state_space), atol=g["atol"])
    assert_allclose(orl.policy.parameters, -c["k"] * orl.policy.discretization.all_points, atol=g["atol"])
    assert (T.LQR_LOOP["outer"], T.LQR_LOOP["inner"], T.LQR_LOOP["learning_rate"]) == (
        g["outer_iterations"], g["gd_steps"], g["learning_rate"])
    # within a sweep's five steps the objective rises: the steps ascend J
    assert all(objectives[5 * k + 4] > objectives[5 * k] for k in range(g["outer_iterations"]))


# ---- the Python layer without a GPU ------------------------------
def test_package_exports_and_docstring():
    import safe_learning_amd as sl
    from safe_learning_amd import training
    assert sl.policy_improvement_step is training.policy_improvement_step
    for cls, names in ((sl.NeuralNetwork, ("parameter_gradient", "lipschitz")), (sl.Triangulation, ("parameter_gradient",)),
                       (sl.PolicyIteration, ("action_gradient", "policy_gradient"))):
        for name in names:
            assert hasattr(cls, name), (cls, name)
    assert "outside this package's scope" not in sl.NeuralNetwork.__doc__


def test_network_lipschitz_constant():
    import safe_learning_amd as sl
    onet, net = T.make_network("notebook", sl=_Networks(sl))
    want = abs(onet.output_scale)
    for w in onet.parameters:
        if w.ndim == 2:
            want *= np.linalg.norm(w, 2)
    assert net.lipschitz() == pytest.approx(want, rel=1e-13)
    # it IS a Lipschitz constant of the chain (contractive nonlinearities)
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-1, 1, (200, 2)), rng.uniform(-1, 1, (200, 2))
    slopes = np.abs(onet(a) - onet(b))[:, 0] / np.linalg.norm(a - b, axis=1)
    assert slopes.max() <= net.lipschitz()
    onet2, net2 = T.make_network("wide", sl=_Networks(sl))
    assert net2.lipschitz() > 0


class _Networks(object):
    def __init__(self, sl):
        self.NeuralNetwork = sl.NeuralNetwork
