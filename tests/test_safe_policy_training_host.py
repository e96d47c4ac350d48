"""CPU checks of the safe policy update (Lyapunov.decrease_gradient, PolicyIteration.action_gradient /
policy_gradient(..., lyapunov=), training.policy_improvement_step(..., lyapunov=)): the NumPy reference the GPU
tests compare with (tests/np_safe_policy_training.py) is itself checked here - against central differences of the
oracle's own future_values(..., lyapunov=), against torch autograd through torch.linalg.solve_triangular, against
its own long-double run - and so is everything of the feature that runs without a GPU: the per-point
arithmetic of safe_learning_amd/csrc/sl_safe_grad.h built with g++ (tests/hostsim/safe_grad.cpp) and the Python
layer on a stand-in engine.  Every test prints the ratio it measured before it asserts."""

import ctypes as C
import inspect
import subprocess
import types

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import hostsim_build
import np_policy_training as T
import np_safe_policy_training as S
from oracle import np_functions as onp

EXTENDED = np.finfo(np.longdouble).eps < 1e-18


def _setup(key):
    system, n_gp, v_kind, lv_kind = key
    case = S._case(system, n_gp)
    return case, S._oracle_dynamics(case), S.safe_spec(case, v_kind, lv_kind)


# ---- 1. the reference against central differences of the oracle's own penalised future_values --------------------
def _oracle_lyapunov(case, safe, orl):
    import oracle
    kind = safe["lv"][0]
    if kind == "const":
        lv = safe["lv"][1]
    elif kind == "abs_linear":
        lv = oracle.AbsFunction(oracle.LinearSystem((safe["lv"][1],)))
    elif kind == "norm_linear":
        lv = oracle.Norm1Function(oracle.LinearSystem((safe["lv"][1],)))
    elif kind == "abs_grad":
        lv = oracle.AbsFunction(safe["V"].gradient)
    else:
        lv = oracle.Norm1Function(safe["V"].gradient)
    grid = oracle.GridWorld(case["limits"], 5)
    return oracle.Lyapunov(grid, safe["V"], orl.dynamics, safe["lf"], lv, safe["tau"], orl.policy)


@pytest.mark.parametrize("combo", [("quadratic", "abs_linear"), ("quadratic", "norm_linear"), ("table", "abs_grad"),
                                   ("table", "const")], ids="-".join)
@pytest.mark.parametrize("name", ["pendulum", "cartpole"])
def test_reference_matches_finite_differences_of_the_oracle(name, combo):
    orl, _ = T.system_pair(name)
    case = S._case(name)
    safe = S.safe_spec(case, *combo)
    olyap = _oracle_lyapunov(case, safe, orl)
    states, actions = T.system_states(name, 200)
    lam, h = 3.0, 1e-6
    # points whose derivative does not jump within the step
    ok = T.comparable(orl, states, actions, margin=1e-4) & S.comparable(orl.dynamics, safe, states, actions, margin=1e-4)
    for shift in (-h, h):
        ok &= T.comparable(orl, states, actions + shift, margin=1e-4)
        ok &= S.comparable(orl.dynamics, safe, states, actions + shift, margin=1e-4)
    assert ok.mean() > 0.5
    ref = S.safe_action_gradient(orl, safe, states, actions, lam)
    value = orl.future_values(states, actions=actions, lyapunov=olyap, lagrange_multiplier=lam)[:, 0]
    assert_allclose(ref["q"], value, rtol=1e-9, atol=1e-12)
    up = orl.future_values(states, actions=actions + h, lyapunov=olyap, lagrange_multiplier=lam)[:, 0]
    down = orl.future_values(states, actions=actions - h, lyapunov=olyap, lagrange_multiplier=lam)[:, 0]
    fd = (up - down) / (2 * h)
    worst = np.abs(fd - ref["grad"][:, 0])[ok].max()
    print("%s, %s: central difference vs reference, largest difference %.3g (gradients up to %.3g)"
          % (name, "-".join(combo), worst, np.abs(ref["grad"]).max()))
    # truncation h^2 f''' / 6 and rounding eps |f| / h of the difference quotient
    assert_allclose(fd[ok], ref["grad"][ok, 0], rtol=1e-5, atol=2e-8 * max(1.0, np.abs(value).max()))


# ---- 2. the reference against torch autograd through solve_triangular ------------------------------
def _torch_diag(kern, Z):
    import torch
    if isinstance(kern, onp.Prod):
        out = _torch_diag(kern.kern_list[0], Z)
        for member in kern.kern_list[1:]:
            out = out * _torch_diag(member, Z)
        return out
    if isinstance(kern, onp.Add):
        return sum(_torch_diag(member, Z) for member in kern.kern_list)
    if isinstance(kern, onp.Linear):
        active = [int(v) for v in kern.active_dims]
        return (Z[:, active] ** 2 * torch.from_numpy(np.broadcast_to(kern.variance, (len(active),)).copy())).sum(dim=1)
    return torch.full((len(Z),), float(kern.variance), dtype=torch.float64)


def _torch_constraint(dynamics, safe, x, u):
    import torch
    import test_policy_training_host as H
    z = torch.cat((x, u), dim=1)
    d = x.shape[1]
    means, errors = [], []
    for gp, _ in S._members(dynamics):
        prior = torch.from_numpy(np.asarray(gp.mean_function.matrix, dtype=np.float64))
        mean = z @ prior.T
        var = _torch_diag(gp.kern, z)
        if len(gp.X):
            chol = torch.from_numpy(gp.cholesky)
            K = H._torch_kernel(gp.kern, torch.from_numpy(gp.X), z)
            a = torch.linalg.solve_triangular(chol, K, upper=False)
            alpha = torch.linalg.solve_triangular(chol.T, torch.from_numpy(gp.alpha), upper=True)
            mean = mean + K.T @ alpha
            var = var - (a * a).sum(dim=0)
        means.append(mean)
        errors.append((safe["beta"] * torch.sqrt(var))[:, None].expand(-1, mean.shape[1]))
    mean, err = torch.cat(means, dim=1), torch.cat(errors, dim=1)
    assert mean.shape[1] == d

    def value(points):
        if isinstance(safe["V"], onp.QuadraticFunction):
            P = torch.from_numpy(np.asarray(safe["V"].matrix, dtype=np.float64))
            return ((points @ P) * points).sum(dim=1)
        return H._torch_table(safe["V"], points, torch.from_numpy(safe["V"].parameters))[:, 0]

    def lipschitz(points):
        kind = safe["lv"][0]
        if kind == "const":
            return torch.full((len(points), 1), float(safe["lv"][1]), dtype=torch.float64)
        if kind in ("abs_linear", "norm_linear"):
            t = torch.abs(points @ torch.from_numpy(np.asarray(safe["lv"][1], dtype=np.float64)).T)
            return t if kind == "abs_linear" else t.sum(dim=1, keepdim=True)
        # the simplex gradient is piecewise constant: a constant of the graph
        c = torch.from_numpy(np.abs(S._simplex_gradient(safe["V"], points.detach().numpy(), np.float64)[0]))
        return c if kind == "abs_grad" else c.sum(dim=1, keepdim=True)

    decrease = value(mean) - value(x) + (lipschitz(mean) * err).sum(dim=1)
    threshold = -lipschitz(x).abs().sum(dim=1) * (1 + float(safe["lf"])) * float(safe["tau"])
    return decrease - threshold


AUTOGRAD_KEYS = ([("rbf", 65, v, lv) for v in S.V_KINDS for lv in S.LV_KINDS if not (v == "quadratic" and "grad" in lv)]
                 + [("pendulum", None, "quadratic", "abs_linear"), ("pendulum", None, "table", "abs_grad"),
                    ("pendulum", None, "table", "norm_linear"), ("ragged", None, "quadratic", "abs_linear"),
                    ("two", None, "quadratic", "abs_linear")])


@pytest.mark.parametrize("key", AUTOGRAD_KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_reference_matches_autograd(key):
    import torch
    case, dynamics, safe = _setup(key)
    states, actions = S.states_of(key[0], 1000)
    ok = S.comparable(dynamics, safe, states, actions)
    assert 1 - ok.mean() <= S.MAX_EXCLUDED
    ref = S.constraint_terms(dynamics, safe, states, actions)
    u = torch.from_numpy(np.ascontiguousarray(actions)).requires_grad_(True)
    c = _torch_constraint(dynamics, safe, torch.from_numpy(states), u)
    c.sum().backward()
    ratio = T.ratio_to_companion(u.grad.numpy(), ref["grad"], ref["A"], ok)
    ratio_c = T.ratio_to_companion(c.detach().numpy(), ref["c"], ref["A_c"], ok)
    r_grad, r_c = S.reference_ratio(key)
    print("%s: autograd vs reference dC/du %.3f, C %.3f x 2^-53 of A (reference vs long double: %.3f, %.3f), %.4f left out"
          % (key, ratio, ratio_c, r_grad, r_c, 1 - ok.mean()))
    tol_grad, tol_c = S.tolerance(key)
    assert ratio * S.UNIT <= tol_grad and ratio_c * S.UNIT <= tol_c
    assert (ref["A"][ok] > 0).all() and (ref["A_c"][ok] > 0).all()


def test_recorded_reference_ratios():
    """Every recorded figure is re-measured: it bounds the measurement and is not slack by more than 4."""
    for key in sorted(S.REFERENCE_RATIO, key=str):
        measured = S.measure_reference_ratio(key)
        print("%s: float64 vs long double dC/du %.3f, C %.3f x 2^-53 of A (recorded %.3g, %.3g)"
              % ((key,) + measured + S.REFERENCE_RATIO[key]))
        if EXTENDED:
            for got, recorded in zip(measured, S.REFERENCE_RATIO[key]):
                assert 0.25 * recorded <= got <= recorded, key
    assert set(S.GPU_KEYS) <= set(S.REFERENCE_RATIO) and set(AUTOGRAD_KEYS) <= set(S.REFERENCE_RATIO)


# ---- 3. the per-point arithmetic, compiled for the host ------------------------------
class _Head(C.Structure):
    """SlPgHead of safe_learning_amd/csrc/sl_policy_grad.h."""
    _fields_ = [("n", C.c_int), ("n_pad", C.c_int), ("dout", C.c_int), ("col0", C.c_int), ("variance", C.c_double),
                ("inv_ls", C.c_void_p), ("xs", C.c_void_p), ("alpha", C.c_void_p), ("kernel", C.c_void_p)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("safe_grad")
    exe = hostsim_build.program("safe_grad.cpp", out, hostsim_build.SHIM_FLAGS)
    assert subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.strip() == "safe_grad: ok"
    return hostsim_build.shared("safe_grad.cpp", out, hostsim_build.SHIM_FLAGS)


def test_header_under_sanitizers(tmp_path_factory):
    """The stand-alone program of tests/hostsim/safe_grad.cpp under AddressSanitizer and UBSan, on its own."""
    exe = hostsim_build.program("safe_grad.cpp", tmp_path_factory.mktemp("safe_grad_san"),
                                hostsim_build.SHIM_FLAGS + ["-g"], sanitize=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "safe_grad: ok", run.stdout


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _shim_decrease_gradient(shim, key, states, actions):
    """The header on the product's own description of the configuration (no engine involved)."""
    import safe_learning_amd as sl
    from safe_learning_amd import _hip
    from safe_learning_amd._model import ModelBuilder
    from safe_learning_amd.functions import _gp_heads, _is_plain_rbf
    case, _, safe = _setup(key)
    dynamics = S.product_dynamics(sl, case)
    d, m = states.shape[1], actions.shape[1]
    p = d + m
    desc = _hip.ModelDesc()
    desc.grid.d, desc.policy.m = d, m
    desc.dynamics.kind = _hip.DYN_GP
    keep, tri_args, table = [], [None, 0, None, None, None, 0], None
    if safe["v_kind"] == "quadratic":
        sl.QuadraticFunction(case["P"])._write_value(desc.value)
    else:
        _, values = S._value_table(case, -1.0 if safe["v_kind"] == "negtable" else +1.0)
        grid = sl.GridWorld(case["limits"], S.TABLE_POINTS)
        tri = sl.Triangulation(grid, values, project=True)
        desc.value.kind, desc.value.negate = _hip.V_TRI, int(safe["v_kind"] == "negtable")
        keep = [grid._desc(), np.ascontiguousarray(tri.unit_simplex_codes, dtype=np.int32),
                np.ascontiguousarray(tri.hyperplanes), np.ascontiguousarray(np.concatenate(grid.discrete_points))]
        tri_args = [C.byref(keep[0]), len(keep[1]), _p(keep[1]), _p(keep[2]), _p(keep[3]), 1]
        table = np.ascontiguousarray(tri.parameters)
    kind = safe["lv"][0]
    if kind == "const":
        lv = safe["lv"][1]
    elif kind in ("abs_linear", "norm_linear"):
        lv = (sl.AbsFunction if kind == "abs_linear" else sl.Norm1Function)(sl.LinearSystem((safe["lv"][1],)))
    else:
        lv = (sl.AbsFunction if kind == "abs_grad" else sl.Norm1Function)(sl.Gradient(None))
    ModelBuilder(None, sl.GridWorld(case["limits"], 5))._write_lipschitz(desc.lipschitz, lv, safe["lf"], safe["tau"])
    gps, beta = _gp_heads(dynamics)
    heads = (_Head * 6)()
    linvs = (C.c_void_p * 6)()
    for h, (gp, _, col0) in enumerate(gps):
        mat = gp.mean_function.matrix
        for r in range(mat.shape[0]):
            for j in range(p):
                desc.dynamics.matrix[col0 + r][j] = float(mat[r, j])
        n = len(gp.X)
        head = heads[h]
        head.n = head.n_pad = n
        head.dout, head.col0 = gp.Y.shape[1], col0
        if n:
            linv = np.ascontiguousarray(gp.cholesky_inverse)
            alpha = np.ascontiguousarray(linv.T.dot(gp.alpha))                         # alpha' = Linv^T alpha
        else:
            linv, alpha = np.zeros((1, 1)), np.zeros((1, head.dout))
        if _is_plain_rbf(gp.kern, p):
            ls = np.broadcast_to(np.asarray(gp.kern.lengthscales, dtype=np.float64), (p,))
            inv_ls, xs = np.ascontiguousarray(1.0 / ls), np.ascontiguousarray((gp.X / ls).T)
            head.variance, kernel = float(gp.kern.variance), None
        else:
            inv_ls, xs = np.ones(p), np.ascontiguousarray(gp.X.T)
            kernel = _hip.GpKernel()
            factors = gp.kern._factors(p)
            kernel.nfactors = len(factors)
            for f, (fkind, product, variance, inv) in enumerate(factors):
                kernel.factor[f].kind, kernel.factor[f].product = int(fkind), int(product)
                for q in range(p):
                    kernel.factor[f].variance[q] = float(variance[q])
                    kernel.factor[f].inv_lengthscales[q] = float(inv[q])
            head.kernel = C.cast(C.pointer(kernel), C.c_void_p)
        if not n:
            xs = np.zeros((p, 1))
        head.inv_ls, head.xs, head.alpha = _p(inv_ls).value, _p(xs).value, _p(alpha).value
        linvs[h] = _p(linv).value
        keep += [alpha, inv_ls, xs, kernel, linv]
    n = len(states)
    states, actions = np.ascontiguousarray(states), np.ascontiguousarray(actions)
    grad, constraint, terms = np.zeros((n, m)), np.zeros(n), np.zeros((n, 2 + 2 * d))
    rc = shim.sg_decrease_gradient(*tri_args, None if table is None else _p(table), C.byref(desc), C.c_double(beta),
                                   len(gps), heads, linvs, d, m, C.c_int64(n), _p(states), _p(actions), _p(grad),
                                   _p(constraint), _p(terms))
    assert rc == 0
    return grad, constraint, terms


HEADER_KEYS = [("pendulum", None, "quadratic", "abs_linear"), ("cartpole", None, "quadratic", "abs_linear"),
               ("two", None, "quadratic", "abs_linear"), ("ragged", None, "quadratic", "abs_linear"),
               ("rbf", 0, "quadratic", "abs_linear"), ("rbf", 65, "quadratic", "const"),
               ("rbf", 65, "quadratic", "norm_linear"), ("rbf", 65, "table", "abs_grad"),
               ("rbf", 65, "negtable", "norm_grad"), ("rbf", 65, "table", "abs_linear"),
               ("rbf", 65, "negtable", "norm_linear")]


@pytest.mark.parametrize("key", HEADER_KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_header_matches_reference(shim, key):
    case, dynamics, safe = _setup(key)
    states, actions = S.states_of(key[0], 1000)
    ok = S.comparable(dynamics, safe, states, actions)
    assert 1 - ok.mean() <= S.MAX_EXCLUDED
    ref = S.constraint_terms(dynamics, safe, states, actions)
    grad, constraint, terms = _shim_decrease_gradient(shim, key, states, actions)
    ratio = T.ratio_to_companion(grad, ref["grad"], ref["A"], ok)
    ratio_c = T.ratio_to_companion(constraint, ref["c"], ref["A_c"], ok)
    r_grad, r_c = S.reference_ratio(key)
    print("%s: header vs reference dC/du %.3f (tolerance %.1f), C %.3f (tolerance %.1f) x 2^-53 of A"
          % (key, ratio, 32 * r_grad, ratio_c, 32 * r_c))
    tol_grad, tol_c = S.tolerance(key)
    assert ratio * S.UNIT <= tol_grad and ratio_c * S.UNIT <= tol_c
    assert_array_equal(constraint, terms[:, 0] - terms[:, 1])
    assert_allclose(terms[ok, 2:2 + states.shape[1]], ref["mean"][ok], rtol=1e-11, atol=1e-13)
    assert_allclose(terms[ok, 2 + states.shape[1]:], ref["error"][ok], rtol=1e-7, atol=0)


def test_header_kernel_diagonal(shim):
    """k(z, z) and its action derivative of the notebook's Linear + Matern32 x Linear heads."""
    import safe_learning_amd as sl
    from safe_learning_amd import _hip
    from safe_learning_amd.functions import _gp_heads
    case = S._case("pendulum")
    dynamics = S._oracle_dynamics(case)
    states, actions = S.states_of("pendulum", 100)
    z = np.ascontiguousarray(np.hstack((states, actions)))
    for (gp, _, _), (ogp, _) in zip(_gp_heads(S.product_dynamics(sl, case))[0], S._members(dynamics)):
        kernel = _hip.GpKernel()
        factors = gp.kern._factors(3)
        kernel.nfactors = len(factors)
        for f, (kind, product, variance, inv) in enumerate(factors):
            kernel.factor[f].kind, kernel.factor[f].product = int(kind), int(product)
            for q in range(3):
                kernel.factor[f].variance[q] = float(variance[q])
                kernel.factor[f].inv_lengthscales[q] = float(inv[q])
        kzz, dkzz = np.zeros(len(z)), np.zeros((len(z), 1))
        assert shim.sg_kernel_diag(C.byref(kernel), 3, 2, 1, _p(z), len(z), _p(kzz), _p(dkzz)) == 0
        want, dwant, _, _ = S.diag_terms(ogp.kern, z, [2])
        assert_allclose(kzz, want, rtol=1e-14)
        assert_allclose(kzz, ogp.kern.Kdiag(z), rtol=1e-14)
        assert_allclose(dkzz, dwant, rtol=1e-14, atol=1e-300)
        assert (dwant != 0).any()


# ---- 4. the Python layer on a stand-in engine ------------------------------
def _stand_in(monkeypatch):
    """A PolicyIteration and a Lyapunov whose engine calls are answered by fixed CPU tensors."""
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate, lyapunov as L, reinforcement_learning as R
    case = S._case("rbf", 5)
    dynamics = S.product_dynamics(sl, case)
    _, policy = T.make_network("notebook", sl)
    rng = np.random.default_rng(0)
    n = 7
    fixed = {k: torch.from_numpy(rng.normal(size=shape)) for k, shape in
             (("grad", (n, 1)), ("q", (n,)), ("dc", (n, 1)), ("c", (n, 1)), ("u", (n, 1)))}
    calls = []
    rl = R.PolicyIteration.__new__(R.PolicyIteration)
    rl.dynamics, rl.policy, rl._world = dynamics, policy, 1
    rl._ctx = types.SimpleNamespace(torch_device=torch.device("cpu"))
    rl.discretization = types.SimpleNamespace(all_points=np.zeros((3, 2)), ndim=2)

    def action_gradient_device(states, policy_arg, actions):
        calls.append(("action_gradient", actions))
        return _evaluate._to_device(rl._ctx, states), fixed["grad"], fixed["q"]

    rl._action_gradient_device = action_gradient_device
    lyap = L.Lyapunov.__new__(L.Lyapunov)
    lyap.dynamics = dynamics

    def decrease_gradient(states, actions=None):
        calls.append(("decrease_gradient", actions))
        return fixed["dc"], fixed["c"]

    lyap.decrease_gradient = decrease_gradient
    monkeypatch.setattr(_evaluate, "policy", lambda spec, points: fixed["u"])
    policy.parameter_gradient = lambda states, coeff: coeff.clone()
    return rl, lyap, fixed, calls, rng.normal(size=(n, 2))


def test_python_layer_on_a_stand_in_engine(monkeypatch):
    import safe_learning_amd as sl
    from safe_learning_amd import lyapunov as L, training
    rl, lyap, fixed, calls, states = _stand_in(monkeypatch)
    # anything that is not a Lyapunov keeps raising what it raised before
    with pytest.raises(NotImplementedError, match="Lyapunov penalty"):
        rl.action_gradient(states, lyapunov=object())
    with pytest.raises(NotImplementedError, match="Lyapunov penalty"):
        rl.policy_gradient(states, lyapunov=object())
    # another dynamics object; deterministic dynamics
    other = L.Lyapunov.__new__(L.Lyapunov)
    other.dynamics = S.product_dynamics(sl, S._case("rbf", 5))
    with pytest.raises(ValueError, match="lyapunov.dynamics must be the dynamics object"):
        rl.policy_gradient(states, lyapunov=other)
    linear = sl.LinearSystem((np.eye(2), np.ones((2, 1))))
    other.dynamics, rl.dynamics = linear, linear
    with pytest.raises(TypeError, match="uncertain dynamics"):
        rl.action_gradient(states, lyapunov=other)
    rl.dynamics = lyap.dynamics
    assert not calls
    # lambda = 0: the unpenalised numbers bit for bit; the actions are evaluated once and shared
    objective0, gradient0 = rl.policy_gradient(states)
    del calls[:]
    objective, gradient = rl.policy_gradient(states, lyapunov=lyap, lagrange_multiplier=0)
    assert objective == objective0
    assert_array_equal(gradient.numpy(), gradient0.numpy())
    assert [name for name, _ in calls] == ["action_gradient", "decrease_gradient"]
    assert calls[0][1] is calls[1][1] and calls[0][1].data_ptr() == fixed["u"].data_ptr()
    # lambda = 2.5, 'sum' and 'mean'
    n = len(states)
    objective, gradient = rl.policy_gradient(states, 'sum', lyapunov=lyap, lagrange_multiplier=2.5)
    assert_array_equal(gradient.numpy(), (fixed["grad"] - 2.5 * fixed["dc"]).numpy())
    assert objective == float((fixed["q"] - 2.5 * fixed["c"][:, 0]).sum())
    objective, gradient = rl.policy_gradient(states, lyapunov=lyap)
    assert_array_equal(gradient.numpy(), ((fixed["grad"] - 1.0 * fixed["dc"]) * (1.0 / n)).numpy())
    got = rl.action_gradient(states, lyapunov=lyap, lagrange_multiplier=2.5)
    assert isinstance(got, np.ndarray)
    assert_array_equal(got, (fixed["grad"] - 2.5 * fixed["dc"]).numpy())
    # explicit actions go to both calls as they are
    del calls[:]
    rl.action_gradient(states, actions=np.full((n, 1), 0.25), lyapunov=lyap)
    assert calls[0][1] is calls[1][1] and (calls[0][1].numpy() == 0.25).all()
    # the step
    params = inspect.signature(training.policy_improvement_step).parameters
    assert list(params)[-2:] == ["lyapunov", "lagrange_multiplier"] and params["lagrange_multiplier"].default == 1.
    assert list(inspect.signature(sl.PolicyIteration.policy_gradient).parameters)[1:] == [
        "states", "reduction", "lyapunov", "lagrange_multiplier"]
    assert list(inspect.signature(sl.PolicyIteration.action_gradient).parameters)[1:] == [
        "states", "policy", "actions", "lyapunov", "lagrange_multiplier"]
    assert hasattr(sl.Lyapunov, "decrease_gradient")
