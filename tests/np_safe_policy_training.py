"""NumPy reference of the Lyapunov penalty of ``PolicyIteration.future_values`` and of its action derivative
(``Lyapunov.decrease_gradient``, ``PolicyIteration.action_gradient / policy_gradient(..., lyapunov=)``,
``training.policy_improvement_step(..., lyapunov=)``), built on tests/np_policy_training.py (``kernel_terms``,
``table_gradient``, the parameter gradients) and tests/np_gp_truth.py (the long-double Cholesky).

    C(x, u)  = V_L(mu) - V_L(x) + sum_k L_k(mu) e_k + |L(x)|_1 (1 + L_f(x)) tau        reinforcement_learning.py:107-112
    e_k      = beta sqrt(var_h),  var_h = k(z, z) - |a|^2,  a = L^-1 k_x              functions.py:438-456, 507-515
    dC/du_a  = sum_j [g_j(mu) + sum_k dL_k/dmu_j e_k] J_ja + sum_k L_k(mu) beta dvar_h/du_a / (2 sqrt(var_h))
    dvar_h/du_a = dk(z, z)/du_a - 2 a^T b_a,  b_a = L^-1 dk_x/du_a

The float64 run takes the engine's route - an explicit ``L^-1`` multiply and ``alpha' = L^-T alpha``, as
``np_gp_truth.explicit_inverse_posterior`` does; the ``np.longdouble`` run does its own long-double Cholesky
and forward / backward substitution.  Every output comes with an error companion ``A`` (every term replaced by
its absolute value, plus the propagation of the inputs' companions: ``|Kdiag| + sum a^2`` for the variance,
``|dKdiag| + 2 sum |a| |b_a|`` for its derivative, ``beta |dvar| A_var / (4 var^(3/2))`` through ``1 / sqrt(var)``).
Results are compared as ``|got - ref| <= 32 r 2^-53 A`` with ``r`` the float64 reference's own measured error
against its long-double run in units of ``2^-53 A``, the maximum over ``RATIO_POINTS`` states per configuration:
the rule and margin of ``np_policy_training.tolerance``, never derived from the engine's output.
"""

import types

import numpy as np
import scipy.linalg

import np_gp_truth as G
import np_policy_training as T
from oracle import np_functions as onp
import training_tolerance
from training_tolerance import LONG, UNIT, recorded_or_measured

ABS_MARGIN = 1e-9
MAX_EXCLUDED = T.MAX_EXCLUDED
RATIO_POINTS = 1000


# ---- k(z, z) and its action derivative ------------------------------
def diag_terms(kern, Z, cols, dtype=np.float64):
    """-> (kzz [q], dkzz [q, m], companions): ``kern.Kdiag`` and its total derivative with respect to the
    columns ``cols`` of the points (0 for a stationary kernel, ``2 variance_q z_q`` for a Linear one)."""
    Z = np.asarray(Z, dtype=dtype)
    q, m = len(Z), len(cols)
    if isinstance(kern, onp.Prod):
        K, dK = np.ones(q, dtype=dtype), np.zeros((q, m), dtype=dtype)
        KA, dKA = np.ones(q, dtype=dtype), np.zeros((q, m), dtype=dtype)
        for member in kern.kern_list:
            k, dk, ka, dka = diag_terms(member, Z, cols, dtype)
            dK, dKA = dK * k[:, None] + K[:, None] * dk, dKA * ka[:, None] + KA[:, None] * dka
            K, KA = K * k, KA * ka
        return K, dK, KA, dKA
    if isinstance(kern, onp.Add):
        parts = [diag_terms(member, Z, cols, dtype) for member in kern.kern_list]
        return tuple(sum(p[i] for p in parts) for i in range(4))
    dK = np.zeros((q, m), dtype=dtype)
    if isinstance(kern, onp.Linear):
        active = list(kern.active_dims)
        var = np.broadcast_to(np.asarray(kern.variance, dtype=dtype), (len(active),))
        Za = Z[:, active]
        K = np.sum(Za * Za * var, axis=1)
        for a, c in enumerate(cols):
            if c in active:
                pos = active.index(c)
                dK[:, a] = 2 * var[pos] * Za[:, pos]
        return K, dK, K.copy(), np.abs(dK)
    K = np.full(q, dtype(kern.variance), dtype=dtype)
    return K, dK, np.abs(K), np.abs(dK)


# ---- linear algebra of the two runs ------------------------------
_FACTORS = {}


def _long_double_factor(gp):
    """(L, alpha' = L^-T L^-1 (Y - m(X))) of one head in long double, kept per data version."""
    key = (id(gp), len(gp.X))
    if key not in _FACTORS:
        X = G.ld(gp.X)
        gram = T.kernel_terms(gp.kern, gp.X, gp.X, [], LONG)[0] + LONG(gp.likelihood_variance) * np.eye(len(X), dtype=LONG)
        chol = G.cholesky(gram)
        alpha = G.forward_substitution(chol, G.ld(gp.Y) - X.dot(G.ld(gp.mean_function.matrix).T))
        out = np.array(alpha, copy=True)
        for i in reversed(range(len(chol))):                                  # L^T x = alpha
            if i + 1 < len(chol):
                out[i] -= chol[i + 1:, i].dot(out[i + 1:])
            out[i] /= chol[i, i]
        _FACTORS[key] = (gp, chol, out)
    return _FACTORS[key][1:]


def posterior_terms(dynamics, z, d, dtype=np.float64):
    """Mean, action Jacobian, variance and its action derivative of an oracle GaussianProcess / FunctionStack at
    ``z = [x, u]``, each with its companion -> dict(mean, A_mean, J, JA [n, d, m], var, A_var [n, d], dvar,
    A_dvar [n, d, m]).  A head without observations contributes its prior alone."""
    z = np.asarray(z, dtype=dtype)
    n, p = z.shape
    m = p - d
    cols = list(range(d, p))
    out = {k: np.zeros((n, d), dtype=dtype) for k in ("mean", "A_mean", "var", "A_var")}
    out.update({k: np.zeros((n, d, m), dtype=dtype) for k in ("J", "JA", "dvar", "A_dvar")})
    for gp, col0 in _members(dynamics):
        assert gp._scale == 1.0
        sl = slice(col0, col0 + gp.Y.shape[1])
        prior = np.asarray(gp.mean_function.matrix, dtype=dtype)
        kzz, dkzz, kzzA, dkzzA = diag_terms(gp.kern, z, cols, dtype)
        out["mean"][:, sl] = z.dot(prior.T)
        out["A_mean"][:, sl] = np.abs(z).dot(np.abs(prior).T)
        out["J"][:, sl, :] = prior[None, :, d:]
        out["JA"][:, sl, :] = np.abs(prior)[None, :, d:]
        ss, sab, sabA = np.zeros(n, dtype=dtype), np.zeros((n, m), dtype=dtype), np.zeros((n, m), dtype=dtype)
        if len(gp.X):
            K, dK, KA, dKA = T.kernel_terms(gp.kern, gp.X, z, cols, dtype)
            if dtype is LONG:
                chol, alpha = _long_double_factor(gp)
                a = G.forward_substitution(chol, K)
                b = G.forward_substitution(chol, dK.reshape(len(gp.X), -1)).reshape(dK.shape)
            else:
                inverse = np.tril(scipy.linalg.solve_triangular(gp.cholesky, np.eye(len(gp.X)), lower=True))
                alpha = inverse.T.dot(gp.alpha)
                a = inverse.dot(K)
                b = np.einsum("ij,jna->ina", inverse, dK)
            out["mean"][:, sl] += K.T.dot(alpha)
            out["A_mean"][:, sl] += KA.T.dot(np.abs(alpha))
            out["J"][:, sl, :] += np.einsum("jia,jk->ika", dK, alpha)
            out["JA"][:, sl, :] += np.einsum("jia,jk->ika", dKA, np.abs(alpha))
            ss = np.sum(a * a, axis=0)
            sab = np.einsum("in,ina->na", a, b)
            sabA = np.einsum("in,ina->na", np.abs(a), np.abs(b))
        out["var"][:, sl] = (kzz - ss)[:, None]
        out["A_var"][:, sl] = (kzzA + ss)[:, None]
        out["dvar"][:, sl, :] = (dkzz - 2 * sab)[:, None, :]
        out["A_dvar"][:, sl, :] = (dkzzA + 2 * sabA)[:, None, :]
    return out


# ---- V_L and L_v ------------------------------
def _simplex_gradient(tri, points, dtype):
    """``tri.gradient`` in ``dtype`` without the mask of ``project`` (what L_v = |gradient| reads)."""
    pts64 = np.asarray(points, dtype=np.float64)
    ids = tri.find_simplex(pts64)
    simplices = tri.simplices(ids)
    H = tri.hyperplanes[ids % tri.triangulation.nsimplex].astype(dtype)
    params = np.asarray(tri.parameters, dtype=dtype)[:, 0][simplices]
    c = np.einsum("nkj,nj->nk", H, params[:, 1:] - params[:, :1])
    cA = np.einsum("nkj,nj->nk", np.abs(H), np.abs(params[:, 1:]) + np.abs(params[:, :1]))
    return c, cA


def value_terms(V, pts, A_pts, dtype):
    """-> (v [n], A_v, g [n, d], A_g): ``V`` an oracle QuadraticFunction or Triangulation."""
    pts = np.asarray(pts, dtype=dtype)
    if isinstance(V, onp.QuadraticFunction):
        P = np.asarray(V.matrix, dtype=dtype)
        S = P + P.T
        g = pts.dot(S)
        A_g = np.abs(pts).dot(np.abs(S)) + A_pts.dot(np.abs(S))
        v = np.einsum("ni,ij,nj->n", pts, P, pts)
        A_v = np.einsum("ni,ij,nj->n", np.abs(pts), np.abs(P), np.abs(pts)) + np.sum(np.abs(g) * A_pts, axis=1)
        return v, A_v, g, A_g
    w, simplices, wA = T.table_weights(V, pts, dtype)
    params = np.asarray(V.parameters, dtype=dtype)[:, 0][simplices]
    g, A_g = T.table_gradient(V, pts, dtype)
    v = np.sum(w * params, axis=1)
    A_v = np.sum(wA * np.abs(params), axis=1) + np.sum(np.abs(g) * A_pts, axis=1)
    return v, A_v, g, A_g


def lv_terms(lv, V, pts, A_pts, dtype):
    """-> (L [n, cols], A_L, dL [n, cols, d] = dL/dpts, A_dL, pre [n, k]: the terms under the abs)."""
    pts = np.asarray(pts, dtype=dtype)
    n, d = pts.shape
    kind, arg = (tuple(lv) + (None,))[:2]
    if kind == "const":
        zero = np.zeros((n, 1, d), dtype=dtype)
        return np.full((n, 1), dtype(arg), dtype=dtype), np.zeros((n, 1), dtype=dtype), zero, zero, np.ones((n, 1))
    if kind in ("abs_linear", "norm_linear"):
        Gm = np.asarray(arg, dtype=dtype)
        t = pts.dot(Gm.T)
        tA = np.abs(pts).dot(np.abs(Gm).T) + A_pts.dot(np.abs(Gm).T)
        dL = np.sign(t)[:, :, None] * Gm[None, :, :]                    # (sign and G are exact: no companion)
        if kind == "abs_linear":
            return np.abs(t), tA, dL, np.zeros_like(dL), t
        dL = np.sum(dL, axis=1, keepdims=True)
        return np.sum(np.abs(t), axis=1, keepdims=True), np.sum(tA, axis=1, keepdims=True), dL, np.zeros_like(dL), t
    c, cA = _simplex_gradient(V, pts, dtype)
    if kind == "abs_grad":
        zero = np.zeros((n, d, d), dtype=dtype)
        return np.abs(c), cA, zero, zero, c
    zero = np.zeros((n, 1, d), dtype=dtype)
    return np.sum(np.abs(c), axis=1, keepdims=True), np.sum(cA, axis=1, keepdims=True), zero, zero, c


def lf_values(lf, x, dtype):
    if np.isscalar(lf):
        return dtype(lf)
    c, M = lf
    return dtype(c) + np.sum(np.abs(np.asarray(x, dtype=dtype).dot(np.asarray(M, dtype=dtype).T)), axis=1)


# ---- the constraint and its action derivative ------------------------------
def constraint_terms(dynamics, safe, states, actions, dtype=np.float64):
    """``safe``: dict(V, lv=(kind, arg), lf, tau, beta) of oracle objects and numbers.  -> dict(grad [n, m], A,
    c [n], A_c, decrease, threshold, mean, error, var, pre)."""
    x = np.atleast_2d(np.asarray(states, dtype=dtype))
    u = np.atleast_2d(np.asarray(actions, dtype=dtype))
    n, d = x.shape
    post = posterior_terms(dynamics, np.hstack((x, u)), d, dtype)
    beta = dtype(safe["beta"])
    var = post["var"]
    s = np.sqrt(var)
    e = beta * s
    A_e = beta * post["A_var"] / (2 * s)
    de = beta * post["dvar"] / (2 * s)[:, :, None]
    A_de = (beta * post["A_dvar"] / (2 * s)[:, :, None]
            + beta * np.abs(post["dvar"]) * (post["A_var"] / (4 * var * s))[:, :, None])
    mean, A_mean = post["mean"], post["A_mean"]
    v_n, A_vn, g, A_g = value_terms(safe["V"], mean, A_mean, dtype)
    v_x, A_vx, _, _ = value_terms(safe["V"], x, np.zeros_like(x), dtype)
    L, A_L, dL, A_dL, pre = lv_terms(safe["lv"], safe["V"], mean, A_mean, dtype)
    L_x, _, _, _, _ = lv_terms(safe["lv"], safe["V"], x, np.zeros_like(x), dtype)
    if L.shape[1] == 1:                                                  # one column multiplies every error
        L, A_L = np.repeat(L, d, axis=1), np.repeat(A_L, d, axis=1)
        dL, A_dL = np.repeat(dL, d, axis=1), np.repeat(A_dL, d, axis=1)
    decrease = (v_n - v_x) + np.sum(L * e, axis=1)
    threshold = -np.sum(np.abs(L_x), axis=1) * (1 + lf_values(safe["lf"], x, dtype)) * dtype(safe["tau"])
    c = decrease - threshold
    A_c = A_vn + A_vx + np.sum(A_L * e + L * A_e, axis=1) + np.abs(threshold)
    w = np.einsum("nk,nkj->nj", e, dL)
    A_w = np.einsum("nk,nkj->nj", e + A_e, np.abs(dL)) + np.einsum("nk,nkj->nj", e, A_dL)
    coeff, A_coeff = g + w, A_g + A_w
    grad = np.einsum("nj,nja->na", coeff, post["J"]) + np.einsum("nk,nka->na", L, de)
    A = (np.einsum("nj,nja->na", A_coeff, np.abs(post["J"])) + np.einsum("nj,nja->na", np.abs(g) + np.abs(w), post["JA"])
         + np.einsum("nk,nka->na", A_L, np.abs(de)) + np.einsum("nk,nka->na", L, A_de))
    return dict(grad=grad, A=A, c=c, A_c=A_c, decrease=decrease, threshold=threshold, mean=mean, error=e, var=var,
                pre=pre, A_mean=A_mean, A_e=A_e)


def comparable(dynamics, safe, states, actions, margin=ABS_MARGIN):
    """Mask of the points at which the constraint and its derivative do not jump nearby: for a table V_L the
    rule of ``np_policy_training.comparable`` at the successor (and no ambiguous simplex at the state either:
    L_v(x) = |gradient| enters the threshold), every term under an abs further than ``margin`` from 0, every
    variance positive."""
    import exclusions
    terms = constraint_terms(dynamics, safe, states, actions)
    ok = (terms["var"] > 0).all(axis=1) & (np.abs(terms["pre"]) > margin).all(axis=1)
    if isinstance(safe["V"], onp.Triangulation):
        stand_in = types.SimpleNamespace(dynamics=dynamics, value_function=safe["V"], policy=None)
        ok &= T.comparable(stand_in, states, actions, margin)
        ok &= ~exclusions.ambiguous_points(safe["V"], np.asarray(states, dtype=np.float64))
        lim = safe["V"].discretization.limits
        for pts in (np.asarray(states, dtype=np.float64), terms["mean"]):     # (beyond a corner: see states_of)
            ok &= ((pts < lim[:, 0]) | (pts > lim[:, 1])).sum(axis=1) <= 1
    return ok


# ---- the safe objective Q - lambda C ------------------------------
def safe_action_gradient(orl, safe, states, actions, lagrange_multiplier=1.0, dtype=np.float64):
    """-> dict(grad, A, q, A_q) of ``future_values(states, actions=actions, lyapunov=.., lagrange_multiplier=..)``."""
    base = T.action_gradient(orl, states, actions, dtype)
    pen = constraint_terms(orl.dynamics, safe, states, actions, dtype)
    lam = dtype(lagrange_multiplier)
    return dict(grad=base["grad"] - lam * pen["grad"], A=base["A"] + abs(lam) * pen["A"],
                q=base["q"] - lam * pen["c"], A_c=pen["A_c"], c=pen["c"])


def safe_policy_gradient(orl, safe, states, reduction="mean", lagrange_multiplier=1.0, dtype=np.float64):
    """-> (objective, gradient, companion) with respect to ``orl.policy.parameters``."""
    states = orl.state_space if states is None else np.atleast_2d(states)
    u = T.policy_actions(orl.policy, states, dtype)
    terms = safe_action_gradient(orl, safe, states, u, lagrange_multiplier, dtype)
    scale = dtype(1) / len(states) if reduction == "mean" else dtype(1)
    objective = np.sum(terms["q"]) * scale
    if isinstance(orl.policy, onp.NeuralNetwork):
        grad, _ = T.network_parameter_gradient(orl.policy, states, terms["grad"] * scale, dtype)
        _, comp = T.network_parameter_gradient(orl.policy, states, terms["A"] * scale, dtype)
    else:
        grad, _ = T.table_parameter_gradient(orl.policy, states, terms["grad"] * scale, dtype)
        _, comp = T.table_parameter_gradient(orl.policy, states, terms["A"] * scale, dtype)
    return objective, grad, comp


def safe_policy_improvement_step(orl, safe, states, learning_rate, reduction="mean", lagrange_multiplier=1.0):
    objective, grad, comp = safe_policy_gradient(orl, safe, states, reduction, lagrange_multiplier)
    if isinstance(grad, list):
        orl.policy.parameters = [w + learning_rate * g for w, g in zip(orl.policy.parameters, grad)]
    else:
        orl.policy.parameters = orl.policy.parameters + learning_rate * grad
    return float(objective), grad, comp


# ---- the configurations of the tests ------------------------------
V_KINDS = ("quadratic", "table", "negtable")
LV_KINDS = ("const", "abs_linear", "norm_linear", "abs_grad", "norm_grad")
TABLE_POINTS = 9


def _case(system, n_gp=None):
    """``make_case`` dict of a dynamics configuration: 'pendulum' / 'cartpole' of np_policy_training.system_case,
    'rbf' (the pendulum with ONE RBF head of ``n_gp`` points over both outputs), 'two' (2 states, 2 actions, one
    RBF head of 40 points), 'ragged' (the notebook-kernel pendulum stack with 70 and 0 observations)."""
    import cases
    from safe_learning_amd.benchmarks import notebook_kernels
    if system in ("pendulum", "cartpole"):
        return T.system_case(system)["case"]
    if system == "rbf":
        n_gp = 70 if n_gp is None else n_gp
        case = cases.make_case("pendulum", n_gp=max(n_gp, 1), **_RBF_HYPER)
        if n_gp == 0:
            case["empty_heads"] = (0,)
        return case
    if system == "ragged":
        case = cases.make_case("pendulum", n_gp=70, stack=True)
        case["dynamics"]["kernels"] = notebook_kernels(case)
        case["empty_heads"] = (1,)
        return case
    assert system == "two"
    A = np.array([[1.0, 0.1], [-0.05, 0.95]])
    B = np.array([[0.02, 0.1], [0.1, -0.03]])
    rng = np.random.default_rng(11)
    X = rng.uniform(-1, 1, (40, 4))
    Y = X.dot(np.hstack((A, B)).T) + 0.02 * np.sin(2.0 * X[:, :2]) + rng.normal(0, 0.002, (40, 2))
    P = np.array([[1.0, 0.2], [0.2, 0.7]])
    return dict(name="two", stack=False, d=2, m=2, limits=[[-1., 1.]] * 2, num_points=[5, 5], saturate=None,
                K=np.array([[-0.3, 0.1], [0.05, -0.2]]), P=P, lv=("abs_linear", 2 * P), lf=1.3, tau=0.01,
                dynamics={"kind": "gp", "X": X, "Y": Y, "variance": 0.03 ** 2, "lengthscales": np.full(4, 1.5),
                          "noise_variance": 0.002 ** 2, "prior": np.hstack((A * 0.98, B)), "beta": 2.0})


_RBF_HYPER = dict(signal_std=0.03, noise_std=0.0005, lengthscale=1.5)


def _without_observations(gp):
    """What the reference reads of a head that has no observations yet (the notebook's starting state)."""
    return types.SimpleNamespace(X=np.zeros((0, gp.X.shape[1])), Y=np.zeros((0, gp.Y.shape[1])), kern=gp.kern,
                                 mean_function=gp.mean_function, likelihood_variance=gp.likelihood_variance,
                                 _scale=1.0)


def _oracle_dynamics(case):
    """The oracle's model of a case; heads without observations (which the oracle's GPRCached does not
    factorise) as plain records: ``members`` lists (head, first column) for posterior_terms."""
    import cases
    import oracle
    if case["name"] == "two":                                            # (oracle_specs builds d + 1 inputs)
        dyn = case["dynamics"]
        kern = oracle.RBF(case["d"] + case["m"], dyn["variance"], dyn["lengthscales"], ARD=True)
        gp = oracle.GPRCached(dyn["X"], dyn["Y"], kern, oracle.LinearSystem((dyn["prior"],)),
                              likelihood_variance=dyn["noise_variance"])
        return oracle.GaussianProcess(gp, dyn["beta"])
    empty_heads = case.get("empty_heads", ())
    model =cases.oracle_specs(dict(case, K=np.zeros((case["m"], case["d"])), saturate=None))[1]
    if not empty_heads:
        return model
    members = [(_without_observations(gp) if h in empty_heads else gp, col0)
               for h, (gp, col0) in enumerate(T._gp_members(model))]
    return types.SimpleNamespace(members=members)


def _members(dynamics):
    return dynamics.members if hasattr(dynamics, "members") else T._gp_members(dynamics)


def _value_table(case, sign):
    import oracle
    grid = oracle.GridWorld(case["limits"], TABLE_POINTS)
    return grid, T.smooth_table(grid, case["P"], sign=sign)


def safe_spec(case, v_kind="quadratic", lv_kind=None):
    """-> dict(V, lv, lf, tau, beta) of oracle objects for one (V_L, L_v) combination on a case."""
    import oracle
    if v_kind == "quadratic":
        V = oracle.QuadraticFunction(case["P"])
    else:
        # 'negtable': the notebook's lyapunov_function = -rl.value_function; the oracle holds the negated values
        grid, values = _value_table(case, +1.0)
        V = oracle.Triangulation(grid, values, project=True)
    lv_kind = case["lv"][0] if lv_kind is None else lv_kind
    if lv_kind == "const":
        lv = ("const", 0.8)
    elif lv_kind in ("abs_linear", "norm_linear"):
        lv = (lv_kind, 2 * np.asarray(case["P"]) + 0.05 * np.arange(case["d"] ** 2).reshape(case["d"], case["d"]))
    else:
        assert v_kind != "quadratic"
        lv = (lv_kind,)
    return dict(V=V, lv=lv, lf=case["lf"], tau=case["tau"], beta=case["dynamics"]["beta"], v_kind=v_kind)


def product_lyapunov(sl, case, safe, dynamics, policy):
    """The product's ``Lyapunov`` of a spec, on a 5-point grid, sharing ``dynamics`` and ``policy``."""
    grid = sl.GridWorld(case["limits"], 5)
    if safe["v_kind"] == "quadratic":
        V = sl.QuadraticFunction(case["P"])
    else:
        tgrid, values = _value_table(case, -1.0 if safe["v_kind"] == "negtable" else +1.0)
        V = sl.Triangulation(sl.GridWorld(case["limits"], TABLE_POINTS), values, project=True)
        if safe["v_kind"] == "negtable":
            V = -V
    kind = safe["lv"][0]
    if kind == "const":
        lv = safe["lv"][1]
    elif kind == "abs_linear":
        lv = sl.AbsFunction(sl.LinearSystem((safe["lv"][1],)))
    elif kind == "norm_linear":
        lv = sl.Norm1Function(sl.LinearSystem((safe["lv"][1],)))
    elif kind == "abs_grad":
        lv = sl.AbsFunction(sl.Gradient(V))
    else:
        lv = sl.Norm1Function(sl.Gradient(V))
    return sl.Lyapunov(grid, V, dynamics, safe["lf"], lv, safe["tau"], policy)


def product_dynamics(sl, case):
    from safe_learning_amd.benchmarks import build_specs
    from safe_learning_amd import functions as F
    if case["name"] == "two":
        dyn = case["dynamics"]
        kern = F.RBF(case["d"] + case["m"], dyn["variance"], dyn["lengthscales"], ARD=True)
        gp = F.GPRCached(dyn["X"], dyn["Y"], kern, F.LinearSystem((dyn["prior"],)),
                         likelihood_variance=dyn["noise_variance"])
        return F.GaussianProcess(gp, dyn["beta"])
    _, dynamics, _, _ = build_specs(dict(case, K=np.zeros((case["m"], case["d"])), saturate=None))
    if case.get("empty_heads"):
        heads = list(dynamics.functions) if isinstance(dynamics, F.FunctionStack) else [dynamics]
        p = case["d"] + case["m"]
        for h in case["empty_heads"]:
            gp = heads[h].gaussian_process
            empty = F.GPRCached(np.zeros((0, p)), np.zeros((0, gp.Y.shape[1])), gp.kern, gp.mean_function,
                                likelihood_variance=case["dynamics"]["noise_variance"])
            heads[h] = F.GaussianProcess(empty, case["dynamics"]["beta"])
        dynamics = F.FunctionStack(heads) if isinstance(dynamics, F.FunctionStack) else heads[0]
    return dynamics


def states_of(system, n, seed=5):
    """States in [-1.15, 1.15]^d and actions in [-1, 1]^m."""
    case_d = {"pendulum": (2, 1), "cartpole": (4, 1), "rbf": (2, 1), "ragged": (2, 1), "two": (2, 2)}[system]
    rng = np.random.default_rng(seed + n)
    states = rng.uniform(-1.15, 1.15, (n, case_d[0]))
    # outside the unit box in one coordinate at a time: beyond a corner of a table's grid the clipped unit-cell
    # coordinates sit on a shared face and the simplices there extrapolate differently (tests/exclusions.py)
    outside = np.abs(states) > 1
    for k in range(1, case_d[0]):
        redo = outside[:, :k].any(axis=1) & outside[:, k]
        states[redo, k] = rng.uniform(-0.95, 0.95, int(redo.sum()))
        outside[:, k] = np.abs(states[:, k]) > 1
    return states, rng.uniform(-1, 1, (n, case_d[1]))


# ---- the tolerance ------------------------------
# max |float64 - long double| / A of this reference in units of 2^-53 over the RATIO_POINTS states of
# states_of(system, RATIO_POINTS), measured by measure_reference_ratio below and rounded up
# (tests/test_safe_policy_training_host.py re-measures them).  Keys: (system, n_gp or None, V kind, L_v kind) ->
# (figure for dC/du, figure for C).
REFERENCE_RATIO = {
    ('pendulum', None, 'quadratic', 'abs_linear'): (1.76, 0.993),
    ('cartpole', None, 'quadratic', 'abs_linear'): (4.52, 1.5),
    ('two', None, 'quadratic', 'abs_linear'): (5.76, 1.59),
    ('ragged', None, 'quadratic', 'abs_linear'): (0.891, 1.6),
    ('rbf', 0, 'quadratic', 'abs_linear'): (0.978, 1.03),
    ('rbf', 1, 'quadratic', 'abs_linear'): (1.46, 1.15),
    ('rbf', 63, 'quadratic', 'abs_linear'): (7.96, 2.87),
    ('rbf', 64, 'quadratic', 'abs_linear'): (7.74, 1.8),
    ('rbf', 130, 'quadratic', 'abs_linear'): (5.16, 1.32),
    ('rbf', 300, 'quadratic', 'abs_linear'): (8.25, 1.38),
    ('rbf', 65, 'quadratic', 'const'): (13.3, 4.93),
    ('rbf', 65, 'quadratic', 'abs_linear'): (7.71, 1.81),
    ('rbf', 65, 'quadratic', 'norm_linear'): (12.1, 3.06),
    # (the oracle holds the negated values of a negated table: the same function, the same figures)
    ('rbf', 65, 'table', 'const'): (16.2, 5.94), ('rbf', 65, 'negtable', 'const'): (16.2, 5.94),
    ('rbf', 65, 'table', 'abs_linear'): (21.8, 3.86), ('rbf', 65, 'negtable', 'abs_linear'): (21.8, 3.86),
    ('rbf', 65, 'table', 'norm_linear'): (28.4, 4.99), ('rbf', 65, 'negtable', 'norm_linear'): (28.4, 4.99),
    ('rbf', 65, 'table', 'abs_grad'): (20.9, 3.73), ('rbf', 65, 'negtable', 'abs_grad'): (20.9, 3.73),
    ('rbf', 65, 'table', 'norm_grad'): (27.3, 4.78), ('rbf', 65, 'negtable', 'norm_grad'): (27.3, 4.78),
    ('pendulum', None, 'negtable', 'abs_grad'): (3.94, 1.49),
    ('pendulum', None, 'table', 'abs_grad'): (3.94, 1.49),
    ('pendulum', None, 'table', 'norm_linear'): (3.91, 2.09)}
RBF_SIZES = (0, 1, 63, 64, 65, 130, 300)          # training points of the one-head RBF pendulum
COMBOS = [(v, lv) for v in V_KINDS for lv in LV_KINDS if not (v == "quadratic" and "grad" in lv)]
SYSTEM_KEYS = [(name, None, "quadratic", "abs_linear") for name in ("pendulum", "cartpole", "two", "ragged")]
GPU_KEYS = (SYSTEM_KEYS + [("rbf", k, "quadratic", "abs_linear") for k in RBF_SIZES if k != 65]
            + [("rbf", 65, v, lv) for v, lv in COMBOS]
            + [("pendulum", None, "negtable", "abs_grad"), ("pendulum", None, "table", "abs_grad"),
               ("pendulum", None, "table", "norm_linear")])


def measure_reference_ratio(key):
    system, n_gp, v_kind, lv_kind = key
    case = _case(system, n_gp)
    dynamics = _oracle_dynamics(case)
    safe = safe_spec(case, v_kind, lv_kind)
    states, actions = states_of(system, RATIO_POINTS)
    ok = comparable(dynamics, safe, states, actions)
    assert 1.0 - ok.mean() <= MAX_EXCLUDED, (key, 1.0 - ok.mean())
    t64 = constraint_terms(dynamics, safe, states, actions)
    t80 = constraint_terms(dynamics, safe, states, actions, LONG)
    assert (t64["A"][ok] > 0).all() and (t64["A_c"][ok] > 0).all()
    return (T.ratio_to_companion(t64["grad"], t80["grad"], t64["A"], ok),
            T.ratio_to_companion(t64["c"], t80["c"], t64["A_c"], ok))


def reference_ratio(key):
    return recorded_or_measured(REFERENCE_RATIO, key, measure_reference_ratio)


def tolerance(key):
    """-> (tolerance for dC/du, tolerance for C), each 32 times the reference's own measured error."""
    r_grad, r_c = reference_ratio(tuple(key))
    return training_tolerance.tolerance(r_grad), training_tolerance.tolerance(r_c)
