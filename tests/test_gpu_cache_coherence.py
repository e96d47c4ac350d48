"""State the engine keeps between calls follows inputs edited IN PLACE (needs an MI355X).

The engine keeps what it derived from its inputs between calls: the successor cache and its
policy-select arrays (csrc/sl_succ.hip), the distinct actions and tile order of k_bellman4_policy
(sl_bellman4.hip), the GP heads / tables / networks of every ModelBuilder (_model.py), the
persistent builder of the point evaluation (_evaluate.py).  Each piece is keyed on a token, and is
only right if every way a user can change an input also changes that token.  Every scenario here
warms the engine, checks that the next call is served from what it keeps, changes ONE input without
building a new object, calls again and compares with a freshly built engine object of the changed
problem (bit for bit where both take the same kernel) and with the oracle on the changed inputs."""

import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cases
import exclusions
import oracle
from test_gpu_rl import _rl_pair, ambiguous_points

pytestmark = pytest.mark.gpu

NV, NA = [12, 64], 5


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _actions(na=NA):
    return np.linspace(-1, 1, na)[:, None]


def _table(n, na=NA, seed=21):
    return _actions(na)[np.random.default_rng(seed).integers(0, na, n)]


def _edited(table, values, step=7):
    """Every `step`-th vertex moved to the next value of `values` (cyclically)."""
    out = table.copy()
    idx = np.arange(3, len(table), step)
    pos = np.argmax(values[None, :, 0] == out[idx], axis=1)
    out[idx] = values[(pos + 1) % len(values)]
    return out, idx


def _warm_max_sweeps(rl, vf, v0, actions):
    """Two Bellman max sweeps: the first fills the successor cache, the second is served from it."""
    for sweep in range(2):
        vf.parameters = v0.copy()
        rl.value_iteration(actions)
    assert "k_bellman_cached" in rl._ctx.last_kernel(), rl._ctx.last_kernel()


def _evaluate_policy(rl, vf, v0):
    """value_iteration() from v0, then bellmann_error(): (V, residual, error, kernel of the sweep)."""
    vf.parameters = v0.copy()
    res = rl.value_iteration()
    kernel = rl._ctx.last_kernel()
    return vf._host_parameters().copy(), res, rl.bellmann_error(), kernel


def _oracle_policy_evaluation(orl, ovf, v0, table, label):
    """The oracle's V after one policy-evaluation sweep under the per-vertex `table`, and the mask
    of vertices whose successor is not ambiguous in the oracle's table look-up."""
    orl.policy = lambda states, _table=table: _table
    x = orl.state_space
    ok = ~ambiguous_points(ovf, orl.dynamics(x, table)[0])
    exclusions.report(label, ok, "successor")
    ovf.parameters = v0.copy()
    orl.value_iteration()
    return ovf.parameters.copy(), ok


def _same(got, want):
    """Tables and residuals (a max) bit for bit; bellmann_error is a sum whose order of addition
    across workgroups is not fixed."""
    assert_array_equal(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])
    assert_allclose(got[2], want[2], rtol=1e-12)


# ---- rows 1 - 4: a per-vertex action table as the policy ---------------------------------------

@pytest.mark.parametrize("edit", ["setitem", "copy_", "flat"])
def test_device_tensor_policy_edited_under_the_select_cache(sl, edit):
    """Row 1: a CUDA float64 tensor policy after max sweeps filled the successor cache is served by
    k_bellman_cached<policy> through the select arrays; an in-place edit of the tensor (item
    assignment, copy_, a 1-D [nindex] tensor) must reach value_iteration() and bellmann_error()."""
    import torch
    case = cases.make_case("pendulum", num_points=NV, n_gp=70)
    actions = _actions()
    rl, orl, vf, ovf = _rl_pair(sl, case, NV)
    n = vf.discretization.nindex
    v0 = ovf.parameters.copy()
    table = _table(n)
    new, idx = _edited(table, actions)
    _warm_max_sweeps(rl, vf, v0, actions)
    shape = (n,) if edit == "flat" else (n, 1)
    t = torch.tensor(table.reshape(shape), dtype=torch.float64, device=rl._ctx.torch_device)
    rl.policy = t
    for _ in range(2):
        warm = _evaluate_policy(rl, vf, v0)
        assert "k_bellman_cached" in warm[3] and "policy" in warm[3], warm[3]
    hits = rl.successor_cache_info["policy_hits"]
    if edit == "copy_":
        t.copy_(torch.from_numpy(new.reshape(shape)))
    else:
        t[torch.from_numpy(idx).to(t.device)] = torch.from_numpy(new[idx].reshape((-1,) + shape[1:])).to(t.device)
    assert t.data_ptr() == rl._builder._policy_table.data_ptr()        # the engine reads t itself
    got = _evaluate_policy(rl, vf, v0)
    assert "k_bellman_cached" in got[3] and "policy" in got[3], got[3]
    assert rl.successor_cache_info["policy_hits"] == hits + 2
    # a fresh object of the changed problem, warmed the same way
    rl_f, _, vf_f, _ = _rl_pair(sl, case, NV)
    _warm_max_sweeps(rl_f, vf_f, v0, actions)
    rl_f.policy = torch.tensor(new.reshape(shape), dtype=torch.float64, device=rl_f._ctx.torch_device)
    fresh = _evaluate_policy(rl_f, vf_f, v0)
    assert "k_bellman_cached" in fresh[3], fresh[3]
    _same(got, fresh)
    want, ok = _oracle_policy_evaluation(orl, ovf, v0, new, "cache_coherence_tensor_policy[%s]" % edit)
    assert_allclose(got[0][ok], want[ok], rtol=1e-9, atol=1e-12)
    assert not np.array_equal(got[0], warm[0])                         # the edit matters


def test_device_tensor_policy_edited_under_the_policy_data_of_bellman4(sl):
    """Row 2: without the successor cache k_bellman4_policy keeps the distinct actions and the tile
    order of a table policy; an in-place edit with values of the old action set, then with a value
    outside it, must be evaluated as the new table (not through the old action list)."""
    import torch
    case = cases.make_case("pendulum", num_points=NV, n_gp=70)
    actions = _actions()
    rl, orl, vf, ovf = _rl_pair(sl, case, NV, cache=False)
    n = vf.discretization.nindex
    v0 = ovf.parameters.copy()
    table = _table(n, seed=22)
    t = torch.tensor(table, dtype=torch.float64, device=rl._ctx.torch_device)
    rl.policy = t
    first = _evaluate_policy(rl, vf, v0)
    second = _evaluate_policy(rl, vf, v0)
    assert "k_bellman4_policy" in first[3] and "reused" not in first[3], first[3]
    assert "k_bellman4_policy" in second[3] and "reused" in second[3], second[3]
    _same(second, first)
    inside, _ = _edited(table, actions)
    outside = inside.copy()
    outside[n // 2 + 5::11] = 0.123
    for label, new in (("inside", inside), ("outside", outside)):
        t.copy_(torch.from_numpy(new))
        got = _evaluate_policy(rl, vf, v0)
        assert "k_bellman4_policy" in got[3] and "reused" not in got[3], got[3]
        rl_f, _, vf_f, _ = _rl_pair(sl, case, NV, cache=False)
        rl_f.policy = torch.tensor(new, dtype=torch.float64, device=rl_f._ctx.torch_device)
        fresh = _evaluate_policy(rl_f, vf_f, v0)
        assert "k_bellman4_policy" in fresh[3], fresh[3]
        _same(got, fresh)
        want, ok = _oracle_policy_evaluation(orl, ovf, v0, new, "cache_coherence_bellman4_policy[%s]" % label)
        assert_allclose(got[0][ok], want[ok], rtol=1e-9, atol=1e-12)
        again = _evaluate_policy(rl, vf, v0)                           # the new table's data are kept
        assert "reused" in again[3], again[3]
        _same(again, got)


def test_unchanged_tensor_policy_keeps_both_caches(sl):
    """Row 3: a tensor policy that is not touched between sweeps keeps the select arrays of the
    successor cache and the policy data of k_bellman4_policy (no recomputation per sweep)."""
    import torch
    case = cases.make_case("pendulum", num_points=NV, n_gp=70)
    actions = _actions()
    rl, _, vf, ovf = _rl_pair(sl, case, NV)
    rl_u, _, vf_u, _ = _rl_pair(sl, case, NV, cache=False)
    n = vf.discretization.nindex
    v0 = ovf.parameters.copy()
    table = _table(n, seed=23)
    _warm_max_sweeps(rl, vf, v0, actions)
    rl.policy = torch.tensor(table, dtype=torch.float64, device=rl._ctx.torch_device)
    rl_u.policy = torch.tensor(table, dtype=torch.float64, device=rl_u._ctx.torch_device)
    hits = rl.successor_cache_info["policy_hits"]
    runs = [(_evaluate_policy(rl, vf, v0), _evaluate_policy(rl_u, vf_u, v0)) for _ in range(2)]
    for (c, u) in runs:
        assert "k_bellman_cached" in c[3] and "policy" in c[3], c[3]
        assert_allclose(c[0], u[0], rtol=1e-11, atol=1e-13)
    assert "reused" not in runs[0][1][3] and "reused" in runs[1][1][3], runs[1][1][3]
    assert rl.successor_cache_info["policy_hits"] == hits + 4
    _same(runs[1][0], runs[0][0])
    _same(runs[1][1], runs[0][1])


@pytest.mark.parametrize("kind", ["cpu_tensor", "cuda_float32", "numpy"])
def test_copied_policy_tables_edited_in_place(sl, kind):
    """Row 4 (controls): a CPU tensor, a float32 device tensor and a NumPy array are copied into a
    float64 device table at every upload, so an in-place edit reaches the next sweep."""
    import torch
    case = cases.make_case("pendulum", num_points=NV, n_gp=70)
    actions = _actions()
    rl, orl, vf, ovf = _rl_pair(sl, case, NV)
    n = vf.discretization.nindex
    v0 = ovf.parameters.copy()
    table = _table(n, seed=24)
    new, idx = _edited(table, actions)

    def make(values, ctx):
        if kind == "numpy":
            return values.copy()
        if kind == "cpu_tensor":
            return torch.tensor(values, dtype=torch.float64)
        return torch.tensor(values, dtype=torch.float32, device=ctx.torch_device)

    _warm_max_sweeps(rl, vf, v0, actions)
    policy = make(table, rl._ctx)
    rl.policy = policy
    warm = _evaluate_policy(rl, vf, v0)
    assert "k_bellman_cached" in warm[3], warm[3]
    if kind == "numpy":
        policy[idx] = new[idx]
    else:
        policy[torch.from_numpy(idx).to(policy.device)] = torch.from_numpy(new[idx]).to(policy.device, policy.dtype)
    got = _evaluate_policy(rl, vf, v0)
    assert "k_bellman_cached" in got[3], got[3]
    rl_f, _, vf_f, _ = _rl_pair(sl, case, NV)
    _warm_max_sweeps(rl_f, vf_f, v0, actions)
    rl_f.policy = make(new, rl_f._ctx)
    _same(got, _evaluate_policy(rl_f, vf_f, v0))
    want, ok = _oracle_policy_evaluation(orl, ovf, v0, new, "cache_coherence_copied_policy[%s]" % kind)
    assert_allclose(got[0][ok], want[ok], rtol=1e-9, atol=1e-12)


# ---- Lyapunov problems --------------------------------------------------------------------------

LYAP_KW = dict(num_points=40, n_gp=60, tau_scale=0.0)


def _lyapunov_pair(case):
    from safe_learning_amd.benchmarks import build_lyapunov
    return build_lyapunov(case), cases.oracle_lyapunov(case)


def _records(lyap):
    from test_gpu_lyapunov import _engine_records
    return _engine_records(lyap)[2]


def _check_safe_set(lyap, olyap, fresh):
    """Per-cell records [decrease, threshold, mean, error] of the decrease sweep, safe set and c_max
    of `lyap` against a fresh object (bit for bit) and the oracle; returns the records."""
    rec, rec_fresh = _records(lyap), _records(fresh)
    assert_array_equal(rec, rec_fresh)
    orec = cases.oracle_cell_records(olyap, np.arange(olyap.discretization.nindex))
    assert_allclose(rec[:, 2:], orec[:, 2:], rtol=1e-8, atol=1e-12)
    for other in (olyap, fresh):
        other.update_safe_set()
    lyap.update_safe_set()
    assert_array_equal(lyap.safe_set, fresh.safe_set)
    assert lyap.c_max == fresh.c_max
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max
    return rec


def test_lyapunov_with_a_tensor_policy_edited_in_place(sl):
    """Row 5 (control): update_safe_set with a device tensor per-vertex policy, edited in place."""
    import torch
    case = cases.make_case("pendulum", **LYAP_KW)
    lyap, olyap = _lyapunov_pair(case)
    fresh, _ = _lyapunov_pair(case)
    ogrid = olyap.discretization
    x = ogrid.all_points
    table = np.clip(x.dot(case["K"].T), -1, 1)
    new = table.copy()
    new[::5] *= 0.5
    t = torch.tensor(table, dtype=torch.float64, device=lyap._ctx.torch_device)
    lyap.policy = t
    host = table.copy()
    olyap.policy = lambda states: host[ogrid.state_to_index(states)]
    fresh.policy = torch.tensor(table, dtype=torch.float64, device=fresh._ctx.torch_device)
    _check_safe_set(lyap, olyap, fresh)
    t.copy_(torch.from_numpy(new))
    host[:] = new
    fresh.policy = torch.tensor(new, dtype=torch.float64, device=fresh._ctx.torch_device)
    _check_safe_set(lyap, olyap, fresh)


def _count_uploads(monkeypatch, ctx):
    """Record the full head uploads and the appended rows of a context (for this test only)."""
    calls = []
    for name in ("gp_set_head", "gp_set_head_kernel", "gp_append_point"):
        real = getattr(ctx, name)
        monkeypatch.setattr(ctx, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _rbf_change(kern):
    # (smaller variance, shorter length scale: the posterior variance with the old factors stays
    # positive)
    kern.variance = 0.8 * kern.variance
    kern.lengthscales[0] *= 0.9


@pytest.mark.parametrize("update_cache", [False, True], ids=["live_kernel", "update_cache"])
def test_rbf_hyper_parameters_assigned_after_construction(sl, update_cache, monkeypatch):
    """Rows 6 and 8: `kern.variance = ...`, `kern.lengthscales[0] *= ...` of the dynamics' RBF GP.
    Without update_cache() the cached factors stay and the kernel is live (reference functions.py
    :438-450; the oracle does the same); with update_cache() the factors are rebuilt as well.  Both
    must reach update_safe_set, the successor cache of value_iteration(actions) (it refills) and
    the point evaluation of the shared evaluation builder."""
    from safe_learning_amd import _evaluate
    case = cases.make_case("pendulum", **LYAP_KW)
    lyap, olyap = _lyapunov_pair(case)
    fresh, _ = _lyapunov_pair(case)
    lyap.update_safe_set()
    olyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    uploads = _count_uploads(monkeypatch, lyap._ctx)
    lyap.update_safe_set()
    assert uploads == []                                   # warm: nothing is uploaded again
    perturbations, limits = np.array([[0.], [0.1], [-0.1]]), np.array([[-1., 1.]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sl.get_safe_sample(lyap, perturbations, limits, positive=True, num_samples=100)
    ectx, _ = _evaluate._builder(2)
    eval_uploads = _count_uploads(monkeypatch, ectx)
    rng = np.random.default_rng(31)
    states, acts = rng.uniform(-1, 1, (50, 2)), rng.uniform(-1, 1, (50, 1))
    before = _evaluate.dynamics(lyap.dynamics, states, acts)
    assert eval_uploads == []                              # warm: the evaluation builder has the GP
    # the successor cache of a PolicyIteration on the same GP model
    actions = _actions()
    rl, orl, vf, ovf = _rl_pair(sl, cases.make_case("pendulum", num_points=NV, n_gp=70), NV)
    rl_u, _, vf_u, _ = _rl_pair(sl, cases.make_case("pendulum", num_points=NV, n_gp=70), NV, cache=False)
    v0 = ovf.parameters.copy()
    _warm_max_sweeps(rl, vf, v0, actions)
    rec_before = _records(lyap)

    for gp, ogp in ((lyap.dynamics.gaussian_process, olyap.dynamics.gaussian_process),
                    (fresh.dynamics.gaussian_process, None),
                    (rl.dynamics.gaussian_process, orl.dynamics.gaussian_process),
                    (rl_u.dynamics.gaussian_process, None)):
        for model in (gp, ogp):
            if model is None:
                continue
            _rbf_change(model.kern)
            if update_cache:
                model.update_cache()
    # (`fresh` and `rl_u` upload the changed model for the first time; the warm objects must follow)
    rec = _check_safe_set(lyap, olyap, fresh)
    assert "gp_set_head" in uploads and "gp_append_point" not in uploads, uploads
    assert not np.array_equal(rec[:, 4:], rec_before[:, 4:])            # the change matters
    # point evaluation on the shared builder
    mean, err = _evaluate.dynamics(lyap.dynamics, states, acts)
    assert "gp_set_head" in eval_uploads and "gp_append_point" not in eval_uploads, eval_uploads
    omean, oerr = olyap.dynamics(states, acts)
    assert_allclose(mean, omean, rtol=1e-8, atol=1e-12)
    assert_allclose(err, oerr, rtol=1e-8, atol=1e-12)
    assert not np.allclose(err, before[1], rtol=1e-6, atol=0)      # the change matters
    # value_iteration(actions): the successor cache refills, the tables equal a cache-less context
    for r, v in ((rl, vf), (rl_u, vf_u)):
        v.parameters = v0.copy()
        r.value_iteration(actions)
    assert "k_bellman_cached" not in rl._ctx.last_kernel(), rl._ctx.last_kernel()
    assert_array_equal(vf._host_parameters(), vf_u._host_parameters())
    assert_array_equal(rl.policy._host_parameters(), rl_u.policy._host_parameters())
    orl.policy = oracle.Triangulation(ovf.discretization, np.zeros((ovf.discretization.nindex, 1)))
    x = orl.state_space
    ok = np.ones(len(x), dtype=bool)
    for action in actions:
        ok &= ~ambiguous_points(ovf, orl.dynamics(x, np.broadcast_to(action, (len(x), 1)))[0])
    exclusions.report("cache_coherence_rbf_successors", ok, "successor")
    ovf.parameters = v0.copy()
    oq, _ = orl.discrete_policy_optimization(actions)
    assert_allclose(vf._host_parameters()[ok, 0], oq.max(axis=1)[ok], rtol=1e-9, atol=1e-12)
    for r, v in ((rl, vf), (rl_u, vf_u)):
        v.parameters = v0.copy()
        r.value_iteration(actions)
    assert "k_bellman_cached" in rl._ctx.last_kernel()
    assert_array_equal(vf._host_parameters(), vf_u._host_parameters())


def test_notebook_kernel_leaf_variance_changed(sl, monkeypatch):
    """Row 7: the notebooks' `Linear + Matern32 * Linear` heads (sl_gp_set_head_kernel); the
    variance of a Linear leaf assigned after construction must reach update_safe_set."""
    from safe_learning_amd.benchmarks import build_lyapunov, notebook_kernels
    case = cases.make_case("pendulum", stack=True, **LYAP_KW)
    case["dynamics"]["kernels"] = notebook_kernels(case)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    lyap.update_safe_set()
    olyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    uploads = _count_uploads(monkeypatch, lyap._ctx)
    lyap.update_safe_set()
    assert uploads == []

    def change(dynamics):
        leaf = dynamics.functions[1].gaussian_process.kern.kern_list[0]      # Linear(3, ARD)
        leaf.variance = 0.5 * leaf.variance

    rec_before = _records(lyap)
    change(lyap.dynamics)
    change(olyap.dynamics)
    fresh = build_lyapunov(case)
    change(fresh.dynamics)
    rec = _check_safe_set(lyap, olyap, fresh)
    assert "gp_set_head_kernel" in uploads, uploads
    assert not np.array_equal(rec[:, 4:], rec_before[:, 4:])            # the change matters


def test_two_problems_alternate_on_the_evaluation_builder(sl):
    """Row 9: two Lyapunov problems share the evaluation context's one builder; one of them adds a
    data point in between.  The append log of one GP must never be applied to the head of the
    other (a full upload then), and each get_safe_sample equals the oracle's."""
    from safe_learning_amd.benchmarks import _true_dynamics_numpy
    case_a = cases.make_case("pendulum", seed=0, **LYAP_KW)
    case_b = cases.make_case("pendulum", seed=5, **LYAP_KW)
    pairs = [_lyapunov_pair(case_a), _lyapunov_pair(case_b)]
    perturbations, limits = np.array([[0.], [0.1], [-0.1]]), np.array([[-1., 1.]])
    for lyap, olyap in pairs:
        lyap.update_safe_set()
        olyap.update_safe_set()
    for step in range(4):
        for k, (lyap, olyap) in enumerate(pairs):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                np.random.seed(step)
                sa, bound = sl.get_safe_sample(lyap, perturbations, limits, positive=True, num_samples=150)
                np.random.seed(step)
                osa, obound = oracle.get_safe_sample(olyap, perturbations, limits, positive=True,
                                                     num_samples=150)
            assert_allclose(bound, obound, rtol=1e-7)
            assert_array_equal(sa, osa)
            if k == 0 and step < 2:
                y = _true_dynamics_numpy(case_a, osa)
                lyap.dynamics.add_data_point(sa, y)
                olyap.dynamics.add_data_point(osa, y)


# ---- Triangulation tables and networks ---------------------------------------------------------

def test_triangulation_parameters_refuse_in_place_writes(sl):
    """Row 10: the host table `parameters` returns cannot be written into (the device copies of a
    V table or a policy table would not follow); assigning a new array is followed."""
    case = cases.make_case("pendulum", num_points=NV, n_gp=70)
    rl, orl, vf, ovf = _rl_pair(sl, case, NV)
    n = vf.discretization.nindex
    v0 = ovf.parameters.copy()
    table = _table(n, seed=25)
    rl.policy = sl.Triangulation(vf.discretization, table)
    vf.parameters = v0.copy()
    rl.value_iteration()
    with pytest.raises(ValueError):
        vf.parameters[3] = 1.0
    with pytest.raises(ValueError):
        rl.policy.parameters[3] = -table[3]
    with pytest.raises(ValueError):
        vf.parameters += 1.0
    # a table adopted from the device (value iteration) reads back read-only too
    assert isinstance(vf.parameters, np.ndarray) and not vf.parameters.flags.writeable
    # assignments are followed
    new, _ = _edited(table, _actions())
    v1 = v0 - 0.25
    rl.policy.parameters = new
    vf.parameters = v1.copy()
    rl.value_iteration()
    got = vf._host_parameters().copy()
    rl_f, _, vf_f, _ = _rl_pair(sl, case, NV)
    rl_f.policy = sl.Triangulation(vf_f.discretization, new)
    vf_f.parameters = v1.copy()
    rl_f.value_iteration()
    assert_array_equal(got, vf_f._host_parameters())
    orl.policy = oracle.Triangulation(ovf.discretization, new)
    ovf.parameters = v1.copy()
    x = orl.state_space
    label = "cache_coherence_triangulation_assign"
    amb = exclusions.check_own_vertices(label, orl, orl.policy, x, got)
    ok = ~amb & ~ambiguous_points(ovf, orl.dynamics(x, orl.policy(x))[0])
    exclusions.report(label, ok | amb, "successor")
    orl.value_iteration()
    assert_allclose(got[ok], ovf.parameters[ok], rtol=1e-9, atol=1e-12)


def test_lyapunov_network_weights_edited_in_place(sl):
    """Row 11: the weights of a LyapunovNetwork V edited in place; update_values() follows (the
    builder's signature hashes the weight bytes)."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=40, dynamics="analytic", tau_scale=0.0)
    dims = [16, 16, 24]
    case["V"] = {"kind": "network", "layer_dims": dims, "activations": ["tanh"] * 3, "eps": 1e-8,
                 "weights": cases.lyapunov_like_network_weights(case["P"], dims)}
    case["lv"] = ("norm_grad",)
    weights = [w.copy() for w in case["V"]["weights"]]
    lyap = build_lyapunov(case)                     # (shares the arrays of case["V"]["weights"])
    before = lyap.values.copy()
    lyap.update_values()
    assert_array_equal(lyap.values, before)
    lyap.lyapunov_function.weights[0][:] *= 1.25                       # W of the first layer
    lyap.update_values()
    case2 = dict(case)
    case2["V"] = dict(case["V"], weights=weights)
    weights[0] = weights[0] * 1.25
    fresh, olyap = build_lyapunov(case2), cases.oracle_lyapunov(case2)
    assert_array_equal(lyap.values, fresh.values)
    assert_allclose(lyap.values, olyap.values, rtol=1e-12, atol=1e-18)
    assert not np.array_equal(lyap.values, before)
