"""The ledger of the GP kernels of the Lyapunov sweep: every instantiation of ``k_gp_small`` (``sl_gp_small.hip``)
and ``k_gp_sweep`` (``sl_gp.hip``) that the dispatch sites compile, and for each one either the existing test that
asserts its kernel note, the smallest case that selects it, or the reason why no sweep can select it.

Plain data and a few lines of arithmetic; imports without torch and without a GPU (NumPy and the package's case
builders are imported inside the functions that build a case).  ``tests/test_gp_sweep_matrix_host.py`` holds the
ledger against the sources (the dispatch lists, the constants, the launchers' rules restated here, the oracle-side
well-posedness of every case); ``tests/test_gpu_gp_sweep_matrix.py`` runs the cases.

``sl_with_dim<D0, D1, ...>(v, f)`` calls ``f`` with the first listed value equal to ``v`` and with the LAST listed
value when none matches: a site's list is the set of instantiations it compiles.
"""

import ctypes as C

# ---------------------------------------------------------------------------------------------
# The dispatch lists as the sources state them, unit by unit in source order.
# ---------------------------------------------------------------------------------------------
DISPATCH = {
    "sl_common.h": [
        ("sl_with_dim: its own recursion", ("Ds...",)),
        ("sl_with_flavour: d of the table flavours (GENERAL)", ("2", "0")),
        ("sl_with_flavour: d of the fast flavours", ("1", "2", "3", "4", "0")),
    ],
    "sl_gp_small.hip": [
        ("k_gp_small: flags (bit 1: factor in LDS, bit 0: sum-of-products heads)", ("3", "2", "1", "0")),
        ("k_gp_small: wavefronts, DT > 0", ("WAVES_MAX", "WAVES_TOP", "WAVES_TINY", "WAVES_MIN")),
        ("k_gp_small: wavefronts, DT = 0", ("WAVES_MIN",)),
    ],
    "sl_gp.hip": [
        ("gp_sweep_xs_global: d (0: the generic table flavour)", ("4", "2", "0")),
        ("sl_debug_fp64_rate: which probe (no sweep kernel)", ("0", "1", "2", "3", "4", "5", "6", "7", "8")),
    ],
}
# the two panel shapes of k_gp_sweep: index 0 the configuration of small heads, 1 every other
CFG = {"kCfgW": (4, 8), "kCfgR": (1, 4), "kCfgCB": (1, 4)}

# The constants the rules use (names of the sources where they have one).
CONSTANTS = dict(
    WAVES_TINY=4, WAVES_MIN=8, WAVES_MAX=12, WAVES_TOP=16,
    # round-cost weights of 4 / 8 / 12 wavefronts; of 16 with the factor in LDS | where 12 would have it | from L2
    WEIGHTS=(105, 128, 160, (220, 240, 190)),
    COUNTER_EXTRA=12,                  # added to the weight of eight wavefronts when the tile counter is on
    ROUNDS=4,                          # the round-cost rule holds below ROUNDS * num_cu * WAVES_TOP tiles
    LDS_BYTES=160 * 1024, LDS_RESERVE=256,
    SMALL_PAD_MAX=256,                 # sl_gp_small_supports: padded capacity of a head
    ONE_PANEL_PAD=256, ONE_PANEL_ABOVE=224,      # gp4_one_panel: n_pad == 256 and n > 224
    SMALL_HEAD_MAX=256,                # choose_cfg: up to 256 points the small configuration
    SL_GP_SLABS_PER_CHUNK=16,
    SL_MAX_STATE_DIM=6, SL_MAX_INPUT_DIM=8, SL_MAX_SIMPLICES=32, SL_KERNEL_MAX_FACTORS=8,
    SL_TRI_CODES=64, SL_TRI_MAXCAND=12,
)


def tri_offset(i):
    """128-double fragments of the factor's lower triangle before row block ``i``."""
    return i * (i + 1)


# ---- sizeof(SlTri) and sizeof(sl_gp_kernel), restated member by member (the host test holds the member lists
# against sl_model.h / sl_hip.h): the table flavours keep two SlTri in static LDS, a head with a kernel
# description KERNEL_DOUBLES more doubles -------------------------------------------------------------------
_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "uint8_t": C.c_uint8,
           "const double*": C.c_void_p}
GRID_DESC_MEMBERS = [("int32_t", "d", ()), ("int32_t", "reserved", ()), ("int64_t", "num_points", ("SL_MAX_STATE_DIM",)),
                     ("double", "offset", ("SL_MAX_STATE_DIM",)), ("double", "unit_maxes", ("SL_MAX_STATE_DIM",)),
                     ("double", "upper", ("SL_MAX_STATE_DIM",))]
TRI_MEMBERS = [
    ("sl_grid_desc", "grid", ()), ("int32_t", "nsimplex", ()), ("int32_t", "project", ()), ("int32_t", "ncols", ()),
    ("int32_t", "set", ()), ("int32_t", "simplices", ("SL_MAX_SIMPLICES", "SL_D + 1")),
    ("double", "hyper", ("SL_MAX_SIMPLICES", "SL_D", "SL_D")), ("double", "hyper_c", ("SL_MAX_SIMPLICES", "SL_D")),
    ("int64_t", "stride", ("SL_D",)), ("const double*", "points", ()), ("int32_t", "points_off", ("SL_D",)),
    ("int32_t", "affine_points", ()), ("int32_t", "reserved", ()), ("double", "inv_unit", ("SL_D",)),
    ("uint8_t", "ncand", ("SL_TRI_CODES",)), ("uint8_t", "cand", ("SL_TRI_CODES", "SL_TRI_MAXCAND")),
    ("int32_t", "has_fine", ()), ("int32_t", "reserved2", ()), ("uint8_t", "perm_index", ("SL_TRI_CODES",)),
    ("uint8_t", "fine", ("24 * 64", "4")), ("const double*", "table", ()),
]
KERNEL_FACTOR_MEMBERS = [("int32_t", "kind", ()), ("int32_t", "product", ()),
                         ("double", "variance", ("SL_MAX_INPUT_DIM",)),
                         ("double", "inv_lengthscales", ("SL_MAX_INPUT_DIM",))]
KERNEL_MEMBERS = [("int32_t", "nfactors", ()), ("int32_t", "reserved", ()),
                  ("sl_gp_kernel_factor", "factor", ("SL_KERNEL_MAX_FACTORS",))]


def _struct(members, k, nested):
    names = dict(k, SL_D=k["SL_MAX_STATE_DIM"])
    fields = []
    for ctype, name, dims in members:
        t = nested[ctype] if ctype in nested else _CTYPES[ctype]
        for dim in reversed(dims):
            t = t * int(eval(dim, {}, names))
        fields.append((name, t))
    return type("S", (C.Structure,), {"_fields_": fields})


def tri_lds_bytes(k=CONSTANTS):
    """sizeof(SlTriLds<true>): two SlTri."""
    grid = _struct(GRID_DESC_MEMBERS, k, {})
    return 2 * C.sizeof(_struct(TRI_MEMBERS, k, {"sl_grid_desc": grid}))


def kernel_doubles(k=CONSTANTS):
    """KERNEL_DOUBLES: sizeof(sl_gp_kernel) in 16-byte units, as doubles."""
    factor = _struct(KERNEL_FACTOR_MEMBERS, k, {})
    return (C.sizeof(_struct(KERNEL_MEMBERS, k, {"sl_gp_kernel_factor": factor})) + 15) // 16 * 2


# ---------------------------------------------------------------------------------------------
# What the lists compile.
# ---------------------------------------------------------------------------------------------
def _values(unit, index, k):
    return [int(k.get(v, v)) for v in DISPATCH[unit][index][1]]


def flavours(k=CONSTANTS):
    """(general, d, m) of sl_with_flavour: m = 1 beside a compile-time d, 0 beside d = 0."""
    return ([(0, d, int(d != 0)) for d in _values("sl_common.h", 2, k)] +
            [(1, d, int(d != 0)) for d in _values("sl_common.h", 1, k)])


def instantiations(k=CONSTANTS):
    """kernel -> set of parameter tuples.
    k_gp_small: (general, d, m, factor in LDS, wavefronts, sum-of-products heads);
    k_gp_sweep: (W, R, CB, general, d, m, xs_global)."""
    flags = _values("sl_gp_small.hip", 0, k)
    small = set()
    for g, d, m in flavours(k):
        for w in _values("sl_gp_small.hip", 1 if d > 0 else 2, k):
            small |= {(g, d, m, (f >> 1) & 1, w, f & 1) for f in flags}
    sweep = {(CFG["kCfgW"][s], CFG["kCfgR"][s], CFG["kCfgCB"][s], g, d, m, 0) for s in (0, 1) for g, d, m in flavours(k)}
    sweep |= {(8, 4, 4, int(d == 0), d, int(d != 0), 1) for d in _values("sl_gp.hip", 0, k)}
    return {"k_gp_small": small, "k_gp_sweep": sweep}


def small_note(p, heads):
    return "k_gp_small<general=%d, d=%d, m=%d, Linv in %s, %d wavefronts> (%d head(s))" % (
        p[0], p[1], p[2], "LDS" if p[3] else "L2", p[4], heads)


def sweep_note(p):
    return "k_gp_sweep<W=%d, R=%d, CB=%d, general=%d, d=%d, m=%d, xs_global=%d>" % tuple(p)


# ---------------------------------------------------------------------------------------------
# The rules that pick an instantiation, restated.  A model is described by
#   d, m, p = d + m, general, heads = [(n, dout, has a kernel description), ...]
# and a context by its switches env = {"SL_GP_CFG": .., "SL_GP_SMALL": .., "SL_GP_SMALL_WAVES": ..,
# "SL_GP4_ONE_PANEL": ..} (strings as a test sets them; absent = -1).
# ---------------------------------------------------------------------------------------------
SWITCHES = ("SL_GP_CFG", "SL_GP_SMALL", "SL_GP_SMALL_WAVES", "SL_GP4_ONE_PANEL")


def _env(env, name):
    value = int((env or {}).get(name, -1))
    if name == "SL_GP_CFG" and (value == 1 or value > 3):
        value = -1
    return value


def sl_dim_variant_of(d, m):
    return d if m == 1 and 1 <= d <= 4 else 0


def sl_model_is_general(value_kind, policy_kind, lv_kind):
    """Kinds by name: value 'quadratic' | 'table' | 'network', policy 'linear' | 'table',
    lv 'const' | 'abs_linear' | 'norm_linear' | 'abs_grad' | 'norm_grad'."""
    return value_kind != "quadratic" or policy_kind == "table" or lv_kind in ("abs_grad", "norm_grad")


def flavour_of(general, d, m, k=CONSTANTS):
    """sl_with_flavour(general, sl_dim_variant_of(model)) -> (general, d, m) of the instantiation."""
    variant = sl_dim_variant_of(d, m)
    listed = _values("sl_common.h", 1 if general else 2, k)
    dt = variant if variant in listed else listed[-1]
    return (int(general), dt, int(dt != 0))


def head_cfg(n, env, k=CONSTANTS):
    """choose_cfg."""
    forced = _env(env, "SL_GP_CFG")
    return forced if forced >= 0 else (0 if n <= k["SMALL_HEAD_MAX"] else 2)


def n_pad(n, env=None, k=CONSTANTS):
    """Padded capacity of a head: whole panels of its configuration (cfg_panel_rows)."""
    s = int(head_cfg(n, env, k) != 0)
    rows = 16 * CFG["kCfgR"][s] * CFG["kCfgW"][s]
    return -(-n // rows) * rows


def lds_capacity(general, k=CONSTANTS):
    return k["LDS_BYTES"] - (tri_lds_bytes(k) if general else 0) - k["LDS_RESERVE"]


def _small_doubles(heads, p, env, k):
    total = 0
    for n, dout, kern in heads:
        pad = n_pad(n, env, k)
        total += ((p * pad + 1) & ~1) + ((pad * dout + 1) & ~1) + (kernel_doubles(k) if kern else 0)
    return total


def _tri_doubles(heads):
    return sum(tri_offset((n + 15) // 16) * 128 for n, _, _ in heads)


def fits(waves, with_tri, heads, p, d, general, env=None, k=CONSTANTS):
    """launch_small's ``fits``: inputs, alpha' (and the factor) of every head plus the check's scratch of `waves`
    wavefronts within the LDS capacity."""
    doubles = _small_doubles(heads, p, env, k) + (_tri_doubles(heads) if with_tri else 0) + waves * 64 * (1 + 2 * d)
    return 8 * doubles <= lds_capacity(general, k)


def allowed(w, wcap, k=CONSTANTS):
    """launch_small's ``allowed`` under SL_GP_SMALL_WAVES = wcap (-1: unset)."""
    return (w == k["WAVES_MIN"] or wcap < 0 or (k["WAVES_MIN"] < w <= wcap) or
            (w == k["WAVES_TINY"] and wcap == k["WAVES_TINY"]))


def launch_small(ntiles, num_cu, heads, p, d, general, dt, waves_env=-1, k=CONSTANTS):
    """-> (wavefronts, factor in LDS) of launch_small<GENERAL, DT, MT> for a sweep of `ntiles` 64-cell tiles."""
    tiny, wmin, wmax_, top = k["WAVES_TINY"], k["WAVES_MIN"], k["WAVES_MAX"], k["WAVES_TOP"]

    def fit(w, tri):
        return fits(w, tri, heads, p, d, general, None, k)
    wmax = waves_env if waves_env >= 0 else top
    waves, alds = wmin, fit(wmin, True)
    if dt > 0 and ntiles < k["ROUNDS"] * num_cu * top:
        sizes = (tiny, wmin, wmax_, top)
        lds, loses, l2 = k["WEIGHTS"][3]
        weight = k["WEIGHTS"][:3] + (lds if fit(top, True) else (loses if fit(wmax_, True) else l2),)
        best = -1
        for i in range(4):
            if not allowed(sizes[i], waves_env, k) or not fit(sizes[i], False):
                continue
            per_round = sizes[i] * num_cu
            if ntiles > 4 * per_round:
                cost = ntiles * (weight[i] + (k["COUNTER_EXTRA"] if i == 1 else 0)) // per_round
            else:
                cost = -(-ntiles // per_round) * weight[i]
            if best < 0 or cost < best:
                best, waves = cost, sizes[i]
        alds = fit(waves, True)
    elif dt > 0 and allowed(wmax_, waves_env, k) and fit(wmax_, alds):
        waves = wmax_
    if dt > 0 and wmax >= top and ntiles >= k["ROUNDS"] * num_cu * top:
        if alds and fit(top, True):
            waves = top
        elif not (alds and waves == wmax_) and fit(top, False):
            waves, alds = top, False
    return waves, alds


def small_supports(heads, p, d, general, env=None, k=CONSTANTS):
    """sl_gp_small_supports (for heads of one input dimension)."""
    if _env(env, "SL_GP_SMALL") == 0 or not heads:
        return False
    if any(n_pad(n, env, k) > k["SMALL_PAD_MAX"] or n_pad(n, env, k) % 16 for n, _, _ in heads):
        return False
    return 8 * (_small_doubles(heads, p, env, k) + k["WAVES_MIN"] * 64 * (1 + 2 * d)) <= lds_capacity(general, k)


def xs_global_takes(heads, p, env=None, k=CONSTANTS):
    """The LDS test of gp_sweep_xs_global: the training inputs do not fit beside the fixed buffers."""
    xs_max = max(p * n_pad(n, env, k) for n, _, _ in heads)
    fixed = 8 * (2 * k["SL_GP_SLABS_PER_CHUNK"] * 4 * 64 + 8 * 64 + 8 * 16 * k["SL_MAX_STATE_DIM"] +
                 2 * 64 * k["SL_MAX_STATE_DIM"] + 2 * 8)
    return fixed + 8 * xs_max > k["LDS_BYTES"]


# the order of sl_gp_sweep_launch's chain; behind it the panel shape of the configuration
CHAIN = ("gp_small_other_kernels", "gp4_one_panel", "gp_small_cfg0", "gp4_cfg2", "gp_sweep_xs_global")


def select(model, env, ntiles, num_cu, k=CONSTANTS):
    """The kernel note's head for a sweep of `ntiles` tiles of `model` (see describe) in a context with the
    switches `env` on a device with `num_cu` compute units: sl_gp_sweep_launch's chain."""
    d, m, p, general, heads = model["d"], model["m"], model["p"], model["general"], model["heads"]
    kern = any(h[2] for h in heads)
    cfgs = {head_cfg(n, env, k) for n, _, _ in heads}
    assert len(cfgs) == 1, "sl_gp_configure refuses heads of different configurations"
    gp_cfg = cfgs.pop()
    flavour = flavour_of(general, d, m, k)
    gp4 = not general and sl_dim_variant_of(d, m) >= 1
    for step in CHAIN:
        if step == "gp_small_other_kernels":
            took = kern and small_supports(heads, p, d, general, env, k) and "small"
        elif step == "gp4_one_panel":
            took = (gp_cfg == 0 and not kern and gp4 and _env(env, "SL_GP4_ONE_PANEL") != 0 and
                    all(n_pad(n, env, k) == k["ONE_PANEL_PAD"] and n > k["ONE_PANEL_ABOVE"] for n, _, _ in heads)
                    and "k_gp_sweep4")
        elif step == "gp_small_cfg0":
            took = gp_cfg == 0 and small_supports(heads, p, d, general, env, k) and "small"
        elif step == "gp4_cfg2":
            took = gp_cfg == 2 and not kern and gp4 and "k_gp_sweep4"
        else:
            took = gp_cfg != 0 and xs_global_takes(heads, p, env, k) and "xs"
        if took == "small":
            waves, alds = launch_small(ntiles, num_cu, heads, p, d, general, flavour[1],
                                       _env(env, "SL_GP_SMALL_WAVES"), k)
            return small_note(flavour + (int(alds), waves), len(heads))
        if took == "xs":
            listed = _values("sl_gp.hip", 0, k)
            variant = 0 if general else sl_dim_variant_of(d, m)
            dt = variant if variant in listed else listed[-1]
            return sweep_note((8, 4, 4, int(dt == 0), dt, int(dt != 0), 1))
        if took:
            return took
    s = int(gp_cfg != 0)
    return sweep_note((CFG["kCfgW"][s], CFG["kCfgR"][s], CFG["kCfgCB"][s]) + flavour + (0,))


def describe(case):
    """The rules' view of a case dict (benchmarks.make_case's format)."""
    dyn = case["dynamics"]
    d, m = case["d"], case["m"]
    n = len(dyn["X"])
    heads = [(n, 1, "kernels" in dyn)] * d if case["stack"] else [(n, d, False)]
    general = sl_model_is_general(case.get("V", {"kind": "quadratic"})["kind"],
                                  "table" if "policy_table" in case else "linear", case["lv"][0])
    return dict(d=d, m=m, p=d + m, general=general, heads=heads)


# ---------------------------------------------------------------------------------------------
# Cases: one model family per flavour, a sum-of-products variant of each, and the training-set sizes that put the
# factor where an entry wants it.
# ---------------------------------------------------------------------------------------------
INFORMED = dict(signal_std=0.03, noise_std=0.0005, lengthscale=1.5)     # benchmarks.GP_VARIANTS['informed']
TIGHT = dict(signal_std=0.001, noise_std=0.0002, lengthscale=1.0)       # benchmarks.GP_VARIANTS['tight']

# family -> (flavour it selects, the grid of the round-cost cases, a small grid, builder kwargs)
FAMILIES = {
    "gp1d": ((0, 1, 1), [220002], [1500], dict(tau_scale=0.02)),
    "pendulum": ((0, 2, 1), [472, 473], [44, 39], dict(tau_scale=0.01, **INFORMED)),
    "chain3": ((0, 3, 1), [60, 61, 61], [9, 10, 13], dict(tau_scale=0.0005)),
    "cartpole": ((0, 4, 1), [22, 22, 22, 22], [6, 5, 5, 7], dict(tau_scale=0.0, **TIGHT)),
    "two_actions": ((0, 0, 0), None, [44, 39], dict(tau_scale=0.01)),
    "table": ((1, 2, 1), [472, 473], [44, 39], dict(tau_scale=0.01)),
    "table1d": ((1, 0, 0), None, [1500], dict(tau_scale=0.02)),
}
# (an even axis keeps the origin, where a Linear kernel's posterior variance is exactly zero, off the grid)
FAMILY_OF = {flavour: name for name, (flavour, _, _, _) in FAMILIES.items()}
# table vertices per axis: no interior line of the table grid passes through a cell (gcd(T - 1, N - 1) = 1)
TABLE_POINTS = {"table": (12, 10), "table1d": (12,)}


def case(family, num_points, n_gp, kernels=False, env=None, waves=None):
    """`waves`: the wavefront count the sweep range aims at (None: the whole grid)."""
    return dict(family=family, num_points=list(num_points), n_gp=n_gp, kernels=bool(kernels), env=dict(env or {}),
                waves=waves)


def case_id(c):
    return "%s-%s-n%d%s%s%s" % (c["family"], "x".join(map(str, c["num_points"])), c["n_gp"],
                               "-kernels" if c["kernels"] else "", "-w%d" % c["waves"] if c["waves"] else "",
                               "".join("-%s=%s" % kv for kv in sorted(c["env"].items())))


def _gp_data(case, true_matrix, prior, n_gp, noise_std, signal_std, lengthscale, seed=0):
    import numpy as np
    p = true_matrix.shape[1]
    X = np.random.default_rng(seed).uniform(-1, 1, (n_gp, p))
    Y = X @ true_matrix.T + np.random.default_rng(seed + 1).normal(0, noise_std, (n_gp, true_matrix.shape[0]))
    case["dynamics"] = {"kind": "gp", "X": X, "Y": Y, "variance": signal_std ** 2,
                        "lengthscales": np.full(p, lengthscale), "noise_variance": noise_std ** 2,
                        "prior": prior, "beta": 2.0}


def gp_1d_case(num_points, n_gp, tau_scale):
    """benchmarks.make_case('1d') (x' = x + u under u = -0.1 x) with its dynamics learned by a GP over [x, u] from
    noisy samples of x' = x + 0.9 u; prior: the nominal x + u."""
    import numpy as np
    from safe_learning_amd.benchmarks import make_case
    out = make_case("1d", num_points=num_points[0], tau_scale=tau_scale)
    out.update(A_true=np.array([[1.0]]), B_true=np.array([[0.9]]), initial_radius=0.2)
    del out["initial_set"]
    _gp_data(out, np.array([[1.0, 0.9]]), np.array([[1.0, 1.0]]), n_gp, **INFORMED)
    return out


def two_action_gp_case(num_points, n_gp, tau_scale):
    """The linear pendulum of make_case with a second input column (half the first one's gain on the other state)
    and a 2 x 2 saturated linear policy - the smallest model with two action dimensions, as in
    bellman_matrix.two_action_case - with GP dynamics over [x, u1, u2]."""
    import numpy as np
    from safe_learning_amd.benchmarks import make_case
    out = make_case("pendulum", num_points=num_points, dynamics="linear", tau_scale=tau_scale)
    a, b = out["A_true"], out["B_true"]
    b2 = np.hstack((b, 0.5 * b[::-1]))
    out.update(name="two_actions", m=2, K=np.vstack((out["K"], 0.3 * out["K"][:, ::-1])), B_true=b2)
    prior = np.hstack((a, b2)) * np.array([[1.0, 0.97, 1.0, 1.0], [0.97, 1.0, 0.9, 1.0]])
    _gp_data(out, np.hstack((a, b2)), prior, n_gp, **INFORMED)
    return out


def table_value(case, table_points):
    """V a piecewise-linear table (the quadratic plus a smooth bump, as benchmarks.table_case builds it) and
    L_v = |grad V|: a model of the table flavours with a closed-form policy."""
    import numpy as np
    axes = [np.linspace(lo, hi, n) for (lo, hi), n in zip(case["limits"], table_points)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, case["d"])
    vals = np.einsum("ij,jk,ik->i", pts, case["P"], pts)
    vals = vals * (1.0 + 0.05 * np.sin(3.0 * pts[:, 0]) * np.cos(2.0 * pts[:, -1]))
    case["V"] = {"kind": "table", "values": vals[:, None], "project": True, "num_points": list(table_points)}
    case["lv"] = ("abs_grad",)
    return case


def sum_of_products(case):
    """One kernel per output as examples/inverted_pendulum.ipynb:145-158 builds them (benchmarks.notebook_kernels
    for any number of inputs): Linear(p, ARD) + Matern32(1, active_dims=[0]) * Linear(1)."""
    import numpy as np
    prior = case["dynamics"]["prior"]
    variances = np.clip((np.hstack((case["A_true"], case["B_true"])) - prior) ** 2, 1e-5, None)
    p = prior.shape[1]
    return [[[("linear", dict(input_dim=p, variance=[float(v) for v in variances[k]], ARD=True))],
             [("matern32", dict(input_dim=1, lengthscales=1.0, active_dims=[0])),
              ("linear", dict(input_dim=1, variance=float(variances[k, 1])))]]
            for k in range(case["d"])]


def make(c):
    """The parameter dict of a ledger case (the same numbers for the engine and the oracle)."""
    import numpy as np
    import cases
    from safe_learning_amd.benchmarks import make_case, table_case
    family, kw = c["family"], dict(FAMILIES[c["family"]][3])
    if family in ("gp1d", "table1d"):
        out = gp_1d_case(c["num_points"], c["n_gp"], **kw)
    elif family == "two_actions":
        out = two_action_gp_case(c["num_points"], c["n_gp"], **kw)
    elif family == "chain3":
        out = cases.make_case_3d(num_points=c["num_points"], dynamics="gp", n_gp=c["n_gp"], **kw)
    elif family == "table":
        out = table_case(num_points=c["num_points"], table_points=TABLE_POINTS["table"], n_gp=c["n_gp"], **kw)
        del out["policy_table"]                    # closed-form policy: every cell's action has one value
    else:
        out = make_case(family, num_points=c["num_points"], n_gp=c["n_gp"], **kw)
    if family == "table1d":
        table_value(out, TABLE_POINTS["table1d"])
    if c["kernels"]:
        dyn = out["dynamics"]
        out["stack"] = True
        dyn["lengthscales"] = np.stack([np.asarray(dyn["lengthscales"], dtype=float)] * out["d"])
        dyn["kernels"] = sum_of_products(out)
    return out


def model_of(c):
    """describe(make(c)) without building the case."""
    d = len(FAMILIES[c["family"]][2])
    m = 2 if c["family"] == "two_actions" else 1
    heads = [(c["n_gp"], 1, True)] * d if c["kernels"] else [(c["n_gp"], d, False)]
    return dict(d=d, m=m, p=d + m, general=c["family"].startswith("table"), heads=heads)


# ---- sweep ranges: the launcher's own rule steers the wavefront count ------------------------------------------
# tiles per compute unit of the range: inside (0, 4], (4, 8], (8, 12], (12, 16] x num_cu, where the unrestricted
# round-cost choice is 4 / 8 / 12 / 16 wavefronts
TILES_PER_CU = {4: 3, 8: 6, 12: 10, 16: 13}


def sweep_range(c, num_cu):
    """(lo, hi) of the case's full-range sweep: the whole grid, or its last TILES_PER_CU[waves] x num_cu tiles (lo
    a multiple of 64, hi the grid's end: the last tile is ragged)."""
    n = 1
    for v in c["num_points"]:
        n *= v
    if c["waves"] is None:
        return 0, n
    tiles = -(-n // 64)
    return 64 * max(0, tiles - TILES_PER_CU[c["waves"]] * num_cu), n


def ntiles(c, num_cu):
    lo, hi = sweep_range(c, num_cu)
    return (hi - lo + 63) // 64


def compared_cells(c):
    """np_gp_truth.compared_cells by size: every cell of a grid up to 4 096 cells; of a larger one 1 024 cells drawn
    with default_rng(0) plus the first 64-cell block and the last, ragged, one."""
    import numpy as np
    n = int(np.prod(c["num_points"]))
    if n <= 4096:
        return np.arange(n)
    drawn = np.random.default_rng(0).choice(n, 1024, replace=False)
    return np.unique(np.concatenate((drawn, np.arange(64), np.arange(n - n % 64 if n % 64 else n - 64, n))))


# ---------------------------------------------------------------------------------------------
# Entries.
# ---------------------------------------------------------------------------------------------
ENTRIES = []
CFG_TESTS = "tests.test_gpu_configs::"


def _new(kernel, params, case, expect, anchor, down=None, yardstick="long double"):
    """`anchor`: True - this entry is its group's anchor (held against the extended-precision posterior and the
    oracle); else the anchor's case (same model, eight wavefronts), whose full-range sweep this entry's must equal
    bit for bit.  `down`: (switches, expected kernel family) of the kernel one step down the chain on the same
    model.  `yardstick`: 'long double' (32 x the oracle's own error) or 'oracle' (8 eps cond(K), where the
    extended-precision factorisation is too slow for a test)."""
    ENTRIES.append(dict(kind="new", kernel=kernel, params=tuple(params), case=case, expect=expect, anchor=anchor,
                        down=down, yardstick=yardstick))


def _existing(kernel, params, test, flags, env, expect):
    """`flags`: bench.py's flags of the workload that test builds, `env` the switches of the run that selects the
    instantiation; the test asserts `expect` in full."""
    ENTRIES.append(dict(kind="existing", kernel=kernel, params=tuple(params), existing=test, flags=dict(flags),
                        env=dict(env), expect=expect))


def _unreachable(kernel, params, reason, check):
    """`reason`: a statement that `check(constants)` verifies by its own arithmetic."""
    ENTRIES.append(dict(kind="unreachable", kernel=kernel, params=tuple(params), reason=reason, check=check))


# ---- the cases of tests/test_gpu_configs.py that assert a full note (on an MI355X: 256 compute units) ---------
SIXTEEN = CFG_TESTS + "test_sixteen_wavefront_workgroups_of_the_small_gp_kernel[flags%d]"
FOUR = CFG_TESTS + "test_four_wavefront_workgroups_of_the_small_gp_kernel[flags%d]"
# (test id, bench flags, switches) -> k_gp_small parameters and head count
CONFIG_CASES = [
    (SIXTEEN % 0, dict(config="C2-table-large"), {}, (1, 2, 1, 1, 16, 0), 1),
    (SIXTEEN % 0, dict(config="C2-table-large"), {"SL_GP_SMALL_WAVES": "12"}, (1, 2, 1, 1, 12, 0), 1),
    (SIXTEEN % 1, dict(config="C2-notebook"), {}, (1, 2, 1, 0, 16, 1), 2),
    (SIXTEEN % 1, dict(config="C2-notebook"), {"SL_GP_SMALL_WAVES": "12"}, (1, 2, 1, 0, 12, 1), 2),
    (SIXTEEN % 2, dict(config="C2", num_points=2048, n_gp=128), {}, (0, 2, 1, 1, 16, 0), 1),
    (SIXTEEN % 2, dict(config="C2", num_points=2048, n_gp=128), {"SL_GP_SMALL_WAVES": "12"}, (0, 2, 1, 1, 12, 0), 1),
    (SIXTEEN % 3, dict(config="C4", num_points=48, n_gp=192), {}, (0, 4, 1, 0, 16, 0), 1),
    (SIXTEEN % 3, dict(config="C4", num_points=48, n_gp=192), {"SL_GP_SMALL_WAVES": "12"}, (0, 4, 1, 0, 12, 0), 1),
    (FOUR % 0, dict(config="C2-table"), {}, (1, 2, 1, 1, 4, 0), 1),
    (FOUR % 0, dict(config="C2-table"), {"SL_GP_SMALL_WAVES": "8"}, (1, 2, 1, 1, 8, 0), 1),
    (FOUR % 1, dict(config="C2-notebook", num_points=251), {}, (1, 2, 1, 0, 4, 1), 2),
    (FOUR % 1, dict(config="C2-notebook", num_points=251), {"SL_GP_SMALL_WAVES": "8"}, (1, 2, 1, 0, 8, 1), 2),
    (FOUR % 2, dict(config="C2", num_points=128, n_gp=128), {}, (0, 2, 1, 1, 4, 0), 1),
    (FOUR % 2, dict(config="C2", num_points=128, n_gp=128), {"SL_GP_SMALL_WAVES": "8"}, (0, 2, 1, 1, 8, 0), 1),
]
MI355X_CUS = 256


def config_note(flags, cap):
    """The full kernel note of one launch of those tests: the workload of bench.py's `flags` under
    SL_GP_SMALL_WAVES = `cap` (None: unset) on an MI355X."""
    for _, known, env, params, heads in CONFIG_CASES:
        if known == flags and env.get("SL_GP_SMALL_WAVES") == cap:
            return small_note(params, heads)
    raise KeyError((flags, cap))


for _test, _flags, _env_, _params, _heads in CONFIG_CASES:
    _existing("k_gp_small", _params, _test, _flags, _env_, small_note(_params, _heads))
_EXISTING = {e["params"] for e in ENTRIES}

# ---- k_gp_small --------------------------------------------------------------------------------------------
# Training points per head (never a multiple of 16: padded rows) of family and kernel kind that put the factor
#   'lds': in LDS at every wavefront count, 'l2': in L2 at every one, 'mid': in LDS at eight, in L2 at sixteen
# (the pair the strongest comparison comes from: the same model, two placements, bit for bit).
SIZES = {
    ("gp1d", 0): dict(lds=90, mid=170, l2=210), ("gp1d", 1): dict(lds=90, mid=170, l2=210),
    ("pendulum", 0): dict(lds=90, mid=170, l2=210), ("pendulum", 1): dict(lds=40, mid=100, l2=150),
    ("chain3", 0): dict(lds=90, mid=150, l2=210), ("chain3", 1): dict(lds=40, mid=70, l2=150),
    ("cartpole", 0): dict(lds=90, mid=150, l2=210), ("cartpole", 1): dict(lds=40, mid=60, l2=100),
    ("two_actions", 0): dict(lds=90, l2=210), ("two_actions", 1): dict(lds=40, l2=150),
    ("table", 0): dict(lds=90, mid=130, l2=210), ("table", 1): dict(lds=40, mid=90, l2=150),
    ("table1d", 0): dict(lds=90, l2=210), ("table1d", 1): dict(lds=90, l2=210),
}
EIGHT = {"SL_GP_SMALL_WAVES": "8"}
# the 1-D model fails the decrease check around the origin only: its four-wavefront range (768 tiles on 256 compute
# units) is a whole grid of its own, so that the compared mask has both classes
GRID_OF = {("gp1d", 4): [49002]}


def _small_case(family, kern, size, waves):
    grid, small_grid = FAMILIES[family][1], FAMILIES[family][2]
    if grid is None:                              # a runtime-dimension flavour: eight wavefronts on any range
        return case(family, small_grid, SIZES[(family, kern)][size], kern, EIGHT)
    return case(family, GRID_OF.get((family, waves), grid), SIZES[(family, kern)][size], kern,
                EIGHT if waves == 8 else {}, waves)


for _params in sorted(instantiations()["k_gp_small"] - _EXISTING):
    _g, _d, _m, _alds, _w, _kern = _params
    _family = FAMILY_OF[(_g, _d, _m)]
    _size = "lds" if _alds else ("mid" if _w == 16 and "mid" in SIZES[(_family, _kern)] else "l2")
    _c = _small_case(_family, _kern, _size, _w)
    _heads = len(FAMILIES[_family][2]) if _kern else 1          # a stack: one head per state dimension
    _new("k_gp_small", _params, _c, small_note(_params, _heads),
         anchor=True if _w == 8 else dict(_c, env=dict(EIGHT)))

# ---- k_gp_sweep --------------------------------------------------------------------------------------------
NO_SMALL = {"SL_GP_SMALL": "0"}                 # small heads stay on k_gp_sweep's (4, 1, 1) shape
CFG3 = {"SL_GP_CFG": "3"}                       # every head on k_gp_sweep's (8, 4, 4) shape
for _s, _switch in ((0, NO_SMALL), (1, CFG3)):
    for _g, _d, _m in flavours():
        _family = FAMILY_OF[(_g, _d, _m)]
        _params = (CFG["kCfgW"][_s], CFG["kCfgR"][_s], CFG["kCfgCB"][_s], _g, _d, _m, 0)
        _new("k_gp_sweep", _params, case(_family, FAMILIES[_family][2], 90, False, _switch), sweep_note(_params),
             anchor=True, down=({}, "k_gp_small<"))
# gp_sweep_xs_global: training inputs beyond LDS (p x n_pad doubles: 2 049+ points at p = 5 or 4, 3 073+ at p = 3).
# The extended-precision factorisation of such a head takes minutes: the yardstick is the oracle under the
# 8 eps cond(K) rule of tests/test_gpu_reference_gp.py.  k_gp_sweep4 takes fast-path models of this size first
# (gp4_cfg2), so d = 4 and d = 2 are reached under SL_GP_CFG=3 only; one step down is that kernel.
XS_CASES = {4: case("cartpole", [6, 5, 5, 7], 2100, False, CFG3),
            2: case("pendulum", [44, 39], 3100, False, CFG3),
            0: case("chain3", [9, 10, 13], 2100, False, CFG3)}
for _d, _c in sorted(XS_CASES.items()):
    _params = (8, 4, 4, int(_d == 0), _d, int(_d != 0), 1)
    _new("k_gp_sweep", _params, _c, sweep_note(_params), anchor=True, down=({}, "k_gp_sweep4<"), yardstick="oracle")


def entries(kind, kernel=None):
    return [e for e in ENTRIES if e["kind"] == kind and (kernel is None or e["kernel"] == kernel)]


def entry_id(e):
    tail = "-" + case_id(e["case"]) if e["kind"] == "new" else ""
    return "%s<%s>%s" % (e["kernel"], ",".join(str(p) for p in e["params"]), tail)
