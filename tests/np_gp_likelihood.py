"""NumPy restatement of the GP log marginal likelihood and its gradient (TEST INFRASTRUCTURE): float64, and long
double built on ``np_gp_truth``'s ``ld``, ``cholesky`` and ``forward_substitution``.

With ``R = Y - m(X)``, ``K = k(X, X) + sigma_n^2 I = L L^T``, ``B = K^-1 R`` and ``W = B B^T - D K^-1``:
``lml = -1/2 sum(R o B) - D sum_i log L_ii - n D / 2 log 2 pi`` (gpflow 0.4.0 ``GPR.build_likelihood``) and
``d lml / d theta = 1/2 sum_ij W_ij dK_ij / d theta``.  The kernel is the DESCRIPTION the engine gets
(``Kern._factors``: per factor kind, product, ``variance[p]``, ``inv_lengthscales[p]``), so the float64 numbers
are the same for all parties and the long-double functions convert them exactly.

Two float64 variants (``VARIANTS``): SciPy's Cholesky and ``np_gp_sample.blocked_cholesky``.  "The restatement's
own distance" from the long-double truth is the larger of the two variants' distances, so that one lucky rounding
of a scalar does not set the bar; ``bound`` and ``distance`` are those of ``np_gp_sample`` (factor 32, a floor of
one rounding of the largest entry).

The kernels of the tests are built from ``Leaf`` records (``families``): the same record gives the description,
the natural parameters (variance, lengthscales per leaf OBJECT - one record may stand in several products) with
their chain rule, and the package's kernel object.
"""

import numpy as np
import scipy.linalg

import np_gp_sample as S
import np_gp_truth as T

LD = T.LD
RBF, MATERN32, LINEAR = 0, 1, 2
VARIANTS = ("scipy", "blocked")
LOG_2PI = np.log(2 * np.pi)


# ---- the description-level mathematics, in the precision of `X` -------------------------------------------------
def _convert(factors, dtype):
    return [(kind, product, np.asarray(v).astype(dtype), np.asarray(a).astype(dtype)) for kind, product, v, a in factors]


def factor_parts(factor, X):
    """``K_f``, ``{q: dK_f/dvariance[q]}``, ``{q: dK_f/dinv_lengthscales[q]}`` of one factor (entries that are zero
    in the description have no derivative, as in the engine)."""
    kind, _, variance, inv_ls = factor
    dtype = X.dtype.type
    n, p = X.shape
    if kind == LINEAR:
        K = np.zeros((n, n), dtype=dtype)
        dv = {}
        for q in range(p):
            if variance[q] != 0:
                dv[q] = X[:, q][:, None] * X[None, :, q]
                K = K + variance[q] * dv[q]
        return K, dv, {}
    diff2 = [np.square(X[:, q][:, None] - X[None, :, q]) for q in range(p)]
    s = np.zeros((n, n), dtype=dtype)
    for q in range(p):
        s = s + diff2[q] * (inv_ls[q] * inv_ls[q])
    v = variance[0]
    if kind == RBF:
        e = np.exp(-s / dtype(2))
        K = v * e
        da = {q: -K * diff2[q] * inv_ls[q] for q in range(p) if inv_ls[q] != 0}
        return K, ({0: e} if v != 0 else {}), da
    r = dtype(np.sqrt(3.)) * np.sqrt(s + dtype(1e-12))
    e = np.exp(-r)
    K = v * (dtype(1) + r) * e
    da = {q: -dtype(3) * v * e * diff2[q] * inv_ls[q] for q in range(p) if inv_ls[q] != 0}
    return K, ({0: (dtype(1) + r) * e} if v != 0 else {}), da


def kernel_and_derivatives(factors, X):
    """``K`` (without noise) and ``[(what, f, q, dK/dtheta)]``, ``what`` in ``('variance', 'inv_ls')``, in the
    engine's slot order."""
    parts = [factor_parts(factor, X) for factor in factors]
    n = len(X)
    K = np.zeros((n, n), dtype=X.dtype)
    for number in sorted({factor[1] for factor in factors}):
        term = np.ones((n, n), dtype=X.dtype)
        for factor, (Kf, _, _) in zip(factors, parts):
            if factor[1] == number:
                term = term * Kf
        K = K + term
    slots = []
    for f, (factor, (_, dv, da)) in enumerate(zip(factors, parts)):
        others = np.ones((n, n), dtype=X.dtype)
        for g, (other, (Kg, _, _)) in enumerate(zip(factors, parts)):
            if g != f and other[1] == factor[1]:
                others = others * Kg
        slots += [("variance", f, q, others * dv[q]) for q in sorted(dv)]
        slots += [("inv_ls", f, q, others * da[q]) for q in sorted(da)]
    return K, slots


def _tables(factors, p, slots, values, dtype):
    gv, gl = np.zeros((len(factors), p), dtype=dtype), np.zeros((len(factors), p), dtype=dtype)
    for (what, f, q, _), value in zip(slots, values):
        (gv if what == "variance" else gl)[f, q] = value
    return gv, gl


def gradient_from_w(factors, X, W):
    """Long double ``1/2 sum W o dK`` per slot for a given (float64) ``W``, and ``sum |W| |dK|`` per slot - the
    reference and the scale of the summation bound.  -> ``(gv, gl, gnoise), (av, al, anoise)``."""
    X, W = T.ld(X), T.ld(W)
    _, slots = kernel_and_derivatives(_convert(factors, LD), X)
    p = X.shape[1]
    sums = _tables(factors, p, slots, [np.sum(W * dK) / LD(2) for _, _, _, dK in slots], LD)
    scales = _tables(factors, p, slots, [np.sum(np.abs(W) * np.abs(dK)) for _, _, _, dK in slots], LD)
    return sums + (np.trace(W) / LD(2),), scales + (np.sum(np.abs(np.diag(W))),)


def summation_allowance(n, scale):
    """``2 (n^2 + 64) 2^-53 sum |W| |dK|``: the forward bound of a sum of ``n^2`` terms in any order (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2) with room for the roundings inside a term."""
    return 2.0 * (n * n + 64) * T.ROUNDING * np.asarray(scale, dtype=np.float64)


def device_w(B, Kinv):
    """``W = B B^T - D K^-1`` in float64 in the order of ``sl_lml_w``: products added with ascending ``d``, one
    rounding per operation."""
    B = np.asarray(B, dtype=np.float64)
    s = np.zeros((len(B), len(B)))
    for d in range(B.shape[1]):
        s = s + B[:, d][:, None] * B[None, :, d]
    return s - float(B.shape[1]) * np.asarray(Kinv, dtype=np.float64)


def evaluate(factors, X, R, noise, variant):
    """``variant``: ``'ld'`` (the truth), ``'scipy'`` or ``'blocked'`` -> dict with ``lml``, ``gv``, ``gl``
    (``[nfactors, p]``), ``gn``, ``B``, ``Kinv``, or ``None`` when ``K`` cannot be factored.  In long double the
    description may itself be long double (the difference quotients of natural parameters)."""
    dtype = LD if variant == "ld" else np.float64
    X, R = np.asarray(X).astype(dtype), np.asarray(R).astype(dtype)
    n, D = R.shape
    K, slots = kernel_and_derivatives(_convert(factors, dtype), X)
    K = K + dtype(noise) * np.eye(n, dtype=dtype)
    try:
        if variant == "ld":
            L = T.cholesky(K)
            Linv = T.forward_substitution(L, np.eye(n, dtype=LD))
            B = S.backward_substitution(L, T.forward_substitution(L, R))
        else:
            if variant == "scipy":
                L = scipy.linalg.cholesky(K, lower=True)
            else:
                L, info = S.blocked_cholesky(K)
                if info:
                    return None
            Linv = np.tril(scipy.linalg.solve_triangular(L, np.eye(n), lower=True))
            B = scipy.linalg.solve_triangular(L.T, scipy.linalg.solve_triangular(L, R, lower=True), lower=False)
    except np.linalg.LinAlgError:
        return None
    Kinv = Linv.T.dot(Linv)
    W = B.dot(B.T) - dtype(D) * Kinv
    lml = -np.sum(R * B) / dtype(2) - dtype(D) * np.sum(np.log(np.diag(L))) - dtype(n * D) * dtype(LOG_2PI) / dtype(2)
    gv, gl = _tables(factors, X.shape[1], slots, [np.sum(W * dK) / dtype(2) for _, _, _, dK in slots], dtype)
    return dict(lml=lml, gv=gv, gl=gl, gn=np.trace(W) / dtype(2), B=B, Kinv=Kinv)


def flat(result):
    """lml and the whole description-level gradient as one vector."""
    return np.concatenate(([result["lml"]], np.ravel(result["gv"]), np.ravel(result["gl"]), [result["gn"]]))


# ---- leaves, natural parameters, families -----------------------------------------------------------------------
class Leaf(object):
    def __init__(self, kind, input_dim, variance, lengthscales=None, active_dims=None, ARD=False):
        self.kind, self.input_dim, self.ARD = kind, input_dim, ARD
        self.active_dims = list(range(input_dim)) if active_dims is None else list(active_dims)
        self.variance = np.broadcast_to(np.asarray(variance, dtype=np.float64),
                                        (input_dim,) if kind == LINEAR else ()).copy()
        self.lengthscales = None if kind == LINEAR else np.broadcast_to(
            np.asarray(1.0 if lengthscales is None else lengthscales, dtype=np.float64), (input_dim,)).copy()


class Family(object):
    """``leaves``: the leaf objects in order of first appearance; ``products``: lists of leaf numbers; ``build``:
    the package's kernel from its leaf objects (so that a shared leaf is ONE object there too)."""

    def __init__(self, name, p, leaves, products, build):
        self.name, self.p, self.leaves, self.products, self.build = name, p, leaves, products, build

    def factors(self, precision=np.float64):
        """The description, as ``Kern._factors`` makes it (``1 / lengthscales`` in float64 - or, for the difference
        quotients of natural parameters, in long double)."""
        out = []
        for number, product in enumerate(self.products):
            for i in product:
                leaf = self.leaves[i]
                variance, inv_ls = np.zeros(self.p, dtype=precision), np.zeros(self.p, dtype=precision)
                if leaf.kind == LINEAR:
                    variance[leaf.active_dims] = leaf.variance
                else:
                    variance[0] = leaf.variance
                    inv_ls[leaf.active_dims] = precision(1) / leaf.lengthscales.astype(precision)
                out.append((leaf.kind, number, variance, inv_ls))
        return out

    def factor_leaf(self):
        return [i for product in self.products for i in product]

    def names(self):
        out = []
        for i, leaf in enumerate(self.leaves):
            out.append("kern.%d.variance" % i)
            if leaf.kind != LINEAR:
                out.append("kern.%d.lengthscales" % i)
        return out + ["likelihood_variance"]

    def natural(self, noise):
        """``{name: value}`` of the natural parameters (views of the records are not handed out)."""
        out = {}
        for i, leaf in enumerate(self.leaves):
            vector = leaf.ARD and leaf.kind == LINEAR
            out["kern.%d.variance" % i] = leaf.variance.copy() if vector else np.array(np.ravel(leaf.variance)[0])
            if leaf.kind != LINEAR:
                out["kern.%d.lengthscales" % i] = (leaf.lengthscales.copy() if leaf.ARD
                                                   else np.array(leaf.lengthscales[0]))
        out["likelihood_variance"] = np.array(float(noise))
        return out

    def natural_gradient(self, gv, gl, gn):
        """Chain rule from the description-level tables, in their precision."""
        owner = self.factor_leaf()
        out = {}
        for i, leaf in enumerate(self.leaves):
            rows = [f for f, o in enumerate(owner) if o == i]
            v = sum(gv[f] for f in rows)
            if leaf.kind == LINEAR:
                value = v[leaf.active_dims]
                out["kern.%d.variance" % i] = value if leaf.ARD else np.sum(value)
                continue
            out["kern.%d.variance" % i] = v[0]
            a = sum(gl[f] for f in rows)[leaf.active_dims]
            ell = leaf.lengthscales.astype(gl.dtype)
            value = -a / (ell * ell)
            out["kern.%d.lengthscales" % i] = value if leaf.ARD else np.sum(value)
        out["likelihood_variance"] = gn
        return out

    def package_kernel(self, sl):
        made = []
        for leaf in self.leaves:
            if leaf.kind == LINEAR:
                made.append(sl.Linear(leaf.input_dim, variance=leaf.variance if leaf.ARD else leaf.variance[0],
                                      active_dims=leaf.active_dims, ARD=leaf.ARD))
            else:
                cls = sl.RBF if leaf.kind == RBF else sl.Matern32
                made.append(cls(leaf.input_dim, variance=float(leaf.variance),
                                lengthscales=leaf.lengthscales if leaf.ARD else leaf.lengthscales[0],
                                active_dims=leaf.active_dims, ARD=leaf.ARD))
        return self.build(made)


def families():
    """Fresh records (the tests move their numbers): RBF with ARD (p = 3), Matern32 with one lengthscale (p = 2),
    the notebook's ``Linear + Matern32 * Linear`` with ``active_dims`` (p = 2), and ``(Linear + Matern32) * Linear``
    with a leaf in two products (p = 2)."""
    return [
        Family("rbf_ard", 3, [Leaf(RBF, 3, 0.5, [0.7, 1.1, 1.6], ARD=True)], [[0]], lambda k: k[0]),
        Family("matern_shared", 2, [Leaf(MATERN32, 2, 0.3, 0.8)], [[0]], lambda k: k[0]),
        Family("notebook", 2, [Leaf(LINEAR, 2, [0.04, 0.01], ARD=True), Leaf(MATERN32, 1, 0.2, 0.9, active_dims=[0]),
                               Leaf(LINEAR, 1, 0.3, active_dims=[0])], [[0], [1, 2]], lambda k: k[0] + k[1] * k[2]),
        Family("shared_leaf", 2, [Leaf(LINEAR, 2, [0.5, 0.2], ARD=True), Leaf(LINEAR, 1, 0.6, active_dims=[1]),
                                  Leaf(MATERN32, 2, 0.4, 0.7)], [[0, 1], [2, 1]], lambda k: (k[0] + k[2]) * k[1]),
    ]


FAMILY_NAMES = [fam.name for fam in families()]


def family(name):
    return [fam for fam in families() if fam.name == name][0]


def data(fam, n, D, with_mean, seed=3):
    """``X [n, p]``, ``Y [n, D]``, the prior matrix ``[D, p]`` or ``None``: smooth functions of the inputs plus
    noise of standard deviation 0.05."""
    rng = np.random.default_rng(seed + 7 * n + D)
    X = rng.uniform(-1, 1, (n, fam.p))
    M = rng.uniform(-0.5, 0.5, (D, fam.p))
    Y = np.stack([np.sin(2.0 * X[:, 0] + d) * (1.0 + 0.5 * X[:, -1]) for d in range(D)], axis=1)
    Y = Y + X.dot(M.T) + 0.05 * rng.standard_normal((n, D))
    return X, Y, (M if with_mean else None)


def residuals(X, Y, M):
    return Y if M is None else Y - X.dot(M.T)


def package_model(sl, fam, X, Y, M, noise):
    mean = None if M is None else sl.LinearSystem((np.array(M),))
    return sl.GPRCached(X, Y, fam.package_kernel(sl), mean, likelihood_variance=noise)
