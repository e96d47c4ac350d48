"""Function objects of the Lyapunov sweep as declarative specs for the HIP engine.

The reference composes TensorFlow callables (``safe_learning/functions.py``); a GPU kernel
cannot call back into Python, so here every class is a small parameter record with the
reference's constructor signature that knows how to write itself into the C-ABI model
description (``include/sl_hip.h``).  All arithmetic happens in the HIP kernels; this module
only prepares host-side metadata (grids, Cholesky factors, unit-cell triangulations), which
is also host-side NumPy/SciPy work in the reference.

Reference classes mirrored (constructor arguments keep their names):
``GridWorld`` (functions.py:579-817), ``QuadraticFunction`` (:1513-1543), ``LinearSystem``
(:1546-1583), ``Saturation`` (:310-354), ``GPRCached`` (:357-458), ``GaussianProcess``
(:461-546), ``FunctionStack`` (:254-307), ``Triangulation`` (:981-1510) and, from
``examples/utilities.py``, ``InvertedPendulum`` (:144-289), ``CartPole`` (:292-437),
``LyapunovNetwork`` (:48-104).
"""

from itertools import product as _cartesian

import numpy as np
import scipy.linalg
import scipy.signal
from scipy import spatial

import itertools

from . import _hip
from .configuration import config
from .unit_cells import UNIT_CELL_SIMPLICES


def qhull_unit_cell(unit_maxes):
    """The unit-cell triangulation as the reference computes it (``functions.py:1019-1023``):
    ``spatial.Delaunay`` of ``cartesian(*np.diag(unit_maxes))`` (3^d rows with duplicates for
    d >= 3), as corner codes (bit k = coordinate k at ``unit_maxes[k]``)."""
    unit_maxes = np.asarray(unit_maxes, dtype=config.np_dtype)
    d = len(unit_maxes)
    corners = np.array(list(_cartesian(*np.diag(unit_maxes))), dtype=config.np_dtype)
    tri = spatial.Delaunay(corners)
    codes = ((corners > 0).astype(np.int64) << np.arange(d)).sum(axis=1)
    return codes[tri.simplices].astype(np.int32)

# Upload caches (``_model.ModelBuilder``) are keyed on these process-wide, never reused tokens:
# ``id()`` values can be recycled by CPython once an object is collected.
_TOKENS = itertools.count(1)

__all__ = ['GridWorld', 'DimensionError', 'DeterministicFunction', 'UncertainFunction',
           'QuadraticFunction', 'LinearSystem', 'Saturation', 'AbsFunction', 'Norm1Function',
           'AbsGradient', 'Gradient', 'ConstantFunction', 'RBF', 'Matern32', 'Linear', 'GPRCached', 'GaussianProcess',
           'FunctionStack', 'GPMeanFunction', 'Triangulation', 'InvertedPendulum', 'CartPole', 'PolynomialSystem', 'VanDerPol',
           'PolynomialFunction', 'monomial_exponents', 'LyapunovNetwork',
           'NeuralNetwork', 'sample_gp_function', 'GPSampleFunction']


class DimensionError(Exception):
    """Same role as ``safe_learning/functions.py:575-576``."""


# ----------------------------------------------------------------------------------------------
# grid
# ----------------------------------------------------------------------------------------------

class GridWorld(object):
    """Regular grid over a hyper-rectangle (reference: ``functions.py:591-620``).

    ``limits`` is ``[(lo, hi), ...]``, ``num_points`` an int or one int per dimension.  Flat
    indices are C-order (last dimension fastest); state ``k`` of index ``ijk`` is
    ``ijk[k] * unit_maxes[k] + offset[k]`` - the addressing contract of the HIP kernels.
    """

    def __init__(self, limits, num_points):
        dtype = config.np_dtype
        self.limits = np.atleast_2d(limits).astype(dtype)
        self.ndim = len(self.limits)
        self.num_points = np.broadcast_to(num_points, self.ndim).astype(np.int64)
        if np.any(self.num_points < 2):
            raise DimensionError('There must be at least 2 points in each dimension.')
        lower, upper = self.limits[:, 0], self.limits[:, 1]
        self.offset = lower
        self.unit_maxes = ((upper - lower) / (self.num_points - 1)).astype(dtype)
        self.offset_limits = np.stack((np.zeros_like(lower), upper - lower), axis=1)
        self.discrete_points = [np.linspace(lo, hi, n, dtype=dtype)
                                for (lo, hi), n in zip(self.limits, self.num_points)]
        self.nrectangles = int(np.prod(self.num_points - 1))
        self.nindex = int(np.prod(self.num_points))
        self._all_points = None

    def __len__(self):
        return self.nindex

    @property
    def all_points(self):
        """``[nindex, ndim]`` array of every grid point (``functions.py:622-638``).

        Only for small grids / plotting: the kernels generate states from indices instead."""
        if self._all_points is None:
            mesh = np.meshgrid(*self.discrete_points, indexing='ij')
            self._all_points = np.stack([m.ravel() for m in mesh], axis=1).astype(config.np_dtype)
        return self._all_points

    def sample_continuous(self, num_samples):
        """Uniform samples from the continuous domain (``functions.py:644-659``)."""
        rand = np.random.uniform(0, 1, size=(num_samples, self.ndim))
        return rand * np.diff(self.limits, axis=1).T + self.offset

    def sample_discrete(self, num_samples, replace=False):
        """Uniform samples from the grid points (``functions.py:661-677``)."""
        idx = np.random.choice(self.nindex, size=num_samples, replace=replace)
        return self.index_to_state(idx)

    def _check_dimensions(self, states):
        if not states.shape[1] == self.ndim:
            raise DimensionError('the input argument has the wrong dimensions.')

    def _center_states(self, states, clip=True):
        """States relative to the lower corner, optionally clipped 2 eps inside
        (``functions.py:691-712``)."""
        eps = np.finfo(config.np_dtype).eps
        states = np.atleast_2d(states).astype(config.np_dtype) - self.offset[None, :]
        if clip:
            np.clip(states, self.offset_limits[:, 0] + 2 * eps,
                    self.offset_limits[:, 1] - 2 * eps, out=states)
        return states

    def index_to_state(self, indices):
        """Flat indices -> states (``functions.py:714-731``)."""
        ijk = np.stack(np.unravel_index(np.atleast_1d(indices), self.num_points), axis=1)
        return ijk.astype(config.np_dtype) * self.unit_maxes + self.offset

    def state_to_index(self, states):
        """Nearest grid point of each state, clipped to the domain (``functions.py:733-752``)."""
        states = np.atleast_2d(states)
        self._check_dimensions(states)
        clipped = np.clip(states, self.limits[:, 0], self.limits[:, 1])
        ijk = np.rint((clipped - self.offset) * (1. / self.unit_maxes)).astype(np.int32)
        return np.ravel_multi_index(ijk.T, self.num_points)

    def state_to_rectangle(self, states):
        """Index of the grid cell containing each state (``functions.py:754-776``)."""
        cells = []
        for k in range(self.ndim):
            idx = np.digitize(states[:, k], self.discrete_points[k]) - 1
            cells.append(np.clip(idx, 0, self.num_points[k] - 2))
        return np.ravel_multi_index(cells, self.num_points - 1)

    def rectangle_to_state(self, rectangles):
        """Lower-left corner state of each cell (``functions.py:778-798``)."""
        ijk = np.stack(np.unravel_index(np.atleast_1d(rectangles), self.num_points - 1), axis=1)
        return ijk.astype(config.np_dtype) * self.unit_maxes + self.offset

    def rectangle_corner_index(self, rectangles):
        """Flat grid index of each cell's lower-left corner (``functions.py:800-817``)."""
        ijk = np.unravel_index(rectangles, self.num_points - 1)
        return np.ravel_multi_index(np.atleast_2d(ijk), self.num_points)

    # ---- C-ABI view ------------------------------------------------------------------------
    def _desc(self):
        if self.ndim > _hip.MAX_STATE_DIM:
            raise DimensionError('the HIP engine supports at most %d state dimensions'
                                 % _hip.MAX_STATE_DIM)
        g = _hip.GridDesc()
        g.d = self.ndim
        for k in range(self.ndim):
            g.num_points[k] = int(self.num_points[k])
            g.offset[k] = float(self.offset[k])
            g.unit_maxes[k] = float(self.unit_maxes[k])
            g.upper[k] = float(self.limits[k, 1])
        return g


# ----------------------------------------------------------------------------------------------
# spec base classes
# ----------------------------------------------------------------------------------------------

class Function(object):
    """Base of all specs.  ``-f`` is supported as a sign flag (``functions.py:120-122``)."""

    negate = False

    def __neg__(self):
        import copy
        other = copy.copy(self)
        other.negate = not self.negate
        return other

    _role = None      # 'value', 'policy', 'dynamics' or 'linear'

    def __call__(self, *points):
        """Evaluate at explicit points on the GPU (``functions.py:63-82``); several inputs are
        concatenated like ``concatenate_inputs`` does (``utilities.py:123-159``)."""
        from . import _evaluate
        arrays = [np.atleast_2d(np.asarray(p, dtype=config.np_dtype)) for p in points]
        if self._role == 'value':
            out = _evaluate.value(self, np.hstack(arrays))
            return out
        if self._role == 'policy':
            return _evaluate.policy(self, np.hstack(arrays))
        if self._role == 'dynamics':
            joined = np.hstack(arrays)
            d = self.output_dim
            return _evaluate.dynamics(self, joined[:, :d], joined[:, d:])
        if self._role == 'linear':
            joined = np.hstack(arrays)
            if len(arrays) == 2 and self.matrix.shape[0] == arrays[0].shape[1]:
                return _evaluate.dynamics(self, arrays[0], arrays[1])
            if self.matrix.shape[0] <= _hip.MAX_ACTION_DIM and len(arrays) == 1:
                return _evaluate.policy(self, joined)
            return _evaluate.linear_map(self, joined)
        raise NotImplementedError('%s cannot be evaluated on its own' % type(self).__name__)


class DeterministicFunction(Function):
    """Marker base class (``functions.py:233-238``)."""


class UncertainFunction(Function):
    """Marker base class: evaluation yields ``(mean, error_bound)`` (``functions.py:202-230``)."""


def _hstack_matrices(matrices):
    if isinstance(matrices, np.ndarray):
        matrices = (matrices,)
    return np.hstack([np.atleast_2d(m).astype(config.np_dtype) for m in matrices])


class QuadraticFunction(DeterministicFunction):
    """``x P x^T`` (``functions.py:1513-1543``); ``P`` need not be symmetric."""

    _role = 'value'

    def __init__(self, matrix, name='quadratic'):
        self.matrix = np.atleast_2d(matrix).astype(config.np_dtype)
        self.ndim = self.matrix.shape[0]
        self.name = name

    def gradient_function(self):
        """``LinearSystem`` computing ``x (P + P^T)`` (``functions.py:1541-1543``)."""
        return LinearSystem((self.matrix + self.matrix.T,))

    def _write_value(self, desc):
        n = self.ndim
        if n > _hip.MAX_INPUT_DIM:
            raise DimensionError('quadratic form too large for the HIP engine')
        desc.kind = _hip.V_QUADRATIC
        desc.negate = int(self.negate)
        for i in range(n):
            for j in range(n):
                desc.matrix[i][j] = float(self.matrix[i, j])


class LinearSystem(DeterministicFunction):
    """``[x, u] M^T`` with ``M = hstack(matrices)`` (``functions.py:1546-1583``)."""

    _role = 'linear'

    def __init__(self, matrices, name='linear_system'):
        self.matrix = _hstack_matrices(matrices)
        self.output_dim, self.input_dim = self.matrix.shape
        self.name = name


class Saturation(DeterministicFunction):
    """Clamp ``fun`` to ``[lower, upper]`` (``functions.py:310-354``)."""

    _role = 'policy'

    def __init__(self, fun, lower, upper, name='saturation'):
        self.fun, self.lower, self.upper = fun, lower, upper
        self.input_dim = getattr(fun, 'input_dim', None)
        self.output_dim = getattr(fun, 'output_dim', None)
        self.name = name


class ConstantFunction(DeterministicFunction):
    """The same output row for every input (``functions.py:241-251``)."""

    def __init__(self, constant, name='constant_function'):
        self.constant = np.atleast_1d(np.asarray(constant, dtype=config.np_dtype))
        self.output_dim = len(self.constant)
        self.name = name


class AbsFunction(DeterministicFunction):
    """``|fun(x)|`` - replaces ``lambda x: tf.abs(grad(x))`` of the notebooks."""

    def __init__(self, fun):
        self.fun = fun


class Norm1Function(DeterministicFunction):
    """``||fun(x)||_1`` - replaces ``lambda x: tf.norm(grad(x), ord=1, axis=1, keepdims=True)``.

    ``constant + Norm1Function(LinearSystem(M))`` gives the affine form ``c + ||M x||_1`` that the
    engine accepts as a state-dependent ``lipschitz_dynamics`` (``lyapunov.py:227-244``)."""

    def __init__(self, fun, constant=0.0):
        self.fun = fun
        self.constant = float(constant)

    def __add__(self, constant):
        if not np.isscalar(constant):
            return NotImplemented
        return Norm1Function(self.fun, self.constant + float(constant))

    __radd__ = __add__


class Gradient(DeterministicFunction):
    """``dV/dx`` of a table / network value function: ``tri.gradient`` (``functions.py:1302-1326``)
    or ``tf.gradients(V(x), x)`` of the notebooks.  Use inside ``AbsFunction`` / ``Norm1Function``
    as the local Lipschitz constant ``L_v``."""

    def __init__(self, fun):
        self.fun = fun


def AbsGradient(fun):
    """``|dV/dx|`` per dimension (``inverted_pendulum.ipynb`` cell 14)."""
    return AbsFunction(Gradient(fun))


# ----------------------------------------------------------------------------------------------
# Gaussian process
# ----------------------------------------------------------------------------------------------

class Kern(object):
    """Kernels with the gpflow 0.4.0 ``kernels.py`` surface the reference relies on: ``K(X, X2)``,
    ``Kdiag(X)`` (``functions.py:401, 438, 445, 450``), ``active_dims``, ``+`` and ``*``
    (``examples/inverted_pendulum.ipynb:152-158``: ``Linear + Matern32 * Linear``).  The Gram
    matrix of the training set is formed here on the host; the engine evaluates ``k(X, x)`` and
    ``k(x, x)`` of the grid cells from :meth:`_factors`."""

    def __init__(self, input_dim, active_dims=None):
        self.input_dim = int(input_dim)
        if active_dims is None:
            active_dims = range(self.input_dim)          # gpflow: slice(input_dim)
        self.active_dims = np.asarray(list(active_dims), dtype=np.int64)
        if len(self.active_dims) != self.input_dim:
            raise ValueError('active_dims has %d entries, input_dim is %d'
                             % (len(self.active_dims), self.input_dim))

    def _slice(self, X, X2):
        X = np.asarray(X, dtype=config.np_dtype)[:, self.active_dims]
        X2 = X if X2 is None else np.asarray(X2, dtype=config.np_dtype)[:, self.active_dims]
        return X, X2

    def __add__(self, other):
        return Add([self, other])

    def __mul__(self, other):
        return Prod([self, other])

    def _products(self):
        """The kernel as a sum of products of leaves: ``[[leaf, ...], ...]``."""
        return [[self]]

    def _factors(self, p):
        """``[(kind, product, variance[p], inv_lengthscales[p])]`` for ``sl_gp_set_head_kernel``."""
        out = []
        for number, product in enumerate(self._products()):
            for leaf in product:
                variance, inv_ls = np.zeros(p), np.zeros(p)
                if leaf.active_dims.max() >= p:
                    raise ValueError('kernel reads input column %d of %d' % (leaf.active_dims.max(), p))
                leaf._fill(variance, inv_ls)
                out.append((leaf._kind, number, variance, inv_ls))
        return out


class _Stationary(Kern):
    def __init__(self, input_dim, variance=1.0, lengthscales=None, active_dims=None, ARD=False):
        Kern.__init__(self, input_dim, active_dims)
        self.variance = float(variance)
        if lengthscales is None:
            lengthscales = 1.0
        self.lengthscales = np.broadcast_to(np.asarray(lengthscales, dtype=config.np_dtype),
                                            (self.input_dim,)).copy()
        self.ARD = bool(ARD)

    def _square_dist(self, X, X2):
        X, X2 = self._slice(X, X2)
        diff = X[:, None, :] / self.lengthscales - X2[None, :, :] / self.lengthscales
        return np.einsum('ijk,ijk->ij', diff, diff)

    def Kdiag(self, X):
        return np.full(len(X), self.variance, dtype=config.np_dtype)

    def _fill(self, variance, inv_ls):
        variance[0] = self.variance
        inv_ls[self.active_dims] = 1.0 / self.lengthscales


class RBF(_Stationary):
    """Squared-exponential kernel with the gpflow 0.4.0 ``kernels.RBF`` signature:
    ``k(x, x') = variance * exp(-0.5 * sum_q ((x_q - x'_q) / lengthscales_q)^2)``."""

    _kind = _hip.KERNEL_RBF

    def __init__(self, input_dim, variance=1.0, lengthscales=None, active_dims=None, ARD=False):
        _Stationary.__init__(self, input_dim, variance, lengthscales, active_dims, ARD)

    def K(self, X, X2=None):
        """Gram matrix on the host (training-set side only)."""
        return self.variance * np.exp(-0.5 * self._square_dist(X, X2))


class Matern32(_Stationary):
    """``variance * (1 + sqrt(3) r) * exp(-sqrt(3) r)`` with gpflow 0.4.0's
    ``r = sqrt(square_dist + 1e-12)`` (``Stationary.euclid_dist``)."""

    _kind = _hip.KERNEL_MATERN32

    def K(self, X, X2=None):
        r = np.sqrt(3.0) * np.sqrt(self._square_dist(X, X2) + 1e-12)
        return self.variance * (1.0 + r) * np.exp(-r)


class Linear(Kern):
    """``k(x, x') = sum_q variance_q x_q x'_q`` (gpflow 0.4.0 ``kernels.Linear``; one variance
    for all dimensions unless ``ARD``)."""

    _kind = _hip.KERNEL_LINEAR

    def __init__(self, input_dim, variance=1.0, active_dims=None, ARD=False):
        Kern.__init__(self, input_dim, active_dims)
        self.ARD = bool(ARD)
        self.variance = np.broadcast_to(np.asarray(variance, dtype=config.np_dtype),
                                        (self.input_dim,)).copy()

    def K(self, X, X2=None):
        X, X2 = self._slice(X, X2)
        return (X * self.variance).dot(X2.T)

    def Kdiag(self, X):
        X, _ = self._slice(X, None)
        return np.sum(np.square(X) * self.variance, axis=1)

    def _fill(self, variance, inv_ls):
        variance[self.active_dims] = self.variance


class _Combination(Kern):
    def __init__(self, kern_list):
        self.kern_list = []
        for kern in kern_list:
            if not isinstance(kern, Kern):
                raise TypeError('can only combine Kern instances')
            # gpflow flattens nested combinations of the same kind
            self.kern_list.extend(kern.kern_list if type(kern) is type(self) else [kern])
        Kern.__init__(self, max(k.input_dim for k in self.kern_list))


class Add(_Combination):
    def K(self, X, X2=None):
        return sum(k.K(X, X2) for k in self.kern_list)

    def Kdiag(self, X):
        return sum(k.Kdiag(X) for k in self.kern_list)

    def _products(self):
        return [product for k in self.kern_list for product in k._products()]


class Prod(_Combination):
    def K(self, X, X2=None):
        out = self.kern_list[0].K(X, X2)
        for k in self.kern_list[1:]:
            out = out * k.K(X, X2)
        return out

    def Kdiag(self, X):
        out = self.kern_list[0].Kdiag(X)
        for k in self.kern_list[1:]:
            out = out * k.Kdiag(X)
        return out

    def _products(self):
        products = [[]]
        for k in self.kern_list:                       # (a + b) * c = a c + b c
            products = [left + right for left in products for right in k._products()]
        return products


def _is_plain_rbf(kern, p):
    """The kernel of ``sl_gp_set_head`` (and of the MFMA paths that generate RBF values by
    recurrence): an RBF over all ``p`` inputs in their order."""
    return (type(kern) is RBF and kern.input_dim == p
            and np.array_equal(kern.active_dims, np.arange(p)))


class GPRCached(object):
    """GP regression model whose Cholesky data is cached for prediction
    (``functions.py:357-458``).  ``kern`` is a :class:`Kern`; ``mean_function`` a
    :class:`LinearSystem` (or ``None`` for zero mean); ``likelihood_variance`` is gpflow's
    ``likelihood.variance`` (default 1.0, the notebooks overwrite it).  ``scale`` is accepted for
    signature compatibility; it cancels analytically in ``build_predict`` and is not used."""

    def __init__(self, x, y, kern, mean_function=None, scale=1., name='GPRCached',
                 likelihood_variance=1.0):
        self.X = np.atleast_2d(np.asarray(x, dtype=config.np_dtype))
        self.Y = np.atleast_2d(np.asarray(y, dtype=config.np_dtype))
        if not isinstance(kern, Kern):
            raise TypeError('kern must be an RBF, Matern32 or Linear kernel or a sum / product of those')
        if mean_function is not None and not isinstance(mean_function, LinearSystem):
            raise TypeError('mean_function must be a LinearSystem or None')
        self.kern = kern
        self.mean_function = mean_function
        self._scale = float(scale)
        self.likelihood_variance = float(likelihood_variance)
        self.name = name
        self.update_cache()

    def update_cache(self):
        """Cholesky factor, its inverse and ``alpha = L^-1 (Y - m(X))`` (``functions.py:395-415``)."""
        n = len(self.X)
        gram = self.kern.K(self.X) + self.likelihood_variance * np.eye(n)
        self.cholesky = scipy.linalg.cholesky(gram, lower=True) if n else np.zeros((0, 0))
        resid = self.Y.copy()
        if self.mean_function is not None:
            resid = resid - self.X.dot(self.mean_function.matrix.T)
        if n == 0:                                      # no observations yet: the prior
            self.alpha, self.cholesky_inverse = np.zeros_like(resid), np.zeros((0, 0))
        else:
            self.alpha = scipy.linalg.solve_triangular(self.cholesky, resid, lower=True)
            self.cholesky_inverse = scipy.linalg.solve_triangular(self.cholesky, np.eye(n), lower=True)
            self.cholesky_inverse = np.tril(self.cholesky_inverse)
        self._version = next(_TOKENS)
        self._append_log = []          # rank-one extensions since the last full rebuild

    def append_data(self, x, y):
        """Add observations with a rank-one extension of the cached factors, O(n^2) per point
        instead of the reference's O(n^3) rebuild (``functions.py:525-546`` calls
        ``update_cache``).  For ``L' = [[L, 0], [l^T, s]]``: ``l = L^-1 k(X, x)``,
        ``s = sqrt(k(x, x) + sigma_n^2 - l.l)``, ``L'^-1 = [[L^-1, 0], [-(l^T L^-1)/s, 1/s]]`` and
        ``alpha' = [alpha; (r - l^T alpha)/s]`` with ``r = y - m(x)``."""
        x = np.atleast_2d(np.asarray(x, dtype=config.np_dtype))
        y = np.atleast_2d(np.asarray(y, dtype=config.np_dtype))
        for xi, yi in zip(x, y):
            xi, yi = xi[None, :], yi[None, :]
            n = len(self.X)
            k_vec = self.kern.K(self.X, xi)[:, 0]
            row = self.cholesky_inverse.dot(k_vec)                       # l = L^-1 k
            # K(x, x) as the rebuild of functions.py:401 forms it (kern.K, not kern.Kdiag: the
            # two differ by 1.5e-12 for a Matern32 leaf, whose distance carries euclid_dist's 1e-12)
            s2 = self.kern.K(xi)[0, 0] + self.likelihood_variance - row.dot(row)
            if not s2 > 0:
                raise np.linalg.LinAlgError('kernel matrix is not positive definite')
            s = np.sqrt(s2)
            resid = yi[0] - (xi.dot(self.mean_function.matrix.T)[0]
                             if self.mean_function is not None else 0.0)
            chol = np.zeros((n + 1, n + 1))
            chol[:n, :n], chol[n, :n], chol[n, n] = self.cholesky, row, s
            inv = np.zeros((n + 1, n + 1))
            inv[:n, :n] = self.cholesky_inverse
            inv[n, :n] = -row.dot(self.cholesky_inverse) / s
            inv[n, n] = 1.0 / s
            self.alpha = np.vstack((self.alpha, ((resid - row.dot(self.alpha)) / s)[None, :]))
            self.cholesky, self.cholesky_inverse = chol, inv
            self.X = np.vstack((self.X, xi))
            self.Y = np.vstack((self.Y, yi))
            # what the engine needs to follow without re-packing L^-1: the new row and alpha row
            before, self._version = self._version, next(_TOKENS)
            self._append_log.append((before, self._version, xi[0].copy(), inv[n, :n + 1].copy(),
                                     self.alpha[n].copy()))


def _likelihood_engine(X, R, factors, noise_variance, gradient):
    """One ``sl_gp_likelihood`` call (``Context.gp_likelihood``): the only way the hyper-parameter methods of
    :class:`GPRCached` reach the engine."""
    from . import _evaluate
    return _evaluate._ctx().gp_likelihood(X, R, factors, noise_variance, gradient)


class _Hyperparameters(object):
    """The free numbers of a :class:`GPRCached` by name, and the chain rule from the engine's derivatives (with
    respect to ``variance[q]`` / ``inv_lengthscales[q]`` of every factor of ``Kern._factors``) to them."""

    def __init__(self, model):
        self.model = model
        self.leaves, self.factor_leaf = [], []
        for product in model.kern._products():
            for leaf in product:
                if not any(leaf is known for known in self.leaves):
                    self.leaves.append(leaf)
                self.factor_leaf.append([leaf is known for known in self.leaves].index(True))
        self.entries = []                                  # (name, owner, attribute)
        for number, leaf in enumerate(self.leaves):
            self.entries.append(('kern.%d.variance' % number, leaf, 'variance'))
            if isinstance(leaf, _Stationary):
                self.entries.append(('kern.%d.lengthscales' % number, leaf, 'lengthscales'))
        self.entries.append(('likelihood_variance', model, 'likelihood_variance'))
        self.names = [name for name, _, _ in self.entries]

    @staticmethod
    def _is_vector(owner, attribute):
        return isinstance(owner, Kern) and owner.ARD and (attribute == 'lengthscales' or isinstance(owner, Linear))

    def is_vector(self, name):
        return any(self._is_vector(owner, attribute) for known, owner, attribute in self.entries if known == name)

    def get(self):
        out = []
        for name, owner, attribute in self.entries:
            value = np.asarray(getattr(owner, attribute), dtype=config.np_dtype)
            out.append((name, value.copy() if self._is_vector(owner, attribute) else value.reshape(-1)[0]))
        return out

    def set(self, values):
        """``{name: value}`` into the kernel objects and the model (no ``update_cache``)."""
        for name, owner, attribute in self.entries:
            if name not in values:
                continue
            value = np.asarray(values[name], dtype=config.np_dtype)
            current = getattr(owner, attribute)
            if isinstance(current, np.ndarray):
                current[:] = value
            else:
                setattr(owner, attribute, float(value))

    def natural_gradient(self, grad_variance, grad_inv_ls, grad_noise):
        """``{name: ndarray}`` from the engine's ``[nfactors, p]`` tables: ``d/dl_q = -a_q^2 d/da_q``, a leaf
        without ``ARD`` sums over its dimensions, a leaf in several products sums over its factors."""
        out = {}
        for number, leaf in enumerate(self.leaves):
            dims = leaf.active_dims
            gv = sum(grad_variance[f] for f, owner in enumerate(self.factor_leaf) if owner == number)
            if isinstance(leaf, Linear):
                value = gv[dims]
                out['kern.%d.variance' % number] = value.copy() if leaf.ARD else np.array(value.sum())
                continue
            out['kern.%d.variance' % number] = np.array(gv[0])
            gl = sum(grad_inv_ls[f] for f, owner in enumerate(self.factor_leaf) if owner == number)
            value = -gl[dims] / np.square(leaf.lengthscales)
            out['kern.%d.lengthscales' % number] = value if leaf.ARD else np.array(value.sum())
        out['likelihood_variance'] = np.array(grad_noise)
        return out


def _gpr_hyperparameters(self):
    """The hyper-parameters in order, ``[(name, value)]``: per leaf kernel object, in the order of its first
    appearance in ``kern._products()``, ``kern.<i>.variance`` and (RBF, Matern32) ``kern.<i>.lengthscales``, then
    ``likelihood_variance``.  Lengthscales, and the variance of a ``Linear`` leaf, are a vector for ``ARD=True``
    and one scalar otherwise."""
    return _Hyperparameters(self).get()


def _gpr_likelihood(self, gradient):
    from . import distributed as dist_utils
    if dist_utils.rank_and_world()[1] > 1:
        raise NotImplementedError('the GP marginal likelihood runs on one GPU; under torch.distributed fit on one '
                                  'rank and broadcast the hyper-parameters')
    n, p = self.X.shape
    if n > _hip.Context.GP_LIKELIHOOD_MAX_TRAIN:
        raise ValueError('the GP marginal likelihood takes at most %d observations, the model has %d'
                         % (_hip.Context.GP_LIKELIHOOD_MAX_TRAIN, n))
    resid = self.Y if self.mean_function is None else self.Y - self.X.dot(self.mean_function.matrix.T)
    return _likelihood_engine(self.X, resid, self.kern._factors(p), self.likelihood_variance, gradient)


def _gpr_not_factored(pivot, n):
    return np.linalg.LinAlgError('the kernel matrix of the %d observations plus the noise variance is not positive '
                                 'definite: pivot %d is not positive' % (n, pivot))


def _gpr_compute_log_likelihood(self):
    """Log marginal likelihood of the observations (gpflow 0.4.0 ``GPR.build_likelihood``), on the GPU:
    ``-1/2 sum_d r_d^T K^-1 r_d - D sum_i log L_ii - n D / 2 log 2 pi`` with ``K = k(X, X) + sigma_n^2 I = L L^T``
    and ``R = Y - m(X)``.  ``np.linalg.LinAlgError`` (naming the pivot) when ``K`` cannot be factored."""
    lml, _, _, _, pivot = _gpr_likelihood(self, False)
    if pivot:
        raise _gpr_not_factored(pivot, len(self.X))
    return lml


def _gpr_log_likelihood_gradient(self):
    """``{name: ndarray}``: the derivative of :meth:`compute_log_likelihood` with respect to every entry of
    :meth:`hyperparameters` (variances, lengthscales, ``likelihood_variance`` - the natural parameters)."""
    _, gv, gl, gn, pivot = _gpr_likelihood(self, True)
    if pivot:
        raise _gpr_not_factored(pivot, len(self.X))
    return _Hyperparameters(self).natural_gradient(gv, gl, gn)


def _gpr_optimize(self, method='L-BFGS-B', maxiter=1000, tol=None, fixed=(), bounds=None, callback=None, **options):
    """Fit the hyper-parameters: minimise ``-log marginal likelihood`` over the LOGARITHMS of the free parameters
    with ``scipy.optimize.minimize(jac=True)`` (signature after gpflow 0.4.0's ``Model.optimize``); every
    evaluation of the objective is one ``sl_gp_likelihood`` call on the GPU.  gpflow searches through a softplus
    transform instead of the logarithm, so its iterates differ from these; the optimum does not.

    ``fixed``: names (:meth:`hyperparameters`) that keep their value.  ``bounds``: ``{name: (lo, hi)}`` in natural
    units (``None`` for an open end).  A parameter vector whose kernel matrix cannot be factored is a rejected
    point (objective ``+inf``, gradient zeros).  A search that met one is not trusted to have converged (``L-BFGS-B``
    reads the zero gradient as convergence, or stops one evaluation later): it is taken up again from the best
    point seen, with the iterations that are left, as long as that raises the likelihood, so the search that ends
    the call met no rejected point.  Otherwise the result has ``success = False`` and says so in ``message``;
    ``result.rejected`` counts the rejected points.  A model that
    cannot be factored at the start raises ``np.linalg.LinAlgError`` naming the pivot and is left as it was.
    Otherwise the best point seen is assigned to the kernel objects and ``likelihood_variance`` at the end and
    ``update_cache()`` is called once, so every engine follows.  Returns the ``scipy.optimize.OptimizeResult``
    (``x`` in logarithms, ``fun`` the negative log likelihood; both of the best point)."""
    import scipy.optimize
    table = _Hyperparameters(self)
    unknown = [name for name in list(fixed) + list(bounds or {}) if name not in table.names]
    if unknown:
        raise ValueError('optimize: unknown hyper-parameter(s) %s; the model has %s' % (unknown, table.names))
    free = [(name, np.atleast_1d(value)) for name, value in table.get() if name not in set(fixed)]
    if not free:
        raise ValueError('optimize: every hyper-parameter is fixed')
    for name, value in free:
        if not np.all(value > 0):
            raise ValueError('optimize searches over logarithms: %s = %s is not positive' % (name, value))
    sizes = [len(value) for _, value in free]
    x0 = np.log(np.concatenate([value for _, value in free]))
    box = None
    if bounds:
        box = []
        for name, value in free:
            lo, hi = bounds.get(name, (None, None))
            box += [(None if lo is None else np.log(lo), None if hi is None else np.log(hi))] * len(value)

    def assign(x):
        parts = np.split(np.exp(x), np.cumsum(sizes)[:-1])
        table.set({name: part if table.is_vector(name) else part[0] for (name, _), part in zip(free, parts)})

    best = {'fun': np.inf, 'x': x0.copy()}
    state = {'accepted': False, 'search_rejected': False, 'rejected': 0}

    def objective(x):
        assign(x)
        lml, gv, gl, gn, pivot = _gpr_likelihood(self, True)
        if pivot or not np.isfinite(lml):
            if not state['accepted']:
                assign(x0)
                raise _gpr_not_factored(pivot, len(self.X))
            state['search_rejected'] = True
            state['rejected'] += 1
            return np.inf, np.zeros_like(x)
        state['accepted'] = True
        natural = table.natural_gradient(gv, gl, gn)
        grad = np.concatenate([np.atleast_1d(natural[name]) for name, _ in free]) * np.exp(x)
        if -lml < best['fun']:
            best['fun'], best['x'] = -lml, np.array(x, copy=True)
        return -lml, -grad

    # A search that met a rejected point cannot be trusted to have converged: L-BFGS-B reads the zero gradient as
    # convergence, or stops one evaluation later on a small relative reduction.  Such a search is taken up again from
    # the best point seen, with the iterations that are left, as long as that raises the likelihood; the search that
    # ends the call met no rejected point, or it is reported as not successful.
    start, remaining, searches = x0, int(maxiter), 0
    try:
        while True:
            before, state['search_rejected'] = best['fun'], False
            result = scipy.optimize.minimize(objective, start, jac=True, method=method, tol=tol, bounds=box,
                                             callback=callback, options=dict(options, maxiter=remaining))
            searches += 1
            remaining -= max(int(getattr(result, 'nit', 0)), 1)
            if (not state['search_rejected'] or not best['fun'] < before or remaining <= 0
                    or searches >= _OPTIMIZE_SEARCHES):
                break
            start = best['x'].copy()
    finally:
        if state['accepted']:                      # (a model that was never factored keeps its cache as it was)
            assign(best['x'])
            self.update_cache()
    if state['search_rejected']:
        result.success = False
        result.message = ('the last of %d searches met a parameter vector whose kernel matrix cannot be factored (%d '
                          'rejected in all) and could not be taken up again; the best point seen is kept'
                          % (searches, state['rejected']))
    result.x, result.fun, result.rejected = best['x'].copy(), best['fun'], state['rejected']
    return result


_OPTIMIZE_SEARCHES = 20            # searches of one optimize() call: the first and those taken up after a rejected point


GPRCached.hyperparameters = _gpr_hyperparameters
GPRCached.compute_log_likelihood = _gpr_compute_log_likelihood
GPRCached.log_likelihood_gradient = _gpr_log_likelihood_gradient
GPRCached.optimize = _gpr_optimize


class GaussianProcess(UncertainFunction):
    """``(mean, beta * sqrt(var))`` of a GP model (``functions.py:461-546``)."""

    _role = 'dynamics'

    def __init__(self, gaussian_process, beta=2., name='gaussian_process'):
        self.gaussian_process = gaussian_process
        self.beta = float(beta)
        self.input_dim = gaussian_process.X.shape[1]
        self.output_dim = gaussian_process.Y.shape[1]
        self.n_dim = self.input_dim
        self.name = name

    @property
    def X(self):
        return self.gaussian_process.X

    @property
    def Y(self):
        return self.gaussian_process.Y

    def add_data_point(self, x, y):
        """Append observations (``functions.py:525-546``); the cached factors are extended by a
        rank-one update instead of being rebuilt."""
        self.gaussian_process.append_data(x, y)

    def optimize(self, **kw):
        """Fit the model's hyper-parameters (:meth:`GPRCached.optimize`)."""
        return self.gaussian_process.optimize(**kw)

    def to_mean_function(self):
        """The model without its error bars (``functions.py:209-230``): a :class:`GPMeanFunction`."""
        return GPMeanFunction(self)


class FunctionStack(UncertainFunction):
    """One uncertain function per output column (``functions.py:254-307``)."""

    _role = 'dynamics'

    def __init__(self, functions, name='function_stack'):
        self.functions = list(functions)
        self.num_fun = len(self.functions)
        self.input_dim = self.functions[0].input_dim
        self.output_dim = sum(fun.output_dim for fun in self.functions)
        self.name = name

    def add_data_point(self, x, y):
        for fun, yi in zip(self.functions, np.asarray(y).squeeze()):
            fun.add_data_point(x, yi)

    def optimize(self, **kw):
        """``optimize(**kw)`` of every member, one result per head."""
        return [fun.optimize(**kw) for fun in self.functions]

    def to_mean_function(self):
        """The stacked means as one deterministic function: a :class:`GPMeanFunction`."""
        return GPMeanFunction(self)


def _gp_heads(dynamics):
    """Flatten a GaussianProcess / FunctionStack into ``[(model, beta, col0)]``."""
    funs = dynamics.functions if isinstance(dynamics, FunctionStack) else [dynamics]
    heads, col = [], 0
    for fun in funs:
        if not isinstance(fun, GaussianProcess):
            raise TypeError('FunctionStack members must be GaussianProcess instances')
        heads.append((fun.gaussian_process, fun.beta, col))
        col += fun.output_dim
    betas = {b for _, b, _ in heads}
    if len(betas) != 1:
        raise ValueError('all GP heads must share the same beta')
    return heads, betas.pop()


class GPMeanFunction(DeterministicFunction):
    """The posterior mean of GP dynamics as a deterministic function: what
    ``UncertainFunction.to_mean_function()`` returns (``functions.py:209-230``).

    A live view of ``parent`` (a ``GaussianProcess`` or a ``FunctionStack`` of them), not a copy: after
    ``add_data_point`` or ``optimize()`` on the parent it evaluates the new model.  As the dynamics of a
    ``(dynamics, policy)`` pair it takes ``compute_trajectory``, ``compute_roa`` and ``reward_rollout`` to
    the fused kernels of ``csrc/sl_gp_rollout.hip``; ``PolicyIteration`` treats it as its parent (it only
    ever uses the mean).  ``Lyapunov`` and ``ActorCritic`` refuse it."""

    _role = 'dynamics'

    def __init__(self, parent, name=None):
        if not isinstance(parent, (GaussianProcess, FunctionStack)):
            raise TypeError('to_mean_function needs a GaussianProcess or a FunctionStack of them, not %s'
                            % type(parent).__name__)
        _gp_heads(parent)                              # (a stack of anything else is refused here)
        self.parent = parent
        self.name = name if name is not None else parent.name + '_mean'

    @property
    def input_dim(self):
        return self.parent.input_dim

    @property
    def output_dim(self):
        return self.parent.output_dim

    def __call__(self, *points):
        """``f(states, actions)`` (or the concatenated ``[x, u]`` rows) -> the mean ``[n, d]``
        (``sl_gp_mean_points``: the sum over the training points alone, no variance).  NumPy in gives
        NumPy out, device tensors in give device tensors out."""
        import torch
        from . import _evaluate
        keep = any(isinstance(p, torch.Tensor) for p in points)
        d, p = self.output_dim, self.input_dim
        ctx, builder = _evaluate._builder(d)
        parts = [_evaluate._to_device(ctx, q) for q in points]
        inputs = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).contiguous()
        if inputs.shape[1] != p:
            raise ValueError('%s expects %d inputs [x, u], got %d columns' % (self.name, p, inputs.shape[1]))
        builder.upload(ConstantFunction(np.zeros(p - d)), self, QuadraticFunction(np.eye(d)))
        mean = torch.empty((inputs.shape[0], d), dtype=torch.float64, device=ctx.torch_device)
        ctx.gp_mean_points(inputs.shape[0], inputs, mean)
        return mean if keep else mean.cpu().numpy()


# ----------------------------------------------------------------------------------------------
# piecewise-linear table on a grid
# ----------------------------------------------------------------------------------------------

class Triangulation(DeterministicFunction):
    """Delaunay interpolation of per-vertex values on a ``GridWorld`` (``functions.py:981-1510``).

    As in the reference only ONE unit cell is triangulated (SciPy/Qhull on the cell's corners,
    ``functions.py:1019-1022``) and reused for every cell.  ``parameters`` is the ``[nindex, k]``
    vertex table; the device copy is refreshed whenever it is ASSIGNED.  The array it returns is a
    read-only view: a write into it (``tri.parameters[i] = v``) raises ``ValueError`` instead of
    leaving the device table old (in the reference ``parameters`` is a ``tf.Variable``, which
    cannot be written in place either) - assign a new array: ``tri.parameters = values``."""

    _role = 'value'

    def __init__(self, discretization, vertex_values=None, project=False, name='triangulation'):
        self.discretization = disc = discretization
        self.input_dim = disc.ndim
        self.project = bool(project)
        self.name = name
        self._parameters = None
        self._device_table = None
        self._table_thunk = None                   # (callable, columns): a device table not built yet
        self._table_version = next(_TOKENS)
        self._structure_token = next(_TOKENS)      # grid + unit-cell simplices never change
        if vertex_values is not None:
            self.parameters = vertex_values
        d = disc.ndim
        if d == 1:
            simplices = np.array([[0, 1]], dtype=np.int32)            # functions.py:935-958
        elif d in UNIT_CELL_SIMPLICES:
            # the reference asks Qhull (functions.py:1019-1023); which of the valid triangulations
            # of a box Qhull returns, and in which order, is frozen in unit_cells.py (the answer of
            # scipy 1.15.3 for every cell size): another SciPy cannot move product and oracle
            # together (tests/test_host_logic.py compares this table, the fixture and live SciPy)
            simplices = np.array(UNIT_CELL_SIMPLICES[d], dtype=np.int32)
        else:
            simplices = qhull_unit_cell(disc.unit_maxes)               # d > 4: parity unpinned
        self.unit_simplex_codes = simplices
        self.nsimplex_unit = len(simplices)
        self.nsimplex = self.nsimplex_unit * disc.nrectangles
        if self.nsimplex_unit > _hip.MAX_SIMPLICES:
            raise DimensionError('unit cell has %d simplices (engine limit %d)'
                                 % (self.nsimplex_unit, _hip.MAX_SIMPLICES))
        bits = (simplices[:, :, None] >> np.arange(d)) & 1           # [s, d+1, d]
        verts = bits.astype(config.np_dtype) * disc.unit_maxes
        self.hyperplanes = np.stack([np.linalg.inv(v[1:] - v[:1]) for v in verts])   # :1090-1101

    @property
    def nindex(self):
        return self.discretization.nindex

    @property
    def output_dim(self):
        if self._parameters is not None:
            return self._parameters.shape[1]
        if self._device_table is not None:
            return int(self._device_table.shape[1])
        if self._table_thunk is not None:
            return int(self._table_thunk[1])
        return None

    @property
    def parameters(self):
        """``[nindex, k]`` vertex table on the host, read-only; after a sweep that left the table on
        the GPU (value iteration, policy improvement) it is copied back on first access."""
        table = self._host_parameters()
        if table is None:
            return None
        view = table.view()
        view.flags.writeable = False
        return view

    @parameters.setter
    def parameters(self, values):
        self._parameters = np.ascontiguousarray(
            np.asarray(values, dtype=config.np_dtype).reshape(self.nindex, -1))
        self._device_table = None
        self._table_thunk = None
        self._table_version = next(_TOKENS)

    def _device(self, ctx):
        """Device copy of the vertex table (uploaded lazily)."""
        import torch
        self._resolve_table()
        if self._device_table is None or self._device_table.device != ctx.torch_device:
            self._device_table = torch.from_numpy(self._host_parameters()).to(ctx.torch_device)
        return self._device_table

    def _adopt_device_table(self, tensor):
        """Make a device tensor the truth (value iteration keeps V on the GPU)."""
        self._device_table = tensor.reshape(self.nindex, -1)
        self._table_thunk = None
        self._parameters = None
        self._table_version = next(_TOKENS)

    def _adopt_lazy_device_table(self, build, columns):
        """Like ``_adopt_device_table`` with a table that is only built (``build()`` -> device
        tensor) when somebody reads it: the greedy policy of a value-iteration sweep is replaced by
        the next sweep's before anything looked at it."""
        self._device_table = None
        self._table_thunk = (build, int(columns))
        self._parameters = None
        self._table_version = next(_TOKENS)

    def _resolve_table(self):
        if self._table_thunk is not None:
            build, _ = self._table_thunk
            self._table_thunk = None
            self._device_table = build().reshape(self.nindex, -1)

    def __getstate__(self):
        self._resolve_table()                      # a table that is not built yet is a closure: build it
        return self.__dict__

    def _host_parameters(self):
        self._resolve_table()
        if self._parameters is None and self._device_table is not None:
            self._parameters = self._device_table.cpu().numpy().reshape(self.nindex, -1)
        return self._parameters

    def _upload(self, ctx, slot):
        ctx.tri_set(slot, self.discretization._desc(), self.unit_simplex_codes, self.hyperplanes,
                    self.discretization.discrete_points, self.project,
                    self._device(ctx).shape[1], self._device(ctx))

    def parameter_gradient(self, points, coefficients):
        """``sum_i coefficients[i, :] * d table(points[i]) / d parameters`` -> ``[nindex, k]``: vertex
        ``v`` receives ``coefficients[i] * w_ik`` from every point whose simplex has ``v`` as its corner
        ``k`` (weights and simplices as the evaluation computes them, ``project`` included) - what
        ``tf.gradients(sum(coefficients * table(points)), parameters)`` returns for the reference's
        table.  ``points`` ``[n, d]`` and ``coefficients`` ``[n, k]`` are NumPy arrays or device
        tensors; the sums run on the GPU (``sl_tri_param_grad``) in a fixed order, the same bits at
        every call."""
        import torch
        from . import _evaluate
        if self.output_dim is None:
            raise ValueError('the table has no parameters yet')
        ctx, builder = _evaluate._builder(self.input_dim)
        d_points, d_coeff = _evaluate._points_and_coefficients(ctx, points, coefficients, self.input_dim, 'table')
        n = d_points.shape[0]
        if tuple(d_coeff.shape) != (n, self.output_dim):
            raise ValueError('coefficients of shape %s for %d points and %d columns'
                             % (tuple(d_coeff.shape), n, self.output_dim))
        builder._upload_tri(1, self)
        out = torch.empty((self.nindex, self.output_dim), dtype=torch.float64, device=ctx.torch_device)
        ctx.tri_param_grad(1, n, d_points, d_coeff, out)
        gradient = out.cpu().numpy()
        return -gradient if self.negate else gradient


# ----------------------------------------------------------------------------------------------
# analytic dynamics of the examples
# ----------------------------------------------------------------------------------------------

def _normalization(normalization):
    if normalization is None:
        return None, None
    norm = [np.array(v, dtype=config.np_dtype) for v in normalization]
    return norm, [v ** -1 for v in norm]


def _pendulum_linearize(mass, length, friction, dt, norm, gravity=9.81):
    """Discretised linearisation of the pendulum about the upright position
    (``examples/utilities.py:207-240``)."""
    inertia = mass * length ** 2
    A = np.array([[0, 1], [gravity / length, -friction / inertia]])
    B = np.array([[0], [1 / inertia]])
    Tx, Tu = np.diag(norm[0]), np.diag(norm[1])
    A = np.linalg.multi_dot((np.linalg.inv(Tx), A, Tx))
    B = np.linalg.multi_dot((np.linalg.inv(Tx), B, Tu))
    sysd = scipy.signal.StateSpace(A, B, np.eye(2), np.zeros((2, 1))).to_discrete(dt)
    return sysd.A, sysd.B


def _cartpole_linearize(m, M, L, b, dt, norm, gravity=9.81):
    """Zero-order-hold discretisation of the linearised cart-pole
    (``examples/utilities.py:352-385``)."""
    g = gravity
    A = np.array([[0, 0, 1, 0], [0, 0, 0, 1], [0, g * m / M, 0, -b / (M * L)],
                  [0, g * (m + M) / (L * M), 0, -b * (m + M) / (m * M * L ** 2)]])
    B = np.array([0, 0, 1 / M, 1 / (M * L)]).reshape(-1, 1)
    Tx, Tu = np.diag(norm[0]), np.diag(norm[1])
    A = np.linalg.multi_dot((np.linalg.inv(Tx), A, Tx))
    B = np.linalg.multi_dot((np.linalg.inv(Tx), B, Tu))
    Ad, Bd, _, _, _ = scipy.signal.cont2discrete((A, B, 0, 0), dt, method='zoh')
    return Ad, Bd


class InvertedPendulum(DeterministicFunction):
    """Pendulum with 10 explicit-Euler sub-steps (``examples/utilities.py:144-289``)."""

    _role = 'dynamics'

    def __init__(self, mass, length, friction=0, dt=1 / 80, normalization=None):
        self.mass, self.length, self.friction, self.dt = mass, length, friction, dt
        self.gravity = 9.81
        self.normalization, self.inv_norm = _normalization(normalization)
        self.input_dim, self.output_dim = 3, 2

    @property
    def inertia(self):
        return self.mass * self.length ** 2

    def linearize(self):
        """``(A, B)`` of the discretised linearisation about the upright rest position, in
        normalised coordinates when a normalisation is set (same result as
        ``examples/utilities.py:207-240``)."""
        norm = self.normalization if self.normalization is not None else [np.ones(2), np.ones(1)]
        return _pendulum_linearize(self.mass, self.length, self.friction, self.dt, norm,
                                   gravity=self.gravity)

    def _write_dynamics(self, desc):
        desc.kind = _hip.DYN_PENDULUM
        desc.coef[0] = self.dt / 10
        desc.coef[1] = self.gravity / self.length
        desc.coef[2] = self.inertia
        desc.coef[3] = self.friction / self.inertia
        desc.coef[4] = 1.0 if self.friction > 0 else 0.0
        _write_norm(desc, self.normalization, self.inv_norm, 2)


class CartPole(DeterministicFunction):
    """Cart-pole with 10 explicit-Euler sub-steps (``examples/utilities.py:292-437``)."""

    _role = 'dynamics'

    def __init__(self, pendulum_mass, cart_mass, length, rot_friction=0.0, dt=0.01,
                 normalization=None):
        self.pendulum_mass, self.cart_mass, self.length = pendulum_mass, cart_mass, length
        self.rot_friction, self.dt, self.gravity = rot_friction, dt, 9.81
        self.state_dim, self.action_dim = 4, 1
        self.input_dim, self.output_dim = 5, 4
        self.normalization, self.inv_norm = _normalization(normalization)

    def linearize(self):
        """``(A, B)`` of the zero-order-hold discretisation of the linearised cart-pole, in
        normalised coordinates when a normalisation is set (same result as
        ``examples/utilities.py:352-385``)."""
        norm = self.normalization if self.normalization is not None else [np.ones(4), np.ones(1)]
        return _cartpole_linearize(self.pendulum_mass, self.cart_mass, self.length,
                                   self.rot_friction, self.dt, norm, gravity=self.gravity)

    def _write_dynamics(self, desc):
        m, M, L, b, g = (self.pendulum_mass, self.cart_mass, self.length, self.rot_friction,
                         self.gravity)
        desc.kind = _hip.DYN_CARTPOLE
        # the products below are evaluated in the operator order of examples/utilities.py:430-433
        for k, v in enumerate([self.dt / 10, m, M, L, b, m * L, 0.5 * m * g * L, 0.5 * m * L,
                               b * (m + M), (m + M) * g]):
            desc.coef[k] = float(v)
        _write_norm(desc, self.normalization, self.inv_norm, 4)


def _write_norm(desc, normalization, inv_norm, d):
    desc.normalize = 0 if normalization is None else 1
    for k in range(d):
        desc.tx[k] = 1.0 if normalization is None else float(normalization[0][k])
        desc.tx_inv[k] = 1.0 if normalization is None else float(inv_norm[0][k])
    desc.tu[0] = 1.0 if normalization is None else float(normalization[1][0])


class PolynomialSystem(DeterministicFunction):
    """Dynamics whose vector field is a polynomial in ``z = [x, u]``, given as data: the way to run a
    system of one's own (Van der Pol, Duffing, Lotka-Volterra, Lorenz, Taylor models) through the
    sweeps, rollouts and dynamic programming without a callable.

    ``terms`` holds one list per state, each entry ``(coefficient, exponents)`` with one non-negative
    integer exponent per entry of ``z`` (``len(exponents) == state_dim + action_dim``): row ``i`` is
    ``sum coefficient * prod_q z_q ** exponents[q]``.  One call advances the state by
    ``inner_euler_steps`` explicit-Euler steps of ``dt / inner_euler_steps`` with the action held;
    ``inner_euler_steps=0`` makes the polynomial the discrete map ``x+ = p(x, u)`` itself.
    ``normalization = [state_norm, action_norm]`` as for :class:`InvertedPendulum`: inputs and outputs
    are in normalised coordinates, the polynomial in physical ones.  At most ``_hip.POLY_MAX_TERMS``
    terms of total degree ``_hip.POLY_MAX_DEGREE`` or less.  The engine evaluates every term by
    repeated multiplication in the order given (``csrc/sl_polynomial.h``)."""

    _role = 'dynamics'

    def __init__(self, terms, state_dim, action_dim=1, dt=0.01, inner_euler_steps=10, normalization=None):
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        d, m = self.state_dim, self.action_dim
        if not 1 <= d <= _hip.MAX_STATE_DIM or not 1 <= m <= _hip.MAX_ACTION_DIM or d + m > _hip.MAX_INPUT_DIM:
            raise ValueError('PolynomialSystem: %d states and %d actions (the engine takes 1..%d and 1..%d, %d inputs)'
                             % (d, m, _hip.MAX_STATE_DIM, _hip.MAX_ACTION_DIM, _hip.MAX_INPUT_DIM))
        self.input_dim, self.output_dim = d + m, d
        self.dt = float(dt)
        self.inner_euler_steps = int(inner_euler_steps)
        if self.inner_euler_steps < 0:
            raise ValueError('PolynomialSystem: inner_euler_steps must not be negative')
        terms = [list(row) for row in terms]
        if len(terms) != d:
            raise ValueError('PolynomialSystem: %d term lists for %d states (one list per state, [] for none)'
                             % (len(terms), d))
        rows, coef, expo = [], [], []
        for i, row in enumerate(terms):
            for coefficient, exponents in row:
                exponents = [int(e) for e in exponents]
                if len(exponents) != d + m:
                    raise ValueError('PolynomialSystem: a term of row %d has %d exponents, state_dim + action_dim = %d'
                                     % (i, len(exponents), d + m))
                if min(exponents) < 0:
                    raise ValueError('PolynomialSystem: negative exponent in row %d' % i)
                if sum(exponents) > _hip.POLY_MAX_DEGREE:
                    raise ValueError('PolynomialSystem: a term of row %d has total degree %d, the engine takes %d'
                                     % (i, sum(exponents), _hip.POLY_MAX_DEGREE))
                rows.append(i)
                coef.append(float(coefficient))
                expo.append(exponents)
        if len(rows) > _hip.POLY_MAX_TERMS:
            raise ValueError('PolynomialSystem: %d terms, the engine takes %d' % (len(rows), _hip.POLY_MAX_TERMS))
        self.terms = [[(c, tuple(e)) for r, c, e in zip(rows, coef, expo) if r == i] for i in range(d)]
        self._rows = np.array(rows, dtype=np.int32)
        self._coef = np.array(coef, dtype=np.float64)
        self._expo = np.array(expo, dtype=np.uint8).reshape(len(rows), d + m)
        self.normalization, self.inv_norm = _normalization(normalization)
        if self.normalization is not None and (len(self.normalization) != 2 or self.normalization[0].shape != (d,)
                                               or self.normalization[1].shape != (m,)):
            raise ValueError('PolynomialSystem: normalization is [state_norm (%d), action_norm (%d)]' % (d, m))
        self._version = next(_TOKENS)          # a spec is immutable: one upload per context

    @property
    def step(self):
        """Length of one Euler sub-step (not used by a discrete map)."""
        return self.dt / self.inner_euler_steps if self.inner_euler_steps else 0.0

    def ode(self, states, actions=None):
        """The polynomial itself at physical ``states`` ``[n, state_dim]`` and ``actions``
        ``[n, action_dim]`` (``None``: zeros), in NumPy: the time derivative, or the next state of a
        discrete map."""
        states = np.atleast_2d(np.asarray(states, dtype=config.np_dtype))
        if actions is None:
            actions = np.zeros((len(states), self.action_dim), dtype=config.np_dtype)
        actions = np.atleast_2d(np.asarray(actions, dtype=config.np_dtype))
        z = np.hstack((states, np.broadcast_to(actions, (len(states), self.action_dim))))
        out = np.zeros((len(states), self.state_dim), dtype=config.np_dtype)
        for i, row in enumerate(self.terms):
            for coefficient, exponents in row:
                prod = np.full(len(states), coefficient, dtype=config.np_dtype)
                for q, e in enumerate(exponents):
                    for _ in range(e):
                        prod = prod * z[:, q]
                out[:, i] = out[:, i] + prod
        return out

    def linearize(self):
        """``(Ad, Bd)`` about the origin in normalised coordinates: the degree-1 terms under a
        zero-order hold over ``dt``; for a discrete map (``inner_euler_steps=0``) the degree-1 terms
        themselves."""
        d, m = self.state_dim, self.action_dim
        jac = np.zeros((d, d + m), dtype=config.np_dtype)
        for i, row in enumerate(self.terms):
            for coefficient, exponents in row:
                if sum(exponents) == 1:
                    jac[i, exponents.index(1)] += coefficient
        A, B = jac[:, :d], jac[:, d:]
        if self.normalization is not None:
            Tx, Tu = np.diag(self.normalization[0]), np.diag(self.normalization[1])
            Tx_inv = np.diag(self.inv_norm[0])
            A = np.linalg.multi_dot((Tx_inv, A, Tx))
            B = np.linalg.multi_dot((Tx_inv, B, Tu))
        if self.inner_euler_steps == 0:
            return A, B
        Ad, Bd, _, _, _ = scipy.signal.cont2discrete((A, B, 0, 0), self.dt, method='zoh')
        return Ad, Bd

    def _write_dynamics(self, desc, builder):
        d, m = self.state_dim, self.action_dim
        desc.kind = _hip.DYN_POLYNOMIAL
        desc.normalize = 0 if self.normalization is None else 1
        for k in range(d):
            desc.tx[k] = 1.0 if self.normalization is None else float(self.normalization[0][k])
            desc.tx_inv[k] = 1.0 if self.normalization is None else float(self.inv_norm[0][k])
        for a in range(m):
            desc.tu[a] = 1.0 if self.normalization is None else float(self.normalization[1][a])
        if builder._poly_signature != self._version:
            builder.ctx.dynamics_polynomial_set(d, m, self._rows, self._coef, self._expo, self.inner_euler_steps,
                                                self.step)
            builder._poly_signature = self._version


class VanDerPol(PolynomialSystem):
    """Van der Pol oscillator in reverse time, ten explicit-Euler sub-steps
    (``examples/utilities.py:440-519``): ``x' = -y``, ``y' = x + damping (x^2 - 1) y``.
    ``normalization`` holds the two state scales.  The reference evaluates it on ``[state, action]``
    rows with one action column that it drops (``tf.split(state_action, [2, 1])``): here that column
    is an action no term reads."""

    def __init__(self, damping=1, dt=0.01, normalization=None):
        self.damping = damping
        terms = [[(-1.0, (0, 1, 0))],
                 [(1.0, (1, 0, 0)), (float(damping), (2, 1, 0)), (-float(damping), (0, 1, 0))]]
        pair = None if normalization is None else [normalization, [1.0]]
        super(VanDerPol, self).__init__(terms, 2, 1, dt=dt, inner_euler_steps=10, normalization=pair)

    def linearize(self):
        """``Ad`` of the discretised linearisation in normalised coordinates (``examples/utilities.py:471-487``)."""
        return super(VanDerPol, self).linearize()[0]


# ----------------------------------------------------------------------------------------------
# polynomial Lyapunov / value function
# ----------------------------------------------------------------------------------------------

def monomial_exponents(input_dim, degree):
    """Exponent rows of the monomial basis ``m(z)`` of total degree 1 .. ``degree`` (no constant term):
    graded, the first variable's power descending inside a degree.  Two variables, degree 3:
    ``x, y, x^2, xy, y^2, x^3, x^2 y, x y^2, y^3`` - the column order of ``examples/utilities.py:753-782``."""
    input_dim, degree = int(input_dim), int(degree)
    if input_dim < 1 or degree < 1:
        raise ValueError('monomial_exponents: input_dim and degree must be at least 1')

    def rows(n, total):
        if n == 1:
            return [(total,)]
        return [(first,) + rest for first in range(total, -1, -1) for rest in rows(n - 1, total - first)]

    return np.array([row for total in range(1, degree + 1) for row in rows(input_dim, total)], dtype=np.int64)


class PolynomialFunction(DeterministicFunction):
    """A Lyapunov / value function that is a polynomial in the state, given as data: the way to state a
    candidate of one's own (a sum-of-squares certificate, a Taylor model) where a quadratic form is too
    little, without a callable.

    ``terms`` is a list of ``(coefficient, exponents)`` with one non-negative integer exponent per state:
    ``V(x) = sum_t c_t * prod_q (x_q * T_q) ** e_tq`` with ``T = normalization`` (``None``: no scaling) - the
    argument is scaled UP by ``T``, as ``x *= state_norm`` in ``lyapunov_function_learning.ipynb`` cell 17.
    ``V(points)`` and ``V.gradient(points)`` (with respect to the argument: the chain factor ``T_k`` is
    included) run on the device; ``-V`` is supported.  ``Gradient(V)`` inside ``AbsFunction`` /
    ``Norm1Function`` is the local Lipschitz constant.  Limits: ``input_dim <= MAX_STATE_DIM`` (6), total degree
    of a term ``<= POLY_MAX_DEGREE`` (8), and ``POLYV_MAX_ENTRIES`` (256) entries in the device table, which
    holds the value row and one row per partial derivative (a term counts once, and once more for every
    variable it contains).  The engine evaluates every term by repeated multiplication in the order given
    (``csrc/sl_poly_value.h``)."""

    _role = 'value'

    def __init__(self, terms, input_dim, normalization=None, name='polynomial_function'):
        self.input_dim = self.ndim = int(input_dim)
        self.output_dim = 1
        self.name = name
        d = self.input_dim
        if not 1 <= d <= _hip.MAX_STATE_DIM:
            raise ValueError('PolynomialFunction: input_dim = %d, the engine takes 1..MAX_STATE_DIM = %d'
                             % (d, _hip.MAX_STATE_DIM))
        coef, expo = [], []
        for t, (coefficient, exponents) in enumerate(terms):
            exponents = list(np.atleast_1d(np.asarray(exponents)).tolist())
            if len(exponents) != d:
                raise ValueError('PolynomialFunction: term %d has %d exponents, input_dim = %d'
                                 % (t, len(exponents), d))
            if any(isinstance(e, bool) or e != int(e) for e in exponents):
                raise ValueError('PolynomialFunction: term %d has a non-integer exponent %r' % (t, exponents))
            exponents = [int(e) for e in exponents]
            if min(exponents) < 0:
                raise ValueError('PolynomialFunction: term %d has a negative exponent %r' % (t, exponents))
            if sum(exponents) > _hip.POLY_MAX_DEGREE:
                raise ValueError('PolynomialFunction: term %d has total degree %d, the engine takes POLY_MAX_DEGREE = %d'
                                 % (t, sum(exponents), _hip.POLY_MAX_DEGREE))
            coef.append(float(coefficient))
            expo.append(exponents)
        entries = len(coef) + sum(1 for e in expo for v in e if v > 0)
        if entries > _hip.POLYV_MAX_ENTRIES:
            raise ValueError('PolynomialFunction: %d terms need %d entries of the device table (value row and '
                             'gradient rows), the engine takes POLYV_MAX_ENTRIES = %d'
                             % (len(coef), entries, _hip.POLYV_MAX_ENTRIES))
        self.terms = [(c, tuple(e)) for c, e in zip(coef, expo)]
        self._coef = np.array(coef, dtype=np.float64)
        self._expo = np.array(expo, dtype=np.uint8).reshape(len(coef), d)
        if normalization is None:
            self.normalization = None
        else:
            self.normalization = np.array(normalization, dtype=np.float64).reshape(-1)
            if self.normalization.shape != (d,):
                raise ValueError('PolynomialFunction: normalization holds %d scales, input_dim = %d'
                                 % (len(self.normalization), d))
        self._version = next(_TOKENS)          # a spec is immutable: one upload per context

    @classmethod
    def from_gram(cls, Q, degree, input_dim, normalization=None, name='polynomial_function'):
        """``m(z)^T Q m(z)`` with ``m`` the basis of :func:`monomial_exponents`, expanded into a term table
        on the host: one term per distinct monomial in order of first appearance over ``(i, j)`` row-major,
        its coefficient the sum of the ``Q_ij`` that produce it, added in that order.  ``Q`` need not be
        symmetric or definite."""
        basis = monomial_exponents(input_dim, degree)
        Q = np.asarray(Q, dtype=np.float64)
        if Q.shape != (len(basis), len(basis)):
            raise ValueError('PolynomialFunction.from_gram: Q is %s, the basis of degree %d in %d variables has %d '
                             'monomials' % (Q.shape, degree, input_dim, len(basis)))
        coefficients = {}
        for i in range(len(basis)):
            for j in range(len(basis)):
                key = tuple(int(e) for e in basis[i] + basis[j])
                coefficients[key] = Q[i, j] if key not in coefficients else coefficients[key] + Q[i, j]
        return cls([(float(c), key) for key, c in coefficients.items()], input_dim, normalization, name=name)

    def gradient(self, points):
        """``dV/dx`` at ``points`` ``[n, input_dim]`` -> ``[n, input_dim]`` (device tensors stay on the
        device), evaluated on the GPU."""
        from . import _evaluate
        return _evaluate.value_gradient(self, points)

    def _write_value(self, desc, builder):
        if builder.grid.ndim != self.input_dim:
            raise ValueError('%s takes %d inputs, the grid has %d dimensions'
                             % (type(self).__name__, self.input_dim, builder.grid.ndim))
        desc.kind = _hip.V_POLYNOMIAL
        desc.negate = int(self.negate)
        if builder._polyv_signature != self._version:
            builder.ctx.value_polynomial_set(self.input_dim, self._coef, self._expo, self.normalization)
            builder._polyv_signature = self._version


# ----------------------------------------------------------------------------------------------
# positive-definite network
# ----------------------------------------------------------------------------------------------

_ACTIVATIONS = {None: 0, 'linear': 0, 'tanh': 1, 'relu': 2}


class NeuralNetwork(DeterministicFunction):
    """A chain of dense layers as a POLICY (``functions.py:1663-1729``; the policy of
    ``examples/inverted_pendulum.ipynb:215`` and of the reinforcement-learning notebooks).

    ``layers`` are the units of every dense layer (``build_evaluation``, ``:1702-1725``: one
    ``tf.layers.dense`` per entry, the input width is the data's), ``nonlinearities`` one entry per
    layer - ``'relu'``, ``'tanh'``, ``'sigmoid'`` or ``None`` (the reference passes TensorFlow
    callables; the names of the ones it uses are accepted here) -, ``output_scale`` multiplies the
    output (``:1727-1728``); with ``use_bias`` every layer but the last has a bias (``:1712, 1722``).

    The reference's parameters are TensorFlow variables (Xavier initialisation, trained by SGD): here
    they are NumPy arrays on the host, ``parameters = [W_0, b_0, W_1, b_1, ..., W_out]`` in the
    reference's variable order (``_parameter_iter``, ``:1731-1740``; ``W_l`` is ``[in, units]``;
    without biases just the ``W_l``), given or drawn Xavier-uniform from ``seed`` once ``input_dim`` is
    known.  Assigning ``parameters`` again (or calling :meth:`touch` after editing the arrays in place)
    makes the engine upload them again.  Training: :meth:`parameter_gradient` sums ``coefficients *
    d policy / d parameters`` over a batch on the GPU; ``PolicyIteration.policy_gradient`` and
    ``training.policy_improvement_step`` build the notebook's policy-improvement step
    (``optimizer.minimize(-reduce(rl.future_values(states)), var_list=rl.policy.parameters)``) on it."""

    _role = 'policy'
    _ACTIVATIONS = {None: 0, 'linear': 0, 'tanh': 1, 'relu': 2, 'sigmoid': 3}

    def __init__(self, layers, nonlinearities, output_scale=1., use_bias=True, name='neural_network',
                 input_dim=None, parameters=None, seed=0):
        self.layers = [int(v) for v in layers]
        self.nonlinearities = [getattr(a, '__name__', a) for a in nonlinearities]
        if len(self.nonlinearities) != len(self.layers):
            raise ValueError('one nonlinearity (or None) per layer')
        for a in self.nonlinearities:
            if a not in self._ACTIVATIONS:
                raise TypeError('nonlinearity %r: the engine has relu, tanh, sigmoid and None' % (a,))
        self.output_scale = float(output_scale)
        self.use_bias = bool(use_bias)
        self.name = name
        self.output_dim = self.layers[-1]
        self.input_dim = None if input_dim is None else int(input_dim)
        self._parameters = None
        self._version = next(_TOKENS)
        self._seed = seed
        if parameters is not None:
            self.parameters = parameters
        elif input_dim is not None:
            self._initialise()

    def _shapes(self):
        widths = [self.input_dim] + self.layers
        shapes = []
        for l in range(len(self.layers)):
            shapes.append((widths[l], widths[l + 1]))
            if self.use_bias and l < len(self.layers) - 1:
                shapes.append((widths[l + 1],))
        return shapes

    def _initialise(self):
        rng = np.random.default_rng(self._seed)
        params = []
        for shape in self._shapes():
            if len(shape) == 2:                       # tf.contrib.layers.xavier_initializer (uniform)
                params.append(rng.uniform(-1, 1, shape) * np.sqrt(6. / (shape[0] + shape[1])))
            else:
                params.append(np.zeros(shape))        # tf.layers.dense: zero bias
        self.parameters = params

    @property
    def parameters(self):
        return self._parameters

    @parameters.setter
    def parameters(self, values):
        values = [np.asarray(v, dtype=config.np_dtype) for v in values]
        if self.input_dim is None:
            self.input_dim = int(values[0].shape[0])
        if [v.shape for v in values] != self._shapes():
            raise ValueError('parameters must have shapes %s' % (self._shapes(),))
        self._parameters = values
        self._version = next(_TOKENS)

    def touch(self):
        """Say that the parameter arrays were edited in place."""
        self._version = next(_TOKENS)

    def _layers_for_upload(self, d):
        """``(dims, activation codes, kernels, biases)`` of the chain for a d-dimensional state."""
        if self.input_dim is None:
            self.input_dim = int(d)
            self._initialise()
        if self.input_dim != d:
            raise ValueError('the network expects %d inputs, the grid has %d dimensions'
                             % (self.input_dim, d))
        it = iter(self._parameters)
        kernels, biases = [], []
        for l in range(len(self.layers)):
            kernels.append(next(it))
            biases.append(next(it) if (self.use_bias and l < len(self.layers) - 1) else None)
        return ([self.input_dim] + self.layers, [self._ACTIVATIONS[a] for a in self.nonlinearities],
                kernels, biases)

    def _on_engine(self):
        """The point-evaluation context with this network's current parameters on it (uploaded again
        only when they changed: ``ModelBuilder._write_policy``)."""
        from . import _evaluate
        if self.input_dim is None:
            raise ValueError('the network has no parameters yet: give input_dim or parameters')
        ctx, builder = _evaluate._builder(self.input_dim)
        builder._write_policy(_hip.ModelDesc(), self)
        return ctx

    def _description(self):
        """``(dims, activation codes, bias flags)`` of the chain, as the engine's stateless calls take them
        (``sl_critic_batch``, ``sl_dense_param_grad``)."""
        if self.input_dim is None:
            raise ValueError('the network has no parameters yet: give input_dim or parameters')
        nl = len(self.layers)
        return ([self.input_dim] + self.layers, [self._ACTIVATIONS[a] for a in self.nonlinearities],
                [int(self.use_bias and l < nl - 1) for l in range(nl)])

    def _device_parameters(self, ctx):
        """The parameters as ONE device tensor in the order ``W_0, b_0, W_1, b_1, ...`` (what
        ``sl_policy_network_set`` packs on its side), copied again only when ``_version`` moved."""
        import torch
        key = (self._version, str(ctx.torch_device))
        cached = getattr(self, '_device_copy', None)
        if cached is None or cached[0] != key:
            flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in self._parameters])
            cached = (key, torch.from_numpy(flat).to(ctx.torch_device))
            self._device_copy = cached
        return cached[1]

    def _unflatten(self, flat):
        """A flat array in the order of ``_device_parameters`` as a list shaped like ``parameters``."""
        shapes = self._shapes()
        offsets = np.concatenate(([0], np.cumsum([int(np.prod(shape)) for shape in shapes])))
        return [flat[offsets[k]:offsets[k + 1]].reshape(shape).copy() for k, shape in enumerate(shapes)]

    def parameter_gradient(self, points, coefficients):
        """``sum_i sum_o coefficients[i, o] * d policy_o(points[i]) / d theta`` for every array
        ``theta`` of ``parameters`` (a list shaped like ``parameters``): what
        ``tf.gradients(sum(coefficients * policy(points)), parameters)`` returns for the reference's
        network, ``output_scale`` included.  ``points`` ``[n, d]`` and ``coefficients`` ``[n, m]`` are
        NumPy arrays or device tensors; the sum over the points runs on the GPU
        (``sl_policy_param_grad``) and is the same bit for bit at every call."""
        import torch
        from . import _evaluate
        if self.negate:
            raise ValueError('differentiate the network itself, not its negation')
        ctx = self._on_engine()
        d_points, d_coeff = _evaluate._points_and_coefficients(ctx, points, coefficients, self.input_dim, 'network')
        n, d = d_points.shape
        if tuple(d_coeff.shape) != (n, self.output_dim):
            raise ValueError('coefficients of shape %s for %d points and %d outputs'
                             % (tuple(d_coeff.shape), n, self.output_dim))
        shapes = self._shapes()
        sizes = [int(np.prod(shape)) for shape in shapes]
        out = torch.empty(sum(sizes), dtype=torch.float64, device=ctx.torch_device)
        ctx.policy_param_grad(n, d, d_points, d_coeff, out)
        flat = out.cpu().numpy()
        offsets = np.concatenate(([0], np.cumsum(sizes)))
        return [flat[offsets[k]:offsets[k + 1]].reshape(shape).copy() for k, shape in enumerate(shapes)]

    def lipschitz(self):
        """``|output_scale| * prod_l sigma_max(W_l)``: a Lipschitz constant of the network for
        contractive nonlinearities (relu, tanh, sigmoid), by SVD of the host copy of the kernels
        (``functions.py:1744-1786``, whose product leaves the output scale to the caller)."""
        if self._parameters is None:
            raise ValueError('the network has no parameters yet: give input_dim or parameters')
        constant = abs(self.output_scale)
        for w in self._parameters:
            if w.ndim == 2:
                constant *= float(np.linalg.svd(w, compute_uv=False).max())
        return constant


class LyapunovNetwork(DeterministicFunction):
    """``sum(phi(x)^2)`` with layer kernels ``[W^T W + eps I ; W']``
    (``examples/utilities.py:48-104``).  ``activations`` are names ('tanh', 'relu', None);
    ``weights`` the flat variable list in the reference's creation order, or ``None`` for
    Xavier-uniform initialisation from ``seed``."""

    _role = 'value'

    def __init__(self, input_dim, layer_dims, activations, eps=1e-6, weights=None, seed=0,
                 name='lyapunov_network'):
        self.input_dim = int(input_dim)
        self.num_layers = len(layer_dims)
        self.activations = list(activations)
        self.eps = float(eps)
        self.name = name
        if layer_dims[0] < input_dim:
            raise ValueError('The first layer dimension must be at least the input dimension!')
        if not np.all(np.diff(layer_dims) >= 0):
            raise ValueError('Each layer must maintain or increase the dimension of its input!')
        self.output_dims = list(layer_dims)
        self.hidden_dims = [int(np.ceil(((self.input_dim if i == 0 else layer_dims[i - 1]) + 1) / 2))
                            for i in range(self.num_layers)]
        shapes = self.weight_shapes()
        if weights is None:
            rng = np.random.default_rng(seed)
            weights = [rng.uniform(-1, 1, s) * np.sqrt(6. / (s[0] + s[1])) for s in shapes]
        self.weights = [np.asarray(w, dtype=config.np_dtype) for w in weights]
        if [w.shape for w in self.weights] != shapes:
            raise ValueError('weights must have shapes %s' % (shapes,))

    def weight_shapes(self):
        shapes = []
        for i in range(self.num_layers):
            in_dim = self.input_dim if i == 0 else self.output_dims[i - 1]
            shapes.append((self.hidden_dims[i], in_dim))
            if self.output_dims[i] > in_dim:
                shapes.append((self.output_dims[i] - in_dim, in_dim))
        return shapes

    def kernels(self):
        """Per-layer ``[out_i, in_i]`` matrices (``examples/utilities.py:95-100``)."""
        out, it = [], iter(self.weights)
        for i in range(self.num_layers):
            in_dim = self.input_dim if i == 0 else self.output_dims[i - 1]
            W = next(it)
            kernel = W.T.dot(W) + self.eps * np.eye(in_dim)
            if self.output_dims[i] > in_dim:
                kernel = np.concatenate([kernel, next(it)], axis=0)
            out.append(kernel)
        return out

    def _upload(self, ctx):
        dims = [self.input_dim] + self.output_dims
        ctx.network_set(dims, [_ACTIVATIONS[a] for a in self.activations], self.kernels())

    def _on_engine(self):
        """The point-evaluation context with this network's current kernels on it (uploaded again only
        when the weights changed: ``ModelBuilder._write_value``)."""
        from . import _evaluate
        ctx, builder = _evaluate._builder(self.input_dim)
        builder._write_value(_hip.ValueDesc(), self)
        return ctx

    def _weights_gradient(self, kernel_gradients):
        """The derivative with respect to the variables from the derivative ``G_l`` with respect to the
        layer kernels ``[W^T W + eps I ; W']`` (flat, ``[out_l][in_l]`` per layer): ``W (G_top +
        G_top^T)`` and ``G_bottom``, in the order of ``weights``.  NumPy float64 on the host, where
        the master copy of the weights lives."""
        flat = np.asarray(kernel_gradients, dtype=np.float64).ravel()
        out, it, offset = [], iter(self.weights), 0
        for i in range(self.num_layers):
            in_dim = self.input_dim if i == 0 else self.output_dims[i - 1]
            rows = self.output_dims[i]
            G = flat[offset:offset + rows * in_dim].reshape(rows, in_dim)
            offset += rows * in_dim
            W = next(it)
            out.append(W.dot(G[:in_dim] + G[:in_dim].T))
            if rows > in_dim:
                next(it)
                out.append(G[in_dim:].copy())
        return out

    def parameter_gradient(self, points, coefficients):
        """``sum_m coefficients[m] * dV(points[m]) / d theta`` for every array ``theta`` of ``weights``
        (a list shaped like ``weights``): what ``tf.gradients(sum(c * V(p)), parameters)`` returns
        for the reference's network.  ``points`` ``[M, d]`` and ``coefficients`` ``[M]`` are NumPy
        arrays or device tensors; the sum over the points runs on the GPU (``sl_nn_param_grad``) and
        is the same bit for bit at every call."""
        from . import _evaluate
        ctx = self._on_engine()
        d_points, d_coeff = _evaluate._points_and_coefficients(ctx, points, coefficients, self.input_dim, 'network')
        d_coeff = d_coeff.reshape(-1)
        if d_coeff.numel() != d_points.shape[0]:
            raise ValueError('%d coefficients for %d points' % (d_coeff.numel(), d_points.shape[0]))
        gradient = self._weights_gradient(self._kernel_gradient(ctx, d_points, d_coeff))
        return [-g for g in gradient] if self.negate else gradient

    def _kernel_gradient(self, ctx, d_points, d_coeff):
        """``sl_nn_param_grad`` on device tensors -> the flat ``G_l`` on the host."""
        import torch
        dims = [self.input_dim] + self.output_dims
        total = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        out = torch.empty(total, dtype=torch.float64, device=ctx.torch_device)
        ctx.nn_param_grad(d_points.shape[0], d_points.shape[1], d_points, d_coeff, out)
        return out.cpu().numpy()


# ----------------------------------------------------------------------------------------------
# sample paths of a Gaussian process
# ----------------------------------------------------------------------------------------------

SAMPLE_JITTER = 1e-8            # added to the diagonal of the covariance before it is factored (functions.py:1630)


def _sample_setup(discretization, gpfun, who):
    """The checked arguments of the sampling functions -> the ``[N, p]`` discretization and the GP model."""
    from . import distributed as dist_utils
    if dist_utils.rank_and_world()[1] > 1:
        raise NotImplementedError('%s runs on one GPU; under torch.distributed call it on one rank and broadcast '
                                  'the samples' % who)
    if isinstance(discretization, GridWorld):
        discretization = discretization.all_points
    if not isinstance(gpfun, GaussianProcess):
        raise TypeError('%s: gpfun must be a GaussianProcess, not %s' % (who, type(gpfun).__name__))
    if gpfun.output_dim != 1:
        raise ValueError('%s samples one-output Gaussian processes; gpfun has output_dim %d (sample the members of a '
                         'FunctionStack one by one)' % (who, gpfun.output_dim))
    points = np.ascontiguousarray(np.asarray(discretization, dtype=config.np_dtype))
    if points.ndim != 2 or points.shape[0] < 1 or points.shape[1] != gpfun.input_dim:
        raise ValueError('%s: the discretization must be [N, %d] with N >= 1, got %s'
                         % (who, gpfun.input_dim, points.shape))
    return points, gpfun.gaussian_process


def _gp_prior_row(gp):
    return None if gp.mean_function is None else np.asarray(gp.mean_function.matrix, dtype=config.np_dtype)[0]


def _sample_factor(ctx, points, gp, who):
    """Posterior mean ``[N]`` and the lower Cholesky factor of ``cov + 1e-8 I`` at ``points``, on the device."""
    import torch
    n_points, p = points.shape
    d_points = torch.from_numpy(points).to(ctx.torch_device)
    d_mean = torch.empty(n_points, dtype=torch.float64, device=ctx.torch_device)
    d_cov = torch.empty((n_points, n_points), dtype=torch.float64, device=ctx.torch_device)
    ctx.gp_posterior_cov(gp.X, gp.cholesky_inverse, gp.alpha, gp.kern._factors(p), _gp_prior_row(gp), d_points,
                         SAMPLE_JITTER, d_mean, d_cov)
    pivot = ctx.cholesky(d_cov)
    if pivot:
        raise np.linalg.LinAlgError('%s: the covariance of the %d points (plus %g on its diagonal) is not positive '
                                    'definite: pivot %d is not positive' % (who, n_points, SAMPLE_JITTER, pivot))
    return d_points, d_mean, d_cov


class GPSampleFunction(object):
    """One sample path of a GP as a function: ``f(states, actions, ..., noise=True) -> [M, 1]``.

    As in the reference (``functions.py:1641-1649``) the path is evaluated as ``mean_function(x) +
    K(x, discretization) . alpha`` with the PRIOR kernel and ``alpha = (cov + 1e-8 I)^-1 . values`` - also when the
    GP holds observations, whose posterior the values were drawn from (bug-compatible).  The kernel, the mean
    function and the noise variance are read from the GP at every call.  The inputs are concatenated;
    NumPy in gives NumPy out, device tensors in give device tensors out.  ``noise=True`` adds
    ``sqrt(likelihood_variance) * np.random.standard_normal`` (NumPy's global generator).

    Attributes: ``alpha [N]``, ``discretization [N, p]``, ``values [N]`` (the sample at the discretization)."""

    def __init__(self, discretization, gpfun, alpha, values):
        self.discretization, self.gpfun = discretization, gpfun
        self.alpha = np.ascontiguousarray(alpha, dtype=config.np_dtype).reshape(-1)
        self.values = np.ascontiguousarray(values, dtype=config.np_dtype).reshape(-1)
        if len(self.alpha) != len(discretization) or len(self.values) != len(discretization):
            raise ValueError('alpha and values need one entry per point of the discretization')
        self._device = None

    @classmethod
    def from_values(cls, discretization, gpfun, values):
        """The sample functions whose values at the discretization are the rows of ``values [number, N]`` (one
        row: ``[N]``) -> a list, like ``sample_gp_function`` returns."""
        from . import _evaluate
        import torch
        who = 'GPSampleFunction.from_values'
        points, gp = _sample_setup(discretization, gpfun, who)
        values = np.atleast_2d(np.asarray(values, dtype=config.np_dtype))
        if values.shape[1] != len(points):
            raise ValueError('%s: values must be [number, %d], got %s' % (who, len(points), values.shape))
        ctx = _evaluate._ctx()
        _, _, d_chol = _sample_factor(ctx, points, gp, who)
        d_alpha = torch.from_numpy(np.ascontiguousarray(values.T)).to(ctx.torch_device)
        ctx.tri_solve(d_chol, d_alpha, False)
        ctx.tri_solve(d_chol, d_alpha, True)
        alpha = d_alpha.cpu().numpy()
        return [cls(points, gpfun, alpha[:, i], values[i]) for i in range(len(values))]

    def __call__(self, *points, **kwargs):
        from . import _evaluate
        import torch
        noise = kwargs.pop('noise', True)
        if kwargs:
            raise TypeError('unexpected keyword arguments %s' % sorted(kwargs))
        if not points:
            raise TypeError('a sample function needs the points to evaluate')
        ctx = _evaluate._ctx()
        on_device = any(isinstance(x, torch.Tensor) for x in points)
        parts = [_evaluate._to_device(ctx, x) for x in points]
        d_points = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1).contiguous()
        p = self.discretization.shape[1]
        if d_points.shape[1] != p:
            raise ValueError('the sample function expects %d inputs, the points have %d columns' % (p, d_points.shape[1]))
        if self._device is None or self._device[0] is not ctx:
            self._device = (ctx, torch.from_numpy(self.discretization).to(ctx.torch_device),
                            torch.from_numpy(self.alpha[:, None].copy()).to(ctx.torch_device))
        gp = self.gpfun.gaussian_process
        d_out = torch.empty((d_points.shape[0], 1), dtype=torch.float64, device=ctx.torch_device)
        ctx.gp_sample_eval(gp.kern._factors(p), _gp_prior_row(gp), self._device[1], self._device[2], d_points, d_out)
        if noise:
            draws = np.sqrt(gp.likelihood_variance) * np.random.standard_normal(tuple(d_out.shape))
            d_out += torch.from_numpy(draws).to(ctx.torch_device)
        return d_out if on_device else d_out.cpu().numpy()


def sample_gp_function(discretization, gpfun, number=1, return_function=True, standard_normal=None):
    """Sample paths of a GP on a discretization (``functions.py:1586-1662``), factored on the GPU.

    ``discretization`` is a ``GridWorld`` (its ``all_points``) or an ``[N, p]`` array, ``gpfun`` a
    ``GaussianProcess`` with one output.  The samples are ``mean + L z`` with ``mean``, ``cov`` the GP's posterior
    at the discretization (``build_predict(..., full_cov=True)``), ``L`` the Cholesky factor of ``cov + 1e-8 I`` and
    ``z = np.random.standard_normal((number, N))`` from NumPy's global generator (``np.random.seed`` makes a run
    repeatable), or the ``standard_normal [number, N]`` given.  The reference draws the same distribution through
    ``np.random.multivariate_normal`` (an SVD of ``cov``), so after the same seed its NUMBERS differ from these; only
    the distribution is the same.

    ``return_function=False`` returns the ``[number, N]`` array of samples; otherwise a list of ``number``
    :class:`GPSampleFunction` objects, ``f(states, actions, ..., noise=True)``.  A covariance that cannot be factored
    raises ``np.linalg.LinAlgError`` naming the pivot.  One GPU only: ``NotImplementedError`` under
    ``torch.distributed`` with more than one rank."""
    from . import _evaluate
    import torch
    who = 'sample_gp_function'
    points, gp = _sample_setup(discretization, gpfun, who)
    number = int(number)
    if number < 1:
        raise ValueError('%s: number must be at least 1, got %d' % (who, number))
    n_points = len(points)
    if standard_normal is None:
        standard_normal = np.random.standard_normal((number, n_points))
    else:
        standard_normal = np.asarray(standard_normal, dtype=config.np_dtype)
        if standard_normal.shape != (number, n_points):
            raise ValueError('%s: standard_normal must be [%d, %d], got %s'
                             % (who, number, n_points, standard_normal.shape))
    ctx = _evaluate._ctx()
    _, d_mean, d_chol = _sample_factor(ctx, points, gp, who)
    d_normal = torch.from_numpy(np.ascontiguousarray(standard_normal.T)).to(ctx.torch_device)
    d_values = torch.empty_like(d_normal)
    ctx.tri_mult(d_chol, d_normal, d_mean, d_values)
    values = np.ascontiguousarray(d_values.cpu().numpy().T)
    if not return_function:
        return values
    ctx.tri_solve(d_chol, d_values, False)
    ctx.tri_solve(d_chol, d_values, True)
    alpha = d_values.cpu().numpy()
    return [GPSampleFunction(points, gpfun, alpha[:, i], values[i]) for i in range(number)]
