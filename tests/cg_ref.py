"""Host image of the resident SCG / GD vectors (csrc/cg.hip: gp_cg_update, gp_cg_dots, gp_cg_abs, gp_cg_max_d; the trial point of csrc/psi.hip).

``NumpyOps``   the reference's helper names (scg_adapted_local_MapReduce.py:29-243, gd_local_MapReduce.py:14-105) on one in-memory vector: what an
               optimiser is handed where no device is involved.  ``FsumOps`` is the same with every reduction through math.fsum (another summation
               order: the yardstick of the trajectory test).
``Image``      one shard's vectors d, g_new, g_old, g_latest (2 N Q,) and X = [mu | S as stored] (2 N Q,), with the reference's assignments stated
               exactly as the reference computes them in NumPy (a product, then a sum: two roundings), the number ``which`` of gp_cg_update next to
               each, and the reductions as numpy.longdouble sums together with sum |term|.
The exact candidates of the two multiply-add forms (``fused`` by fractions.Fraction, ``two_roundings`` by NumPy), the chain length of the device's
summation order (``chain``) and the longdouble softplus and its slope are here as well, so that the CPU test and the GPU test share one statement."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


class NumpyOps(object):
    """Per-point part X (shape (n,)) with the reference's trial-point protocol: the objective is evaluated at X + step*d."""

    def __init__(self, X0):
        self.X = X0.copy()
        self.latest = np.zeros_like(X0)
        self.new = self.old = self.d = None

    # scg_adapted_local_MapReduce.py / gd_local_MapReduce.py names
    def embeddings_set_grads(self, folder=None):
        self.new, self.old, self.d = self.latest.copy(), self.latest.copy(), -self.latest

    def embeddings_get_grads_mu(self, folder=None):
        return float(np.dot(self.new, self.d))

    def embeddings_get_grads_kappa(self, folder=None):
        return float(np.dot(self.d, self.d))

    def embeddings_get_grads_theta(self, folder=None):
        return float(np.dot(self.d, self.latest - self.new))

    def embeddings_get_grads_current_grad(self, folder=None):
        return float(np.dot(self.new, self.new)) if not self.gd else float(np.sum(np.abs(self.new)))

    def embeddings_get_grads_gamma(self, folder=None):      # sum grad_new * grad_old (:128-140); |grad_new|^2 is in current_grad
        return float(np.dot(self.new, self.old))

    def embeddings_get_grads_max_d(self, folder, alpha):
        return float(np.max(np.abs(alpha * self.d)))

    def embeddings_get_grads_max_gradnow(self, folder=None):
        return float(np.max(np.abs(self.new)))

    def embeddings_set_grads_reset_d(self, folder=None):
        self.d = -self.new

    def embeddings_set_grads_update_d(self, folder, gamma):
        self.d = (gamma * self.d - self.new) if not self.gd else -(self.new + gamma * self.d)

    def embeddings_set_grads_update_X(self, folder, alpha):
        self.X = self.X + alpha * self.d

    def embeddings_set_grads_update_grad_old(self, folder=None):
        self.old = self.new.copy()

    def embeddings_set_grads_update_grad_new(self, folder=None):
        self.new = self.latest.copy()

    embeddings_set_grads_update_grad_now = embeddings_set_grads_update_grad_new
    gd = False


class FsumOps(NumpyOps):
    """NumpyOps with every sum formed by math.fsum (correctly rounded) instead of numpy.dot / numpy.sum: the same algebra in another summation order."""

    def embeddings_get_grads_mu(self, folder=None):
        return math.fsum(self.new * self.d)

    def embeddings_get_grads_kappa(self, folder=None):
        return math.fsum(self.d * self.d)

    def embeddings_get_grads_theta(self, folder=None):
        return math.fsum(self.d * (self.latest - self.new))

    def embeddings_get_grads_current_grad(self, folder=None):
        return math.fsum(self.new * self.new) if not self.gd else math.fsum(np.abs(self.new))

    def embeddings_get_grads_gamma(self, folder=None):
        return math.fsum(self.new * self.old)


# ---- the two candidates of a multiply-add ----------------------------------------------------------------------------------------------
def two_roundings(a, d, other, sign=1.0):
    """fl(fl(a d) + sign other): what NumPy, and a build that does not contract, computes."""
    return a * np.asarray(d, dtype=np.float64) + sign * np.asarray(other, dtype=np.float64)


def fused(a, d, other, sign=1.0):
    """The correctly rounded a d + sign other (one rounding: what a fused multiply-add gives), exactly, element by element.  Where a is zero or
    a power of two the product is exact and the two candidates are one (no element here is near the underflow threshold)."""
    if a == 0.0 or abs(math.frexp(float(a))[0]) == 0.5:
        return two_roundings(a, d, other, sign)
    fa, s = Fraction(float(a)), int(sign)
    return np.array([float(fa * Fraction(float(x)) + s * Fraction(float(y))) for x, y in zip(np.ravel(d), np.ravel(other))])


def sample_indices(n2, nq, grid_cap=8192, want=4096, seed=0):
    """Indices of a (n2,) vector: all of them up to ``want``; beyond, the first, the last, nq - 1, nq (the mu / S split), both sides of every
    256-element block boundary and of every stride boundary of a grid-stride loop capped at ``grid_cap`` blocks, filled up with random ones."""
    if n2 <= want:
        return np.arange(n2)
    idx = {0, n2 - 1, nq - 1, min(nq, n2 - 1)}
    for b in range(256, n2, 256):
        idx.update((b - 1, b))
    stride = min((n2 + 255) // 256, grid_cap) * 256
    for b in range(stride, n2, stride):
        idx.update((b - 1, b))
    rng = np.random.RandomState(seed)
    fill = rng.randint(0, n2, size=max(want, 1024))
    return np.unique(np.concatenate([np.fromiter(idx, dtype=np.int64), fill]))


def ulps(got, ref):
    """|got - ref| in units in the last place of ref, elementwise."""
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.spacing(np.abs(ref))


# ---- the variance transform in extended precision ----------------------------------------------------------------------------------------
def softplus_ld(x):
    """log(1 + exp(x)) in numpy.longdouble (transformVar, supporting_functions.py:160-163)."""
    return np.log1p(np.exp(np.asarray(x, dtype=LD)))


def sigma_ld(x):
    """1 / (1 + exp(-x)) in numpy.longdouble (transformVar_grad, supporting_functions.py:165-168)."""
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=LD)))


# ---- the reductions ------------------------------------------------------------------------------------------------------------------------
def gamma_n(n):
    """Higham's gamma_n = n u / (1 - n u) (the convention of tests/lbfgs_ref.py and tests/gemm_ref.py)."""
    return n * U / (1.0 - n * U)


def reduce_blocks(n2):
    return min((n2 + 255) // 256, 1024)


def chain(n2):
    """The longest chain of additions in cg_reduce's stated order: a thread's ceil(n2 / (nb 256)) terms, 8 levels of block_fold<256>, then the nb
    block partials added on the host in ascending order (nb - 1 additions), nb = min(ceil(n2 / 256), 1024)."""
    nb = reduce_blocks(n2)
    return (n2 + nb * 256 - 1) // (nb * 256) + 8 + nb - 1


DOT_NAMES = ('mu', 'kappa', 'theta', 'current_grad', 'gamma')


class Image(object):
    """One shard's resident vectors on the host.  X = [mu | S as stored] like the direction: the first N Q entries move the means, the rest the
    variances (scg_adapted_local_MapReduce.py:202-211: grad_d[0], grad_d[1])."""

    def __init__(self, X_mu, X_S, d=None, new=None, old=None, latest=None):
        self.shape = np.shape(X_mu)
        self.nq = int(np.size(X_mu))
        self.X = np.concatenate([np.ravel(X_mu), np.ravel(X_S)]).astype(np.float64)
        z = lambda v: np.zeros(2 * self.nq) if v is None else np.array(v, dtype=np.float64).ravel()      # noqa: E731
        self.d, self.new, self.old, self.latest = z(d), z(new), z(old), z(latest)

    @property
    def X_mu(self):
        return self.X[:self.nq].reshape(self.shape)

    @property
    def X_S(self):
        return self.X[self.nq:].reshape(self.shape)

    def copy(self):
        return Image(self.X_mu, self.X_S, self.d, self.new, self.old, self.latest)

    def arrays(self):
        return dict(d=self.d, new=self.new, old=self.old, latest=self.latest, X=self.X)

    # the six assignments of scg_adapted_local_MapReduce.py, in gp_cg_update's numbering
    def reset_d(self):                      # which 0, :160-173
        self.d = -1 * self.new

    def update_d(self, gamma):              # which 1, :175-189
        self.d = gamma * self.d - self.new

    def update_X(self, alpha):              # which 2, :191-214
        self.X = self.X + alpha * self.d

    def update_grad_old(self):              # which 3, :216-229
        self.old = self.new.copy()

    def update_grad_new(self):              # which 4, :231-243
        self.new = self.latest.copy()

    def set_grads(self):                    # which 5, :29-55
        self.new, self.old, self.d = self.latest.copy(), self.latest.copy(), -1 * self.latest

    # gd_local_MapReduce.py: grad_now is g_new; there is no g_old
    def gd_set_grads(self):                 # :14-32
        self.new, self.d = self.latest.copy(), -1 * self.latest

    def gd_update_d(self, gamma):           # :63-74
        self.d = -(self.new + gamma * self.d)

    gd_update_X = update_X                  # :76-94
    gd_update_grad_now = update_grad_new    # :96-105

    def apply(self, which, a=0.0):
        (self.reset_d, lambda: self.update_d(a), lambda: self.update_X(a), self.update_grad_old, self.update_grad_new, self.set_grads)[which]()

    # the reductions: (values (longdouble), sum |term| (float)) in gp_cg_dots' order, and the maxima
    def terms(self):
        """The five term vectors as the kernel forms them from its double inputs; theta's difference is rounded to double first."""
        d, new = self.d.astype(LD), self.new.astype(LD)
        diff = (self.latest - self.new).astype(LD)
        return [new * d, d * d, d * diff, new * new, new * self.old.astype(LD)]

    def dots(self, keep=None):
        """``keep``: a slice of the elements that take part (the dropped-element demonstration)."""
        t = [p[keep] if keep is not None else p for p in self.terms()]
        return np.array([np.sum(p) for p in t], dtype=LD), np.array([float(np.sum(np.abs(p))) for p in t])

    def abs_sum(self, keep=None):
        a = np.abs(self.new).astype(LD)
        a = a[keep] if keep is not None else a
        return np.sum(a), float(np.sum(a))

    def max_d(self):
        return float(np.max(np.abs(self.d)))

    def max_new(self):
        return float(np.max(np.abs(self.new)))

    def bound(self, mags):
        return gamma_n(chain(2 * self.nq) + 2) * np.asarray(mags)
