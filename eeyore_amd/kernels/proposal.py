"""Proposal densities behind the reference's names (``Kernel``, ``NormalizedKernel``, ``NormalKernel``;
eeyore/kernels/{kernel,normalized_kernel,normal_kernel}.py).

Inside the samplers the proposal draw and its log-density are part of the fused HIP step (``ey_mala_step`` /
``ey_mh_step`` / ``ey_mh_tril_step``); a ``NormalKernel`` or ``MultivariateNormalKernel`` object is how a script hands the
proposal scale or factor to ``MetropolisHastings`` and how it can inspect or evaluate the proposal density of the current
state."""
import torch
from torch.distributions import MultivariateNormal, Normal


class Kernel:
    """k(x1, x2): a kernel evaluated at a pair of points, and its matrices and sums over samples (eeyore/kernels/kernel.py:
    ``K``, ``symm_K``, ``sum_K``, ``sum_symm_K``).  A sample is a list of ``[p]`` tensors, as ``chain.vals['sample'][0:n]``
    is, or an ``[n, p]`` tensor.  The homogeneous kernels of ``kernels.homogeneous`` evaluate all pairs at once (and their
    sums of samples on the ROCm device in the HIP kernel ``ey_kernel_pair_sums``); a subclass that only defines ``k`` is
    served pair by pair."""

    def k(self, x1, x2):
        raise NotImplementedError

    # ---- input checks (the reference's names)
    def check_input_dtype(self, x, dtype):
        if not all(e.dtype == dtype for e in x):
            raise ValueError("the elements of the sample differ in dtype")

    def check_inputs_dtype(self, x1, x2, dtype):
        self.check_input_dtype(x1, dtype)
        self.check_input_dtype(x2, dtype)

    def check_input_device(self, x, device):
        if not all(e.device == device for e in x):
            raise ValueError("the elements of the sample differ in device")

    def check_inputs_device(self, x1, x2, device):
        self.check_input_device(x1, device)
        self.check_input_device(x2, device)

    def _checked(self, xs, check_input):
        first = xs[0][0]
        if check_input:
            for x in xs:
                self.check_input_dtype(x, first.dtype)
                self.check_input_device(x, first.device)
        return first.dtype, first.device

    def _all_pairs(self, x1, x2):
        """[n1, n2] values of k in f64 for every pair at once, or None: then k is called pair by pair."""
        return None

    def _pair_sums(self, x1, x2, include_diag):
        """(sum_symm_K(x1), sum_symm_K(x2), sum_K(x1, x2)) as f64 scalars without a matrix, or None.  ``x2=None``: only the
        first is wanted (the other two are then whatever is cheapest)."""
        return None

    def K(self, x1, x2, check_input=False):
        """[n1, n2] matrix of k(x1[i], x2[j])."""
        dtype, device = self._checked((x1, x2), check_input)
        m = self._all_pairs(x1, x2)
        if m is None:
            m = torch.stack([torch.stack([torch.as_tensor(self.k(a, b)).reshape(()) for b in x2]) for a in x1])
        return m.to(dtype=dtype, device=device)

    def symm_K(self, x, check_input=False):
        """[n, n] matrix of k(x[i], x[j]); the lower triangle mirrors the upper one."""
        dtype, device = self._checked((x,), check_input)
        m = self._all_pairs(x, x)
        if m is None:
            n = len(x)
            upper = {(i, j): torch.as_tensor(self.k(x[i], x[j])).reshape(()) for i in range(n) for j in range(i, n)}
            m = torch.stack([torch.stack([upper[(min(i, j), max(i, j))] for j in range(n)]) for i in range(n)])
        else:
            m = torch.triu(m) + torch.triu(m, 1).mT
        return m.to(dtype=dtype, device=device)

    def sum_symm_K(self, x, include_diag=True, check_input=False):
        """Sum of symm_K(x), with or without its diagonal -> tensor of shape [1]."""
        dtype, device = self._checked((x,), check_input)
        sums = self._pair_sums(x, None, include_diag)
        if sums is not None:
            total = sums[0]
        else:
            m = self._all_pairs(x, x)
            if m is not None:
                total = 2.0 * torch.tril(m, -1).sum() + (torch.diagonal(m).sum() if include_diag else 0.0)
            else:
                n = len(x)
                total = sum((2.0 * torch.as_tensor(self.k(x[i], x[j])).reshape(()) for i in range(n) for j in range(i)),
                            torch.zeros((), dtype=dtype, device=device))
                if include_diag:
                    total = total + sum(torch.as_tensor(self.k(e, e)).reshape(()) for e in x)
        return torch.as_tensor(total).reshape(1).to(dtype=dtype, device=device)

    def sum_K(self, x1, x2, check_input=False):
        """Sum of K(x1, x2) -> tensor of shape [1]."""
        dtype, device = self._checked((x1, x2), check_input)
        sums = self._pair_sums(x1, x2, True)
        if sums is not None:
            total = sums[2]
        else:
            m = self._all_pairs(x1, x2)
            if m is not None:
                total = m.sum()
            else:
                total = sum((torch.as_tensor(self.k(a, b)).reshape(()) for a in x1 for b in x2),
                            torch.zeros((), dtype=dtype, device=device))
        return torch.as_tensor(total).reshape(1).to(dtype=dtype, device=device)


class NormalizedKernel(Kernel):
    """A kernel that is a probability density in its first argument: wraps a torch distribution as ``density``;
    ``log_prob`` sums the elementwise log-densities (normalized_kernel.py:14-15)."""

    density = None

    def log_prob(self, state):
        return self.density.log_prob(state).sum()

    def sample(self):
        return self.density.sample()


class NormalKernel(NormalizedKernel):
    """Independent normals N(loc_i, scale_i)."""

    def __init__(self, loc, scale):
        self.set_density(loc, scale)

    def set_density(self, loc, scale):
        self.density = Normal(loc, scale)

    def set_density_params(self, loc, scale=None):
        """Re-centre (and optionally re-scale) the existing density in place."""
        self.density.loc = loc
        if scale is not None:
            self.density.scale = scale

    def k(self, x1, x2, scale=None):
        """Density of x1 under the kernel centred at x2."""
        self.set_density_params(x2, scale=scale)
        return torch.exp(self.log_prob(x1))


def check_scale_tril(t, P):
    """Refuse a proposal factor that ``ey_mh_tril_step`` cannot use: ``t`` must be a ``[P, P]`` or ``[G, P, P]`` tensor
    whose lower triangles are finite with a positive diagonal (the strict upper triangle is never read)."""
    if not torch.is_tensor(t) or t.dim() not in (2, 3) or tuple(t.shape[-2:]) != (P, P) or t.shape[0] < 1:
        shape = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"scale_tril must be a [{P}, {P}] or [G, {P}, {P}] tensor, got {shape}")
    if not bool(torch.isfinite(torch.tril(t)).all()):
        raise ValueError("scale_tril has a non-finite entry in its lower triangle")
    if not bool((torch.diagonal(t, dim1=-2, dim2=-1) > 0).all()):
        raise ValueError("scale_tril must have a positive diagonal")


class MultivariateNormalKernel(NormalizedKernel):
    """N(loc, L L^T) with the lower-triangular factor ``scale_tril`` = L (eeyore/kernels/multivariate_normal_kernel.py).
    ``scale_tril`` keeps the factor as it was given, ``[P, P]`` or ``[C, P, P]``: a batched ``loc`` makes torch broadcast
    the density's own copy, and ``MetropolisHastings`` must see the caller's shape."""

    def __init__(self, loc, scale_tril):
        self.set_density(loc, scale_tril)

    @property
    def scale_tril(self):
        return self._scale_tril

    def set_density(self, loc, scale_tril):
        self._scale_tril = scale_tril
        self.density = MultivariateNormal(loc, scale_tril=scale_tril)

    def set_density_params(self, loc, scale_tril=None):
        """Re-centre the density; a new factor rebuilds it (assigning ``density.scale_tril``, as the reference does,
        changes nothing ``rsample`` reads)."""
        if scale_tril is not None:
            self.set_density(loc, scale_tril)
        elif loc.shape != self.density.loc.shape:  # another batch of chains: the batch shape is fixed at construction
            self.set_density(loc, self._scale_tril)
        else:
            self.density.loc = loc

    def log_prob(self, state):
        return self.density.log_prob(state).sum()

    def k(self, x1, x2, scale_tril=None):
        """Density of x1 under the kernel centred at x2."""
        self.set_density_params(x2, scale_tril=scale_tril)
        return torch.exp(self.log_prob(x1))
