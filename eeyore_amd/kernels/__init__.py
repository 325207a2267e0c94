from .proposal import Kernel, NormalizedKernel, NormalKernel, MultivariateNormalKernel, check_scale_tril
from .homogeneous import HomogeneousKernel, IsoSEKernel, RQKernel, PeriodicKernel
