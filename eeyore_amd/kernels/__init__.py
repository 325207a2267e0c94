from .proposal import Kernel, NormalizedKernel, NormalKernel
from .homogeneous import HomogeneousKernel, IsoSEKernel, RQKernel, PeriodicKernel
