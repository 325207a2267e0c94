from .base import Sampler, SerialSampler, SingleChainSerialSampler
from .hmc import HMC
from .nuts import NUTS
from .metric import DenseMetric, DiagMetric
from .mala import MALA
from .metropolis_hastings import MetropolisHastings
from .power_posterior_sampler import PowerPosteriorSampler
from .ram import RAM
from .gibbs import Gibbs
from .am import AM, Ridge, SoftAbs
from .elliptical_slice import EllipticalSlice
