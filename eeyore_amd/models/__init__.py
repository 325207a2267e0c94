from .base import Model, LogTargetModel, BayesianModel
from .mlp import MLP, Hyperparameters
from . import mlp
from .logistic_regression import LogisticRegression
from . import logistic_regression
from .distribution_model import DistributionModel
from .targets import NormalMixture, MultivariateNormal
from .targets import ExponentialTilt, LogGamma, LogInverseGamma, LogWeibull, Gumbel
from . import targets
