from .dual_averaging import HMCDATuner, PerChainDATuner, Tuner
from .windowed import WindowedAdaptation
