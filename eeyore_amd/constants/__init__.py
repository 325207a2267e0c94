from .constants import (Loss, gaussian_loss, laplace_loss, loss_functions, poisson_loss,  # noqa: F401
                        torch_to_np_types)
