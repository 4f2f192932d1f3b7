"""Fitness models: Genetic-CNN (HIP kernels on MI355X) and GBDT (native C++/HIP engine)."""

from .generic_models import GentunModel  # noqa: F401
from .cnn_ensemble import CnnEnsemble, fit_ensemble  # noqa: F401
from .cnn_distill import distill, soft_targets  # noqa: F401
