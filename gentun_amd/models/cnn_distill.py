"""Knowledge distillation for Genetic-CNN: fit one student on a teacher's probabilities.

A fitted :class:`~gentun_amd.models.cnn_fitted.CnnClassifier` or a
:class:`~gentun_amd.models.cnn_ensemble.CnnEnsemble` is the teacher. :func:`soft_targets` turns its
predictions for the training rows into a table of target rows, and :func:`distill` fits a student on that
table through ``GeneticCnnModel.fit(soft_targets=...)`` -- the soft-target training step of both executors
(:mod:`gentun_amd.models.cnn_engine`, "The target row"; ``gt_head_soft`` on the MI355X).

The targets. With the teacher's fp32 logits ``z`` taken to fp64::

    q = softmax(z / T)                               a classifier
    q = sum_m w_m * softmax(z_m / T)                 an ensemble: its own normalised weights, member order
    t = (1 - alpha) * onehot(y) + alpha * q          fp64, rounded once to fp32

Only the teacher's softmax has a temperature: the student trains at temperature 1.
"""

import math

import numpy as np

from .cnn_ensemble import CnnEnsemble
from .cnn_fitted import CnnClassifier


def _check_blend(alpha, temperature):
    for name, v in (("alpha", alpha), ("temperature", temperature)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("{} must be a real number".format(name))
    alpha, temperature = float(alpha), float(temperature)
    if not (0.0 <= alpha <= 1.0):
        raise ValueError("alpha must be in [0, 1], got {}".format(alpha))
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError("temperature must be finite and positive, got {}".format(temperature))
    return alpha, temperature


def _softmax64(z):
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=-1, keepdims=True)


def soft_targets(teacher, x, y_onehot, alpha=0.5, temperature=1.0, device=None, batch=256):
    """The fp32 ``[n, C]`` target rows ``(1 - alpha) * onehot + alpha * q`` of a teacher (see the module
    text). ``ValueError`` on an ``alpha`` outside ``[0, 1]``, a ``temperature`` that is not finite and
    positive, a teacher that is neither a ``CnnClassifier`` nor a ``CnnEnsemble``, labels that are not
    one-hot ``[n, C]`` with the teacher's ``C``, and images that are not the teacher's input shape."""
    alpha, temperature = _check_blend(alpha, temperature)
    if not isinstance(teacher, (CnnClassifier, CnnEnsemble)):
        raise ValueError("teacher must be a CnnClassifier or a CnnEnsemble, got {}".format(type(teacher).__name__))
    y = np.asarray(y_onehot)
    if y.ndim != 2 or y.dtype == object or y.dtype.kind not in "fiub":
        raise ValueError("y_onehot must be a one-hot array [n, classes]")
    if y.shape[1] != teacher.classes:
        raise ValueError("y_onehot has {} classes, the teacher {}".format(y.shape[1], teacher.classes))
    x = np.asarray(x)
    if x.ndim != 4 or tuple(x.shape[1:]) != tuple(teacher.input_shape):
        raise ValueError("x must be [n, {}, {}, {}] (the teacher's input shape), got {}".format(
            *(tuple(teacher.input_shape) + (list(x.shape),))))
    if x.shape[0] != y.shape[0]:
        raise ValueError("x has {} rows, y_onehot {}".format(x.shape[0], y.shape[0]))
    onehot = np.zeros(y.shape, np.float64)
    onehot[np.arange(y.shape[0]), np.argmax(y, axis=1)] = 1.0
    if isinstance(teacher, CnnEnsemble):
        logits = np.asarray(teacher.predict(x, output="member_logits", device=device, batch=batch), np.float32)
        q = np.zeros(y.shape, np.float64)
        for m in range(logits.shape[0]):                       # member order
            q = q + np.float64(teacher.weights[m]) * _softmax64(logits[m].astype(np.float64) / temperature)
    else:
        logits = np.asarray(teacher.predict(x, output="logits", device=device, batch=batch), np.float32)
        q = _softmax64(logits.astype(np.float64) / temperature)
    t = (1.0 - alpha) * onehot + alpha * q
    return np.ascontiguousarray(t.astype(np.float32))


def distill(teacher, x, y_onehot, genes, alpha=0.5, temperature=1.0, device=None, **additional_parameters):
    """Fit a student with ``genes`` on every row of ``x`` against :func:`soft_targets` of ``teacher`` and
    return it as a ``CnnClassifier``. ``additional_parameters`` are what ``GeneticCnnModel`` takes (the
    search's settings); the student's ``metrics`` are those of ``fit()``: against the hard labels."""
    from .cnn import GeneticCnnModel
    table = soft_targets(teacher, x, y_onehot, alpha=alpha, temperature=temperature, device=device)
    model = GeneticCnnModel(x, y_onehot, genes, device=device, **additional_parameters)
    return model.fit(soft_targets=table)
