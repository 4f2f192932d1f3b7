#!/usr/bin/env python
"""Distil a Genetic-CNN ensemble into one network: fit a k = 3 ensemble on glyph images, then a student with
the first member's genes three ways -- on the hard labels, on smoothed labels (``label_smoothing=0.1``) and on
a blend of the hard labels and the ensemble's probabilities (``CnnEnsemble.distill``). Prints one JSON line
with the held-out categorical accuracy of the teacher and of the three students.

usage: python examples/cnn_distill.py [--device cpu|cuda:0] [--alpha 0.5] [--temperature 2.0]"""
import argparse
import json

import _common

if __name__ == "__main__":
    import numpy as np
    import torch
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.utils.data import make_glyph_classification

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=2.0)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    n = 160 if _common.SMALL else 800
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    ntr = n * 3 // 4
    xtr, ytr, xte, lte = x[:ntr], y[:ntr], x[ntr:], np.argmax(y[ntr:], 1)
    space = dict(nodes=(3, 3), input_shape=shape, kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)),
                 dense_units=32, dropout_probability=0.5, classes=classes, nfold=2,
                 epochs=(1,) if _common.SMALL else (6,), learning_rate=(3e-3,), batch_size=32, loss="ce", seed=0)
    genomes = [{"S_1": "101", "S_2": "110"}, {"S_1": "011", "S_2": "101"}, {"S_1": "111", "S_2": "011"}]

    def held_out(model):
        return float((model.predict(xte, output="label", device=args.device) == lte).mean())

    teacher = fit_ensemble(xtr, ytr, genomes, device=args.device, **space)
    out = {"teacher": held_out(teacher),
           "plain": held_out(GeneticCnnModel(xtr, ytr, genomes[0], device=args.device, **space).fit()),
           "smoothed": held_out(GeneticCnnModel(xtr, ytr, genomes[0], device=args.device, label_smoothing=0.1,
                                                **space).fit()),
           "distilled": held_out(teacher.distill(xtr, ytr, alpha=args.alpha, temperature=args.temperature,
                                                 device=args.device, **space))}
    print(json.dumps(out))
