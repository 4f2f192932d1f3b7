#!/usr/bin/env python
"""Genetic-CNN cross-validation with and without the paper's training augmentation (a random translation
with zero fill and a random horizontal flip, ``augment={"shift": s, "flip": True}``): the same genome, seed
and folds, once on the raw images and once on images re-drawn every step on the device. Evaluation always
sees the raw images. Prints one JSON line with both fitness values.

usage: python examples/cnn_augment.py [--device cpu|cuda:0] [--shift 2]"""
import argparse
import json

import _common

if __name__ == "__main__":
    import numpy as np
    import torch
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.utils.data import make_glyph_classification

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--shift", type=int, default=2)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    x, y = make_glyph_classification(n=160 if _common.SMALL else 640, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    out = {}
    for name, aug in (("plain", None), ("augmented", {"shift": args.shift, "flip": True})):
        model = GeneticCnnModel(x, y, {"S_1": "101", "S_2": "110"}, nodes=(3, 3), input_shape=shape,
                                kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)), dense_units=32,
                                dropout_probability=0.5, classes=classes, nfold=2,
                                epochs=(1,) if _common.SMALL else (6,), learning_rate=(3e-3,), batch_size=32,
                                loss="ce", seed=0, device=args.device, augment=aug)
        out[name] = model.cross_validate()
    print(json.dumps(out))
