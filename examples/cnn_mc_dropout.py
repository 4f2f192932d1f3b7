#!/usr/bin/env python
"""Monte-Carlo dropout of a fitted Genetic-CNN: fit one genome on synthetic glyph images, then sample the dropout
of its dense head a few dozen times per image (``predict_mc``) and compare how unsure the model is about held-out
glyphs and about uniform noise, which it has never seen: the mutual information between the prediction and the
dropout mask (BALD) is what the disagreement of the samples adds to the entropy. Prints one JSON line.

usage: python examples/cnn_mc_dropout.py [--device cpu|cuda:0] [--samples 32] [--images 64]"""
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
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--images", type=int, default=64)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    n = 224 if _common.SMALL else 960
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    held = args.images
    model = GeneticCnnModel(x[held:], y[held:], {"S_1": "101", "S_2": "110"}, nodes=(3, 3), input_shape=shape,
                            kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)), dense_units=32,
                            dropout_probability=0.5, classes=classes, nfold=2,
                            epochs=(1,) if _common.SMALL else (6,), learning_rate=(3e-3,), batch_size=32,
                            loss="ce", seed=0, device=args.device)
    model.fit()
    lo, hi = float(x.min()), float(x.max())
    noise = np.random.default_rng(1).uniform(lo, hi, (held,) + shape).astype(np.float32)
    seen = model.predict_mc(x[:held], samples=args.samples)          # the model's own dropout_probability
    unseen = model.predict_mc(noise, samples=args.samples)
    print(json.dumps({"images": int(held), "samples": int(args.samples),
                      "accuracy": float((seen["label"] == y[:held].argmax(1)).mean()),
                      "mutual_info_held_out": float(seen["mutual_info"].mean()),
                      "mutual_info_noise": float(unseen["mutual_info"].mean())}))
