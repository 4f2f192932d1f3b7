#!/usr/bin/env python
"""RISE saliency of a fitted Genetic-CNN: fit one genome on synthetic glyph images, then ask for a few held-out
images which pixels the prediction rests on -- ``rise`` blends the image with zeros under random soft masks and
weights every mask by the probability the predicted class keeps. Prints a text heat map per image (darker glyph:
the class holds up where this pixel is kept) and one JSON line.

usage: python examples/cnn_rise.py [--device cpu|cuda:0] [--masks 512] [--cells 4] [--images 3]"""
import argparse
import json

import _common

RAMP = " .:*#@"

if __name__ == "__main__":
    import numpy as np
    import torch
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.utils.data import make_glyph_classification

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--masks", type=int, default=None)
    ap.add_argument("--cells", type=int, default=4)
    ap.add_argument("--images", type=int, default=3)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    n = 224 if _common.SMALL else 960
    masks = args.masks or (64 if _common.SMALL else 512)
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    held = args.images
    model = GeneticCnnModel(x[held:], y[held:], {"S_1": "101", "S_2": "110"}, nodes=(3, 3), input_shape=shape,
                            kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)), dense_units=32,
                            dropout_probability=0.5, classes=classes, nfold=2,
                            epochs=(1,) if _common.SMALL else (6,), learning_rate=(3e-3,), batch_size=32,
                            loss="ce", seed=0, device=args.device)
    model.fit()
    maps, info = model.rise(x[:held], masks=masks, cells=args.cells, return_info=True)
    for r in range(held):
        print("image {}: class {} (true {}), probability {:.3f}".format(
            r, int(info["target"][r]), int(y[r].argmax()), float(info["base"][r])))
        lo, hi = float(maps[r].min()), float(maps[r].max())
        for row in maps[r]:
            print("  " + "".join(RAMP[min(len(RAMP) - 1, int(len(RAMP) * (v - lo) / max(hi - lo, 1e-12)))]
                                 for v in row))
    print(json.dumps({"images": int(held), "shape": list(maps.shape[1:]), "masks": masks, "cells": args.cells,
                      "largest": float(maps.max())}))
