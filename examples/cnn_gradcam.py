#!/usr/bin/env python
"""Grad-CAM of a fitted Genetic-CNN: fit one genome on synthetic glyph images, then ask for a few held-out images
which regions of the last feature map speak for the predicted class -- ``gradcam`` weighs the map's channels by
the mean gradient of the class score and sums them: one forward per image, where ``occlusion`` needs one per grid
cell. Prints a coarse text heat map per image (darker glyph: stronger support), upsampled to the image with
``--upsample``, and one JSON line.

usage: python examples/cnn_gradcam.py [--device cpu|cuda:0] [--score logit|proba] [--upsample] [--images 3]"""
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
    ap.add_argument("--score", default="logit", choices=("logit", "proba"))
    ap.add_argument("--upsample", action="store_true")
    ap.add_argument("--images", type=int, default=3)
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
    maps, info = model.gradcam(x[:held], score=args.score, upsample=args.upsample, return_info=True)
    top = max(float(maps.max()), 1e-12)
    for r in range(held):
        print("image {}: class {} (true {}), {} {:.3f}".format(
            r, int(info["target"][r]), int(y[r].argmax()), args.score, float(info["base"][r])))
        for row in maps[r]:
            print("  " + "".join(RAMP[min(len(RAMP) - 1, int(len(RAMP) * v / top))] for v in row))
    print(json.dumps({"images": int(held), "map": list(maps.shape[1:]), "score": args.score,
                      "upsample": bool(args.upsample), "largest": float(maps.max())}))
