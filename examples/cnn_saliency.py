#!/usr/bin/env python
"""Input-gradient saliency of a fitted Genetic-CNN: fit one genome on synthetic glyph images, then ask for a few
held-out images which pixels the predicted class's score depends on -- ``saliency`` differentiates the score with
respect to the input (``--method gradient`` / ``gradxinput``) or integrates that gradient along the straight path
from a baseline image (``--method integrated``, whose attributions add up to the score's change). ``--smooth S``
averages the gradient over ``S`` noisy copies of every image (SmoothGrad; ``--stat sq`` / ``var`` for SmoothGrad^2
and VarGrad). Prints a text heat map per image at input resolution and one JSON line.

usage: python examples/cnn_saliency.py [--device cpu|cuda:0] [--score logit|proba]
                                       [--method gradient|gradxinput|integrated] [--steps 16] [--images 3]
                                       [--smooth 0] [--noise 0.15] [--stat mean|sq|var]"""
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
    ap.add_argument("--method", default="integrated", choices=("gradient", "gradxinput", "integrated"))
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--smooth", type=int, default=0, help="noisy copies per image (0: none); not with integrated")
    ap.add_argument("--noise", type=float, default=0.15)
    ap.add_argument("--stat", default="mean", choices=("mean", "sq", "var"))
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
    smooth = {"samples": args.smooth, "noise": args.noise, "stat": args.stat} if args.smooth else None
    kw = dict(score=args.score, method=args.method, steps=args.steps, smooth=smooth)
    maps, info = model.saliency(x[:held], return_info=True, **kw)
    signed = model.saliency(x[:held], reduce="sum", **kw)
    top = max(float(maps.max()), 1e-12)
    gaps = []
    for r in range(held):
        print("image {}: class {} (true {}), {} {:.3f}".format(
            r, int(info["target"][r]), int(y[r].argmax()), args.score, float(info["base"][r])))
        if args.method == "integrated":                  # completeness: the attributions add up to the change
            change = float(info["base"][r] - info["baseline_score"][r])
            gaps.append(abs(float(signed[r].sum()) - change))
            print("  sum of attributions {:.4f}, score change from the baseline {:.4f}".format(
                float(signed[r].sum()), change))
        for row in maps[r]:
            print("  " + "".join(RAMP[min(len(RAMP) - 1, int(len(RAMP) * v / top))] for v in row))
    print(json.dumps({"images": int(held), "map": list(maps.shape[1:]), "score": args.score, "method": args.method,
                      "smooth": smooth, "largest": float(maps.max()), "completeness_gap": max(gaps) if gaps else None}))
