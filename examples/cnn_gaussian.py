#!/usr/bin/env python
"""Out-of-distribution scoring by Mahalanobis distance in the feature space of a fitted Genetic-CNN (Lee et al.,
2018): fit one genome on the training glyphs, fit class-conditional Gaussians with a tied covariance to their
hidden rows, then score held-out glyphs against uniform-noise images. Prints one JSON line: the AUROC of
``d.min(1)`` (noise above held-out) and how often the Gaussian-discriminant label ``d.argmin(1)`` agrees with
``predict``.

usage: python examples/cnn_gaussian.py [--device cpu|cuda:0] [--shrink 0.01]"""
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
    ap.add_argument("--shrink", type=float, default=0.01)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    n = 224 if _common.SMALL else 960
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    held = n // 4 // 32 * 32 + 5                       # held-out rows: the last chunk of a launch is short
    model = GeneticCnnModel(x[held:], y[held:], {"S_1": "101", "S_2": "110"}, nodes=(3, 3), input_shape=shape,
                            kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)), dense_units=32,
                            dropout_probability=0.5, classes=classes, nfold=2,
                            epochs=(1,) if _common.SMALL else (6,), learning_rate=(3e-3,), batch_size=32,
                            loss="ce", seed=0, device=args.device)
    model.fit()
    stats = model.gaussian_fit(x[held:], labels=y[held:], shrink=args.shrink)
    noise = np.random.default_rng(1).uniform(float(x.min()), float(x.max()), (held,) + shape).astype(np.float32)
    d_in, d_out = model.mahalanobis(x[:held], stats), model.mahalanobis(noise, stats)
    s_in, s_out = d_in.min(1).astype(np.float64), d_out.min(1).astype(np.float64)
    wins = (s_out[:, None] > s_in[None, :]).sum() + 0.5 * (s_out[:, None] == s_in[None, :]).sum()
    print(json.dumps({"held_out_rows": int(held), "bank_rows": int(n - held), "shrink": args.shrink,
                      "class_counts": stats["count"].tolist(),
                      "auroc_noise_vs_held_out": float(wins / (len(s_in) * len(s_out))),
                      "median_score_held_out": float(np.median(s_in)), "median_score_noise": float(np.median(s_out)),
                      "agreement_with_predict": float((d_in.argmin(1) == model.predict(x[:held], output="label"))
                                                      .mean())}))
