#!/usr/bin/env python
"""Test-time augmentation of a fitted Genetic-CNN: fit one genome with the paper's training augmentation
(``augment={"shift": 2, "flip": True}``) on part of the rows, then predict the held-out rows once as they are
and once as the mean over the ten views of ``tta={"shift": 2, "flip": True}`` (the identity, four
translations, and the mirror image of each). Prints one JSON line with both accuracies.

usage: python examples/cnn_tta.py [--device cpu|cuda:0] [--shift 2]"""
import argparse
import json

import _common

if __name__ == "__main__":
    import numpy as np
    import torch
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.models.cnn_fitted import tta_views
    from gentun_amd.utils.data import make_glyph_classification

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--shift", type=int, default=2)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    n = 224 if _common.SMALL else 960
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    held = n // 4 // 32 * 32 + 5                       # held-out rows: the last chunk of a launch is short
    setting = {"shift": args.shift, "flip": True}
    model = GeneticCnnModel(x[held:], y[held:], {"S_1": "101", "S_2": "110"}, nodes=(3, 3), input_shape=shape,
                            kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)), dense_units=32,
                            dropout_probability=0.5, classes=classes, nfold=2,
                            epochs=(1,) if _common.SMALL else (6,), learning_rate=(3e-3,), batch_size=32,
                            loss="ce", seed=0, device=args.device, augment=setting)
    model.fit()
    lab = y[:held].argmax(1)
    plain = model.predict(x[:held], output="label")
    tta = model.predict(x[:held], output="label", tta=setting)
    print(json.dumps({"held_out_rows": int(held), "views": len(tta_views(setting, shape)),
                      "accuracy": float((plain == lab).mean()), "accuracy_tta": float((tta == lab).mean())}))
