#!/usr/bin/env python
"""Nearest neighbours in the feature space of a fitted Genetic-CNN: fit one genome on part of the rows, embed
those rows once as the bank, then look up the ``k`` nearest training rows of every held-out image. Prints the
neighbours and their labels of the first held-out images and one JSON line with what one line of numpy makes of
the result: the accuracy of the kNN label vote next to the softmax head's, and the deep-kNN out-of-distribution
score (the distance to the k-th neighbour) of the held-out images next to that of pure noise.

usage: python examples/cnn_neighbors.py [--device cpu|cuda:0] [--k 5] [--metric l2|cosine]"""
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
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--metric", default="l2")
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
    lab, bank_lab = y[:held].argmax(1), y[held:].argmax(1)
    bank = model.embed(x[held:])                       # embedded once, searched twice below
    idx, dist = model.neighbors(x[:held], bank, k=args.k, metric=args.metric)
    for i in range(4):
        print("held-out image {} (label {}): neighbours {} labels {} distances {}".format(
            i, lab[i], idx[i].tolist(), bank_lab[idx[i]].tolist(), np.round(dist[i], 4).tolist()))
    vote = np.array([np.bincount(r, minlength=classes).argmax() for r in bank_lab[idx]])       # the kNN vote
    noise = np.random.default_rng(1).standard_normal((32,) + shape).astype(np.float32)
    ood = model.neighbors(noise, bank, k=args.k, metric=args.metric)[1][:, -1]                  # deep-kNN score
    print(json.dumps({"held_out_rows": int(held), "bank_rows": int(len(bank)), "k": args.k, "metric": args.metric,
                      "accuracy_head": float((model.predict(x[:held], output="label") == lab).mean()),
                      "accuracy_vote": float((vote == lab).mean()),
                      "kth_distance_held_out": float(np.median(dist[:, -1])),
                      "kth_distance_noise": float(np.median(ood))}))
