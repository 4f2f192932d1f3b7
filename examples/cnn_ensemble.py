#!/usr/bin/env python
"""From a Genetic-CNN population to an ensemble that classifies new images: take the top genomes of a short
search (``--search``) or a fixed genome list, ``fit_ensemble`` them on every training row (on an MI355X: one
population job, every member bit-identical to its own ``GeneticCnnModel.fit()``), ``save`` the ensemble,
``load`` it and ``predict`` held-out images with the weighted mean of the members' probabilities and with
their votes.

usage: python examples/cnn_ensemble.py [--device cpu|cuda:0] [--out ensemble.npz] [--search]"""
import argparse
import json
import os
import tempfile

import _common  # noqa: F401  (puts the repository on sys.path)

if __name__ == "__main__":
    import numpy as np
    import torch
    from gentun_amd.models import CnnEnsemble, fit_ensemble
    from gentun_amd.models.cnn_ensemble import top_genomes
    from gentun_amd.utils.data import make_glyph_classification

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--search", action="store_true", help="take the genomes from a one-generation search")
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    x, y = make_glyph_classification(n=480, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    x_train, y_train, x_new, y_new = x[:384], y[:384], x[384:], y[384:]
    space = dict(nodes=(3, 3), input_shape=shape, kernels_per_layer=(8, 16), kernel_sizes=((3, 3), (3, 3)),
                 dense_units=32, dropout_probability=0.5, classes=classes, nfold=3, epochs=(3,),
                 learning_rate=(3e-3,), batch_size=32, loss="ce", seed=0)

    if args.search:
        from gentun_amd import GeneticCnnIndividual, Population, set_seed
        set_seed(0)
        population = Population(GeneticCnnIndividual, x_train, y_train, size=4, maximize=True,
                                additional_parameters=dict(space, device=args.device))
        population.get_fittest()                       # evaluates every individual
        genomes = top_genomes(population, 3)
    else:
        genomes = [{"S_1": "101", "S_2": "110"}, {"S_1": "111", "S_2": "111"}, {"S_1": "011", "S_2": "101"}]

    ens = fit_ensemble(x_train, y_train, genomes, device=args.device, **space)
    path = args.out or os.path.join(tempfile.mkdtemp(), "cnn_ensemble.npz")
    ens.save(path)
    back = CnnEnsemble.load(path)
    label = back.predict(x_new, device=args.device, output="label")
    voted = back.predict(x_new, device=args.device, output="vote_label")
    same = bool(np.array_equal(label, ens.predict(x_new, device=args.device, output="label")))
    truth = y_new.argmax(1)
    members = [float((m.predict_classes(x_new, device=args.device) == truth).mean()) for m in back.members]
    print(json.dumps({"saved_ensemble": path, "genes": [m.genes for m in back.members],
                      "train_metrics": ens.metrics, "held_out_accuracy": float((label == truth).mean()),
                      "held_out_vote_accuracy": float((voted == truth).mean()),
                      "held_out_member_accuracy": members, "reloaded_predictions_equal": same}))
