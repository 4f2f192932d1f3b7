#!/usr/bin/env python
"""From a Genetic-CNN genome to a model that classifies new images: ``fit`` a fixed genome on synthetic
glyph images, ``save`` the classifier, ``load`` it and ``predict`` held-out images. The reference stops at
the CV fitness; its users had ``model.model.predict`` / ``model.model.save`` through Keras, which is what
``GeneticCnnModel.fit`` and ``CnnClassifier`` provide here (HIP kernels on an MI355X, stock torch on a CPU).

usage: python examples/cnn_fit_predict.py [--device cpu|cuda:0] [--out model.npz]"""
import argparse
import json
import os
import tempfile

import _common  # noqa: F401  (puts the repository on sys.path)

if __name__ == "__main__":
    import numpy as np
    import torch
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.models.cnn_fitted import CnnClassifier
    from gentun_amd.utils.data import make_glyph_classification

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    shape, classes = (16, 16, 1), 4
    x, y = make_glyph_classification(n=480, shape=shape, classes=classes, seed=0, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    x_train, y_train, x_new, y_new = x[:384], y[:384], x[384:], y[384:]

    # a search (examples/mnist_genetic_cnn.py) would hand over best.get_genes(); here a fixed genome
    genes = {"S_1": "101", "S_2": "110"}
    model = GeneticCnnModel(x_train, y_train, genes, nodes=(3, 3), input_shape=shape, kernels_per_layer=(8, 16),
                            kernel_sizes=((3, 3), (3, 3)), dense_units=32, dropout_probability=0.5, classes=classes,
                            nfold=3, epochs=(3,), learning_rate=(3e-3,), batch_size=32, loss="ce", seed=0,
                            device=args.device)
    clf = model.fit()
    path = args.out or os.path.join(tempfile.mkdtemp(), "cnn_model.npz")
    clf.save(path)
    back = CnnClassifier.load(path)
    label = back.predict_classes(x_new, device=args.device)
    same = bool(np.array_equal(label, model.predict(x_new, output="label")))
    print(json.dumps({"saved_model": path, "genes": clf.genes, "train_metrics": clf.metrics,
                      "held_out_accuracy": float((label == y_new.argmax(1)).mean()),
                      "reloaded_predictions_equal": same}))
