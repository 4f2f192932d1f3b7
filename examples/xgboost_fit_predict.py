#!/usr/bin/env python
"""From the search to a model that scores new rows: a small GA over GBDT hyper-parameters on white-wine quality,
then ``fit`` of the fittest individual's genes on the training slice and ``predict`` on a held-out slice.
The reference stops at the CV fitness (tests/test_wine-quality.py); with xgboost installed its users would call
``xgb.train`` / ``Booster.predict`` next, which is what ``XgboostModel.fit`` / ``predict`` provide here."""
import os
import tempfile

import _common

if __name__ == "__main__":
    import numpy as np
    from gentun_amd import GeneticAlgorithm, Population, XgboostIndividual
    from gentun_amd.models.booster import Booster
    from gentun_amd.models.xgboost_models import XgboostModel

    x, y = _common.wine()
    order = np.random.default_rng(0).permutation(len(y))
    x, y = np.asarray(x)[order], np.asarray(y)[order]
    held = len(y) // 5
    x_train, y_train, x_test, y_test = x[held:], y[held:], x[:held], y[:held]

    extra = {"nfold": 3, "num_boost_round": 20 if _common.SMALL else 200, "early_stopping_rounds": 10}
    pop = Population(XgboostIndividual, x_train, y_train, size=3 if _common.SMALL else 6, additional_parameters=extra, maximize=False)
    best = GeneticAlgorithm(pop, tournament_size=3, elitism=True, seed=0, verbose=False).run(2)
    print("best CV rmse", best.get_fitness(), best.get_genes())

    model = XgboostModel(x_train, y_train, best.get_genes(), **extra)
    model.cross_validate()                       # the round count of the final model: the CV's best round
    bst = model.fit()
    pred = model.predict(x_test)
    print("rounds", bst.num_rounds, "held-out rmse", float(np.sqrt(np.mean((pred - y_test) ** 2))))
    path = os.path.join(tempfile.mkdtemp(), "wine_booster.npz")
    bst.save(path)
    assert Booster.load(path).predict(x_test).tobytes() == pred.tobytes()
    print("saved", path)
    # which two features the model uses together: SHAP interaction values, mean |Phi[i][j]| over the held-out rows
    F = x_test.shape[1]
    pair = np.abs(bst.predict(x_test, pred_interactions=True)[:, :F, :F]).mean(axis=0)
    np.fill_diagonal(pair, 0.0)
    i, j = np.unravel_index(int(np.argmax(pair)), pair.shape)
    print("strongest interaction: features", int(min(i, j)), "and", int(max(i, j)), "mean |Phi|", float(pair[i, j]))
