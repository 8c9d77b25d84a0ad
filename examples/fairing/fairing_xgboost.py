"""XGBoost-style regressor trained through the fairing config (reference:
`kubeflow-pipelines/fairing/fairing_xgboost.py`). The Ames-housing download is unavailable offline,
so a synthetic table of the same shape (1460 rows, 36 numeric features) is used.
`--device gpu` trains on the device learner (csrc/gbdt_gpu.hip); the default is the host learner.
`--subsample`, `--colsample-bytree`, `--colsample-bylevel` and `--seed` pass the stochastic-boosting parameters a
hyper-parameter search over this example would tune (1.0 each: nothing is drawn)."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

import numpy as np  # noqa: E402
from sklearn.metrics import mean_absolute_error  # noqa: E402

from mifx import fairing  # noqa: E402
from mifx.gbdt import XGBRegressor  # noqa: E402

ESTIMATORS, LEARNING_RATE, TEST_FRACTION_SIZE, EARLY_STOPPING_ROUNDS = 1000, 0.1, 0.25, 50


def read_input(test_size=TEST_FRACTION_SIZE):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(1460, 36))
    y = 180000 + 40000 * X[:, 0] + 15000 * np.sin(X[:, 1]) + 8000 * X[:, 2] * X[:, 3] + rng.normal(0, 5000, 1460)
    n = int(len(X) * (1 - test_size))
    return (X[:n], y[:n]), (X[n:], y[n:])


def run_training_and_eval(device="cpu", subsample=1.0, colsample_bytree=1.0, colsample_bylevel=1.0, seed=0):
    (tx, ty), (vx, vy) = read_input()
    model = XGBRegressor(n_estimators=ESTIMATORS, learning_rate=LEARNING_RATE, device=device, subsample=subsample,
                         colsample_bytree=colsample_bytree, colsample_bylevel=colsample_bylevel, random_state=seed)
    model.fit(tx, ty, early_stopping_rounds=EARLY_STOPPING_ROUNDS, eval_set=[(vx, vy)])
    logging.info("Best RMSE on eval: %.2f with %d rounds", model.best_score, model.best_iteration + 1)
    mae = mean_absolute_error(model.predict(vx), vy)
    print(f"mean_absolute_error={mae:.2f}")
    # which columns drive the price: the model's importances, and why the first eval row got its prediction
    top = np.argsort(-model.feature_importances_)[:5]
    print("top importances (gain): " + ", ".join(f"f{j}={model.feature_importances_[j]:.3f}" for j in top))
    contribs = model.predict_contribs(vx[:1])[0]  # [features + 1]: one contribution per column, then the bias
    lead = np.argsort(-np.abs(contribs[:-1]))[:5]
    print(f"row 0: prediction {contribs.sum():.0f} = bias {contribs[-1]:.0f} " +
          " ".join(f"{contribs[j]:+.0f}[f{j}]" for j in lead) + " + the other columns")
    return mae


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--device", default="cpu", help="cpu (default), gpu, cuda or cuda:N")
    ap.add_argument("--subsample", type=float, default=1.0, help="rows sampled per round, in (0, 1]")
    ap.add_argument("--colsample-bytree", type=float, default=1.0, help="features sampled per tree, in (0, 1]")
    ap.add_argument("--colsample-bylevel", type=float, default=1.0, help="features sampled per level, in (0, 1]")
    ap.add_argument("--seed", type=int, default=0, help="random_state of the draws")
    args = ap.parse_args()
    fairing.config.set_builder("append", base_image="rocm/pytorch:latest", registry="local", push=False)
    fairing.config.set_deployer("local")
    print(fairing.config.fn(run_training_and_eval)(args.device, args.subsample, args.colsample_bytree,
                                                   args.colsample_bylevel, args.seed))
