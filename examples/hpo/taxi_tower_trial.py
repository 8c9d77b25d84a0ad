"""HPO worker for the taxi Wide&Deep tower: trains WideDeepEstimator on synthetic taxi records for the tower given by
`--first-dnn-layer-size=`, `--num-dnn-layers=`, `--dnn-decay-factor=` (the knobs of the reference's trainer_fn,
`taxi_utils.py:300-302`) and prints `auc=<v>` / `loss=<v>` for the metrics collector (mifx/hpo/study.py). On a GPU
any tower other than the default trains on the general fused kernel (csrc/wd_general.hip)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

from mifx.data.synthetic import synthetic_records  # noqa: E402
from mifx.models.wide_deep import dnn_hidden_units  # noqa: E402
from mifx.trainer.estimator import RunConfig, WideDeepEstimator  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-dnn-layer-size", type=int, default=100)
    ap.add_argument("--num-dnn-layers", type=int, default=4)
    ap.add_argument("--dnn-decay-factor", type=float, default=0.7)
    ap.add_argument("--batch-size", type=int, default=40)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--records", type=int, default=6000)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    hidden = dnn_hidden_units(a.first_dnn_layer_size, a.num_dnn_layers, a.dnn_decay_factor)
    rec = synthetic_records(a.records, seed=11)
    n_train = a.records * 5 // 6
    est = WideDeepEstimator(RunConfig(save_checkpoints_steps=None, device=a.device), hidden_units=hidden,
                            batch_size=a.batch_size)
    est.train(lambda: rec[:n_train], max_steps=a.steps)
    m = est.evaluate(lambda: rec[n_train:])
    print(f"hidden_units={hidden}")
    print(f"auc={m['auc']:.4f}")
    print(f"loss={m['average_loss']:.4f}")
    return m


if __name__ == "__main__":
    main()
