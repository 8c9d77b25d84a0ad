"""Serving the fine-tuned BERT classifier: the `bert_seq_cls` saved-model family, the REST app, the Trainer component's
export, and (GPU) the dynamic batcher over the packed variable-length forward."""
import functools
import json
import math
import os
import threading

import numpy as np
import pytest
import torch

from mifx.models.bert import BertConfig, BertForSequenceClassification, full_init_state
from mifx.serving import saved_model
from mifx.serving.server import ModelManager, create_app

LENGTHS = [1, 17, 40, 128, 3, 65]


def _cfg():
    return BertConfig(vocab_size=512, hidden=128, heads=2, intermediate=256, layers=2, max_position=512)


@functools.lru_cache(maxsize=None)
def _state():
    return full_init_state(_cfg(), 0)


def _instances(lengths=LENGTHS, seed=0):
    g = np.random.default_rng(seed)
    return [{"input_ids": g.integers(0, 512, size=L).tolist(), "token_type_ids": [0] * (L // 2) + [1] * (L - L // 2)}
            for L in lengths]


def _ref_logits(instances):
    """The fp32 CPU model on each sequence alone, unpadded."""
    m = BertForSequenceClassification(_cfg(), None, seed=None)
    m.load_full(_state())
    m.eval()
    with torch.no_grad():
        return torch.cat([m(torch.tensor([r["input_ids"]]), torch.tensor([r["token_type_ids"]]))
                          for r in instances]).numpy()


def _export(tmp_path, version=1, class_names=("neg", "pos")):
    d = tmp_path / "bert" / str(version)
    saved_model.save_bert(str(d), _state(), _cfg(), 128, class_names=list(class_names))
    return str(d)


def test_save_load_predict_round_trip(tmp_path):
    path = _export(tmp_path)
    meta = json.load(open(os.path.join(path, "saved_model.json")))
    assert meta["family"] == "bert_seq_cls" and "model_class" not in meta
    sig = meta["signatures"]["serving_default"]
    assert sig["method"] == "classify" and set(sig["inputs"]) == {"input_ids", "token_type_ids"}
    assert sig["outputs"] == ["logits", "probabilities", "class_ids", "classes"]
    assert os.path.exists(os.path.join(path, "variables", "variables.safetensors"))
    lm = saved_model.load(path, "cpu")
    inst = _instances()
    out = lm.predict(inst)
    ref = _ref_logits(inst)
    assert out["logits"].shape == (len(inst), 2) and out["logits"].dtype == np.float32
    np.testing.assert_allclose(out["logits"], ref, rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["probabilities"].sum(-1), 1.0, atol=1e-6)
    assert out["class_ids"].shape == (len(inst), 1) and np.array_equal(out["class_ids"][:, 0], ref.argmax(-1))
    assert [c for c in out["classes"][:, 0]] == [("neg", "pos")[i] for i in ref.argmax(-1)]
    # the columnar form (what the gRPC service passes): lengths from the attention mask
    S = max(LENGTHS)
    ids = np.zeros((len(inst), S), np.int32)
    tt = np.zeros_like(ids)
    am = np.zeros_like(ids)
    for i, r in enumerate(inst):
        n = len(r["input_ids"])
        ids[i, :n], tt[i, :n], am[i, :n] = r["input_ids"], r["token_type_ids"], 1
    col = lm.predict({"input_ids": ids, "attention_mask": am, "token_type_ids": tt})
    np.testing.assert_allclose(col["logits"], ref, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(col["logits"], out["logits"])
    am[2, 5] = 0  # a hole: not a prefix of ones
    with pytest.raises(ValueError, match="instance 2: attention_mask is not a prefix of ones"):
        lm.predict({"input_ids": ids, "attention_mask": am})
    # token types are optional per row
    np.testing.assert_allclose(lm.predict([{"input_ids": [5, 6, 7]}])["logits"],
                               lm.predict([{"input_ids": [5, 6, 7], "token_type_ids": [0, 0, 0]}])["logits"])


def test_rest_predict_metadata_and_bad_request(tmp_path):
    from fastapi.testclient import TestClient

    _export(tmp_path)
    mgr = ModelManager("bert", str(tmp_path / "bert"), device="cpu", poll_s=0)
    try:
        c = TestClient(create_app({"bert": mgr}))
        inst = _instances()
        r = c.post("/v1/models/bert:predict", json={"instances": inst})
        assert r.status_code == 200, r.text
        preds = r.json()["predictions"]
        logits = np.array([p["logits"] for p in preds])
        assert logits.shape == (len(inst), 2)
        np.testing.assert_allclose(logits, _ref_logits(inst), rtol=0, atol=1e-5)
        bad = [inst[0], {"input_ids": [3, 512, 4]}]
        r = c.post("/v1/models/bert:predict", json={"instances": bad})
        assert r.status_code == 400 and "sequence 1" in r.json()["error"] and "vocabulary" in r.json()["error"]
        r = c.post("/v1/models/bert:predict", json={"instances": [{"input_ids": []}]})
        assert r.status_code == 400 and "empty" in r.json()["error"]
        md = c.get("/v1/models/bert/metadata").json()
        sig = md["metadata"]["signature_def"]["serving_default"]
        assert md["model_spec"] == {"name": "bert", "version": "1"} and sig["method"] == "classify"
        assert set(sig["inputs"]) == {"input_ids", "token_type_ids"} and "logits" in sig["outputs"]
        r = c.post("/v1/models/bert:classify", json={"examples": inst[:2]})
        assert r.status_code == 200 and len(r.json()["results"]) == 2
    finally:
        mgr.close()


def test_grpc_predict_columnar(tmp_path):
    pytest.importorskip("grpc")
    from mifx.serving.grpc_service import PredictionClient, serve

    _export(tmp_path)
    mgr = ModelManager("bert", str(tmp_path / "bert"), device="cpu", poll_s=0)
    server, port = serve({"bert": mgr}, 0)
    try:
        inst = _instances([5, 9, 2])
        ids = np.zeros((3, 9), np.int32)
        am = np.zeros_like(ids)
        for i, r in enumerate(inst):
            ids[i, :len(r["input_ids"])], am[i, :len(r["input_ids"])] = r["input_ids"], 1
        cl = PredictionClient(f"localhost:{port}")
        out = cl.predict("bert", {"input_ids": ids, "attention_mask": am}, output_filter=["logits"])
        want = saved_model.load(str(tmp_path / "bert" / "1"), "cpu").predict(
            [{"input_ids": r["input_ids"]} for r in inst])["logits"]
        np.testing.assert_allclose(np.asarray(out["logits"]), want, rtol=0, atol=1e-6)
    finally:
        server.stop(grace=0.5)
        mgr.close()


def test_trainer_component_export_is_servable(tmp_path):
    """TextExampleGen -> BertTrainer on the CPU: the serving export loads through saved_model.load and predicts the
    eval split with the accuracy the component recorded; load_bert_export still reads the same directory."""
    from mifx.components import EvalArgs, TrainArgs
    from mifx.components.bert import BertTrainer, TextExampleGen, load_bert_export, load_split
    from mifx.components.trainer import SERVING_DIR, latest_model_dir
    from mifx.orchestration import LocalDagRunner, Pipeline

    eg = TextExampleGen(num_synthetic=240, seq_len=32, vocab_size=512, num_labels=2, seed=3)
    tr = BertTrainer(examples=eg.outputs.examples, train_args=TrainArgs(num_steps=6), eval_args=EvalArgs(num_steps=0),
                     custom_config=dict(vocab_size=512, hidden=128, heads=2, intermediate=256, layers=2,
                                        max_position=512, dropout=0.0, tp=1, batch_size=16, learning_rate=1e-3,
                                        graph=False))
    p = Pipeline(pipeline_name="bs", pipeline_root=str(tmp_path / "bs"), components=[eg, tr],
                 metadata_db_root=str(tmp_path / "md"))
    res = LocalDagRunner(device="cpu").run(p)
    assert res.succeeded
    model = res.components["BertTrainer"].outputs["output"][0]
    ev_uri = [a.uri for a in res.components["TextExampleGen"].outputs["examples"] if a.split == "eval"][0]
    metrics = json.load(open(os.path.join(model.uri, "metrics.json")))
    path = latest_model_dir(model.uri, SERVING_DIR)
    assert os.path.samefile(path, metrics["export"])
    lm = saved_model.load(path, "cpu")
    assert lm.family == "bert_seq_cls" and lm.meta["seq_len"] == 32
    ev = load_split(ev_uri)
    out = lm.predict({k: ev[k] for k in ("input_ids", "attention_mask", "token_type_ids")})
    acc = float((out["class_ids"][:, 0] == ev["labels"]).mean())
    assert len(ev["labels"]) == metrics["eval"]["num_eval_examples"]
    assert acc == pytest.approx(metrics["eval"]["accuracy"], abs=1e-12)
    m, S = load_bert_export(path)
    assert S == 32
    with torch.no_grad():
        old = m(torch.from_numpy(ev["input_ids"][:4].astype(np.int64)),
                torch.from_numpy(ev["token_type_ids"][:4].astype(np.int64)),
                torch.from_numpy(ev["attention_mask"][:4].astype(np.float32)))
    np.testing.assert_allclose(out["logits"][:4], old.numpy(), rtol=0, atol=1e-5)
    # and the Pusher's copy of it serves
    import shutil

    shutil.copytree(path, str(tmp_path / "push" / "7"))
    mgr = ModelManager("bert", str(tmp_path / "push"), device="cpu", poll_s=0)
    try:
        one = mgr.get().predict([{"input_ids": ev["input_ids"][0][:int(ev["attention_mask"][0].sum())].tolist()}])
        assert one["logits"].shape == (1, 2)
    finally:
        mgr.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _bf16_ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


@pytest.mark.gpu
def test_server_batches_concurrent_ragged_requests_gpu(tmp_path):
    """16 concurrent ragged requests through the dynamic batcher: each equals the same instance sent alone within
    the end-to-end bound of tests/test_bert_infer.py (2 E_pad + one bf16 ulp of the largest |logit|, E_pad the error
    of the padded bf16 eval forward at S = 128 against the fp32 reference), in fewer than 16 forwards."""
    from mifx.models.bert_infer import _pad_arrays

    _export(tmp_path)
    lengths = [1, 17, 40, 128, 3, 65, 64, 100, 2, 31, 90, 127, 16, 15, 77, 50]
    inst = _instances(lengths, seed=9)
    ref = _ref_logits(inst)
    pm = BertForSequenceClassification(_cfg(), None, seed=None)
    pm.load_full(_state())
    pm = pm.cuda().bfloat16().eval()
    ids, tt, am = _pad_arrays([np.asarray(r["input_ids"]) for r in inst], [r["token_type_ids"] for r in inst], 128)
    with torch.no_grad():
        padded = pm(*(torch.from_numpy(a).cuda() for a in (ids, tt, am))).float().cpu().numpy()
    bound = 2 * float(np.abs(padded - ref).max()) + _bf16_ulp(float(np.abs(ref).max()))
    mgr = ModelManager("bert", str(tmp_path / "bert"), device="cuda", poll_s=0, batching=True)
    try:
        s = mgr.get()
        assert s.batcher is not None and s.model.model.packed
        alone = np.concatenate([s.predict([r])["logits"] for r in inst])
        before = s.batcher.batches_run
        assert before == 16
        gate = threading.Barrier(16)
        got = [None] * 16

        def call(i):
            gate.wait()
            got[i] = s.predict([inst[i]])["logits"]

        ts = [threading.Thread(target=call, args=(i,)) for i in range(16)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
        merged = np.concatenate(got)
        print(f"SERVER batches={s.batcher.batches_run - before} max|merged-alone|={np.abs(merged - alone).max():.3e} "
              f"bound={bound:.3e}")
        assert s.batcher.batches_run - before < 16
        assert float(np.abs(merged - alone).max()) <= bound
        assert float(np.abs(merged - ref).max()) <= bound
        with pytest.raises(ValueError, match="vocabulary"):  # refused alone, before it is merged with others
            s.predict([{"input_ids": [1, 9999]}])
    finally:
        mgr.close()
