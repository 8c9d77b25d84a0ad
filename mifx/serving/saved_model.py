"""SavedModel-equivalent export format and loader.

Layout (mirrors TF's `<export_dir_base>/<timestamp>/` versioned exports consumed by TF Serving,
`Predict_Fashion_MNIST.ipynb:L189` and `taxi_utils.py:326,348-356`)::

    <dir>/saved_model.json            format, model family/class/config, signatures, receiver
    <dir>/variables/variables.safetensors
    <dir>/assets/transform/...        copy of the Transform graph (serving/eval receivers)

Families: ``wide_deep`` (taxi W&D; raw-example receiver through the Transform graph, classify
outputs), ``module`` (any torch.nn.Module given by ``module_class`` + config, tensor inputs) and ``bert_seq_cls``
(the fine-tuned BERT classifier; ragged token-id inputs, served by the packed variable-length forward of
mifx.models.bert_infer).
"""
from __future__ import annotations

import importlib
import json
import os
import shutil

import numpy as np
import torch
from safetensors.torch import load_file, save_file

FORMAT = "mifx.saved_model/v1"


def _write(path: str, meta: dict, state_dict: dict) -> None:
    os.makedirs(os.path.join(path, "variables"), exist_ok=True)
    save_file({k: v.detach().cpu().contiguous() for k, v in state_dict.items()},
              os.path.join(path, "variables", "variables.safetensors"))
    with open(os.path.join(path, "saved_model.json"), "w") as f:
        json.dump(meta, f, indent=1)


def save_wide_deep(path: str, model, receiver: dict | None = None, global_step: int = 0) -> str:
    receiver = dict(receiver or {})
    tdir = receiver.pop("transform_output", None)
    if tdir:
        dst = os.path.join(path, "assets", "transform")
        shutil.copytree(tdir, dst, dirs_exist_ok=True)
    meta = {"format": FORMAT, "family": "wide_deep", "global_step": global_step,
            "model_class": "mifx.models.wide_deep:WideDeepModel",
            "model_config": {"hidden_units": list(model.cfg.hidden_units), "wide": [list(x) for x in model.cfg.wide],
                             "dense_features": list(model.cfg.dense_features), "label": model.cfg.label},
            "receiver": {"kind": receiver.get("kind", "transformed"), "has_transform": bool(tdir),
                         "raw_label_key": receiver.get("raw_label_key"),
                         "label_key": receiver.get("label_key", model.cfg.label)},
            "signatures": {"serving_default": {"method": "classify", "inputs": receiver.get("raw_feature_spec", {}),
                                               "outputs": ["logits", "logistic", "probabilities", "class_ids",
                                                           "classes"]}}}
    _write(path, meta, model.state_dict())
    return path


def save_module(path: str, model: torch.nn.Module, module_class: str, config: dict | None = None,
                input_shape: list | None = None, class_names: list | None = None) -> str:
    meta = {"format": FORMAT, "family": "module", "model_class": module_class, "model_config": config or {},
            "signatures": {"serving_default": {"method": "predict", "inputs": {"input": input_shape},
                                               "outputs": ["scores"], "class_names": class_names}}}
    _write(path, meta, model.state_dict())
    return path


_BERT_CFG = ("vocab_size", "hidden", "layers", "heads", "intermediate", "max_position", "type_vocab", "num_labels",
             "ln_eps")


def save_bert(path: str, state: dict, cfg, seq_len: int, class_names: list | None = None) -> str:
    """Family ``bert_seq_cls``: the TP=1 state of mifx.models.bert.BertForSequenceClassification (fp32) and its
    config. The family is built in (mifx.models.bert_infer.BertInference): the export names no class to import.
    seq_len: the length the model was fine-tuned at (requests may have any length up to min(max_position, 512))."""
    meta = {"format": FORMAT, "family": "bert_seq_cls",
            "model_config": {k: getattr(cfg, k) for k in _BERT_CFG}, "seq_len": int(seq_len),
            "signatures": {"serving_default": {
                "method": "classify",
                "inputs": {"input_ids": {"dtype": "int32", "shape": [-1, -1]},
                           "token_type_ids": {"dtype": "int32", "shape": [-1, -1], "optional": True}},
                "outputs": ["logits", "probabilities", "class_ids", "classes"],
                "class_names": None if class_names is None else [str(c) for c in class_names]}}}
    _write(path, meta, {k: v.detach().float() for k, v in state.items()})
    return path


# Model classes a "module" export may name. An export is data (JSON + safetensors); the class it names is imported and
# called with the export's model_config as keyword arguments, so an open set of classes would let whoever writes an
# export (or uploads one to a model server) run any importable callable. Only these classes -- plus any the serving
# process itself adds with register_servable_class() -- are ever imported by LoadedModel.
_SERVABLE = {
    "mifx.models.cnn:FashionCNN",
    "mifx.models.cnn:TpuMnistCNN",
    "mifx.models.cnn:MnistDPCNN",
    "mifx.models.taxi_dnn:TaxiDNN",
    "mifx.models.resnet:ResNetV2",
    "mifx.models.wide_deep:WideDeepModel",
    "torch.nn:Linear",
}


def register_servable_class(class_path: str) -> None:
    """Allow exports naming `module:Class` (an nn.Module subclass) to be loaded by this process."""
    _SERVABLE.add(class_path)


def servable_classes() -> frozenset:
    return frozenset(_SERVABLE)


def _json_plain(v, depth: int = 0) -> bool:
    if depth > 8:
        return False
    if v is None or isinstance(v, (bool, int, float, str)):
        return True
    if isinstance(v, list):
        return all(_json_plain(x, depth + 1) for x in v)
    if isinstance(v, dict):
        return all(isinstance(k, str) and _json_plain(x, depth + 1) for k, x in v.items())
    return False


def _import(path: str):
    if path not in _SERVABLE:
        raise PermissionError(f"model class {path!r} is not servable (allowed: {sorted(_SERVABLE)}; "
                              "register_servable_class() adds one)")
    mod, _, name = path.partition(":")
    cls = getattr(importlib.import_module(mod), name)
    if not (isinstance(cls, type) and issubclass(cls, torch.nn.Module)):
        raise PermissionError(f"model class {path!r} is not a torch.nn.Module")
    return cls


class LoadedModel:
    def __init__(self, path: str, device: str | None = None):
        self.path = path
        with open(os.path.join(path, "saved_model.json")) as f:
            self.meta = json.load(f)
        if self.meta.get("format") != FORMAT:
            raise ValueError(f"{path}: not a {FORMAT} export")
        self.device = torch.device(device) if device else (torch.device("cuda") if torch.cuda.is_available()
                                                          else torch.device("cpu"))
        sd = load_file(os.path.join(path, "variables", "variables.safetensors"))
        self.family = self.meta["family"]
        self.transform = None
        if self.family not in ("wide_deep", "module", "bert_seq_cls"):
            raise ValueError(f"{path}: unknown model family {self.family!r}")
        if self.family == "bert_seq_cls":
            from ..models.bert import BertConfig
            from ..models.bert_infer import BertInference

            mc = self.meta.get("model_config", {})
            if not (isinstance(mc, dict) and _json_plain(mc)):
                raise ValueError(f"{path}: model_config must be a JSON object of plain values")
            self.model = BertInference(sd, BertConfig(**{k: mc[k] for k in _BERT_CFG if k in mc}), self.device)
        elif self.family == "wide_deep":
            from ..models import wide_deep as wdm

            mc = self.meta["model_config"]
            cfg = wdm.WideDeepConfig(dense_features=mc["dense_features"], wide=[tuple(x) for x in mc["wide"]],
                                     hidden_units=mc["hidden_units"], label=mc["label"])
            self.model = wdm.WideDeepModel(cfg, seed=None)
            self.model.load_state_dict(sd, strict=False)
            tdir = os.path.join(path, "assets", "transform")
            if self.meta["receiver"].get("has_transform") and os.path.isdir(tdir):
                from ..transform import TransformOutput

                self.transform = TransformOutput(tdir)
            self._fused = None
        else:
            cls = _import(self.meta["model_class"])
            cfg = self.meta.get("model_config", {})
            if not (isinstance(cfg, dict) and _json_plain(cfg)):
                raise ValueError(f"{path}: model_config must be a JSON object of plain values")
            self.model = cls(**cfg)
            self.model.load_state_dict(sd)
            self.model.to(self.device).eval()

    @property
    def signatures(self) -> dict:
        return self.meta["signatures"]

    # ------------------------------------------------------------------ wide & deep
    def _wd_records(self, columns: dict, with_label: bool) -> np.ndarray:
        from ..models import wide_deep as wdm

        cols = self.transform.transform_raw_features(columns) if self.transform else columns
        return wdm.pack_transformed_columns(cols, self.model.cfg, with_label=with_label)

    def wd_logits(self, columns: dict) -> np.ndarray:
        from ..models import wide_deep as wdm

        rec = self._wd_records(columns, with_label=False)
        t = torch.from_numpy(rec.view(np.uint8).reshape(-1, 32).copy())
        if self.device.type == "cuda" and len(rec):
            if self._fused is None:
                from ..trainer.dispatch import make_wide_deep_trainer

                # the chained kernel for the taxi tower, the general fused kernel for any other hidden_units
                self._fused = make_wide_deep_trainer(self.model, self.device, batch=64)
            return self._fused.predict_logits(t).cpu().numpy()
        dense, ids, _ = wdm.records_to_tensors(t)
        with torch.no_grad():
            return self.model(dense, ids).numpy()

    # ------------------------------------------------------------------ BERT sequence classification
    def bert_sequences(self, instances):
        """(token-id lists, token-type lists or None) of a request, validated. Row format: a list of
        {"input_ids": [...], "token_type_ids": [...]?} of any lengths (a bare id list is taken as input_ids).
        Columnar: {"input_ids": [N, S], "attention_mask": [N, S]?, "token_type_ids": [N, S]?}; the lengths come from
        the mask, which must be a prefix of ones (without a mask every row has S tokens)."""
        from ..models.bert_infer import validate

        if isinstance(instances, dict):
            if "input_ids" not in instances:
                raise ValueError("inputs need 'input_ids'")
            ids = np.asarray(instances["input_ids"])
            if ids.ndim != 2:
                raise ValueError(f"columnar input_ids must be [N, S], got shape {ids.shape}")
            am = instances.get("attention_mask")
            if am is None:
                lens = np.full(len(ids), ids.shape[1], np.int64)
            else:
                am = np.asarray(am)
                if am.shape != ids.shape:
                    raise ValueError(f"attention_mask shape {am.shape} is not input_ids' {ids.shape}")
                lens = (am != 0).sum(1)
                for i, n in enumerate(lens):
                    if not (am[i, :n] == 1).all() or (am[i, n:] != 0).any():
                        raise ValueError(f"instance {i}: attention_mask is not a prefix of ones")
            tt = instances.get("token_type_ids")
            if tt is not None and np.asarray(tt).shape != ids.shape:
                raise ValueError(f"token_type_ids shape {np.asarray(tt).shape} is not input_ids' {ids.shape}")
            seqs = [ids[i, :n] for i, n in enumerate(lens)]
            tts = None if tt is None else [np.asarray(tt)[i, :n] for i, n in enumerate(lens)]
        else:
            rows = [r if isinstance(r, dict) else {"input_ids": r} for r in instances]
            for i, r in enumerate(rows):
                if "input_ids" not in r:
                    raise ValueError(f"instance {i}: no 'input_ids'")
            seqs = [np.asarray(r["input_ids"]) for r in rows]
            tts = [None if r.get("token_type_ids") is None else np.asarray(r["token_type_ids"]) for r in rows]
            if all(t is None for t in tts):
                tts = None
        validate(seqs, tts, self.model.cfg)
        return seqs, tts

    def validate(self, instances) -> None:
        """Raise ValueError for a request this model would refuse (before it is merged with others into a batch)."""
        if self.family == "bert_seq_cls":
            self.bert_sequences(instances)

    def _bert_predict(self, instances) -> dict:
        seqs, tts = self.bert_sequences(instances)
        logits = self.model.logits(seqs, tts).cpu().numpy()  # packed by token capacity, not by instance count
        z = logits - logits.max(-1, keepdims=True) if len(logits) else logits
        p = np.exp(z) / np.exp(z).sum(-1, keepdims=True) if len(logits) else logits
        ids = logits.argmax(-1).astype(np.int64) if len(logits) else np.zeros(0, np.int64)
        names = self.signatures["serving_default"].get("class_names")
        classes = np.array([names[i] if names else str(i) for i in ids], dtype=object).astype(str)
        return {"logits": logits, "probabilities": p, "class_ids": ids[:, None], "classes": classes[:, None]}

    def predict(self, instances) -> dict:
        """instances: list of feature dicts (TF-Serving row format) or dict of columns."""
        if self.family == "bert_seq_cls":
            return self._bert_predict(instances)
        if self.family == "wide_deep":
            if isinstance(instances, list):
                keys = sorted({k for r in instances for k in r})
                columns = {k: np.array([r.get(k) for r in instances], dtype=object) for k in keys}
                for k, v in columns.items():
                    if all(isinstance(x, (int, float)) or x is None for x in v):
                        if any(isinstance(x, float) for x in v):
                            columns[k] = np.array([np.nan if x is None else x for x in v], dtype=np.float64)
            else:
                columns = instances
            logits = self.wd_logits(columns)
            p = 1.0 / (1.0 + np.exp(-logits))
            cls = (p > 0.5).astype(np.int64)
            return {"logits": logits[:, None], "logistic": p[:, None], "probabilities": np.stack([1 - p, p], 1),
                    "class_ids": cls[:, None], "classes": cls.astype(str)[:, None]}
        x = torch.as_tensor(np.asarray(instances, dtype=np.float32), device=self.device)
        with torch.no_grad():
            return {"scores": self.model(x).float().cpu().numpy()}


def load(path: str, device: str | None = None) -> LoadedModel:
    return LoadedModel(path, device)


def latest_export(export_dir_base: str) -> str:
    vs = [d for d in os.listdir(export_dir_base) if d.isdigit()]
    if not vs:
        raise FileNotFoundError(f"no versioned exports under {export_dir_base}")
    return os.path.join(export_dir_base, max(vs, key=int))
