"""Image pipeline components (BASELINE config 5: ImageNet-shaped ExampleGen -> Transform -> Trainer).

* `ImageExampleGen`: ingests `.npy` shards (uint8 [N, H, W, 3] images + int64 labels; files this
  framework or the user wrote, loaded with allow_pickle=False) or synthesises an ImageNet-shaped
  set; deterministic hash split train:eval = 2:1; writes `images.npy` / `labels.npy` per split.
* `ImageTransform`: full-pass per-channel mean / std analyzer over the training split (fp64 on the
  GPU via the HIP column-moments kernel when available) -> transform artifact (JSON), applied by the
  trainer's fused crop/flip/normalize kernel. It owns the preprocessing recipe: optional `augment`
  ("random_resized_crop": a random box of `rrc_scale` of the image at an aspect ratio in `rrc_ratio`,
  resized to the crop size), and `eval_resize` (evaluate on resize-then-centre-crop); all off by default
  and written as extra keys of `image_transform.json`.
* `ImageTrainer`: ResNet-50 v2 on the fused input kernel, bf16 channels_last, optional
  data-parallel (RCCL) inside the component; exports a servable model (`save_module`)."""
from __future__ import annotations

import json
import os

import numpy as np

from ..orchestration import artifact as A
from ..orchestration.component import (BaseComponent, BaseExecutor, ChannelParameter, ComponentSpec,
                                       ExecutionParameter)


class _KwComponent(BaseComponent):
    """Component whose constructor forwards keyword arguments to its spec."""

    def __init__(self, name: str | None = None, **kwargs):
        super().__init__(self.SPEC_CLASS(**kwargs), name=name)


def _split_ids(n: int, eval_buckets: int = 1, total: int = 3):
    h = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(61)
    is_eval = (h % np.uint64(total)) < np.uint64(eval_buckets)
    return np.nonzero(~is_eval)[0], np.nonzero(is_eval)[0]


class ImageExampleGenSpec(ComponentSpec):
    PARAMETERS = {"num_synthetic": ExecutionParameter(optional=True, default=0),
                  "image_size": ExecutionParameter(optional=True, default=256),
                  "num_classes": ExecutionParameter(optional=True, default=1000),
                  "seed": ExecutionParameter(optional=True, default=0)}
    INPUTS = {"input_base": ChannelParameter(A.EXTERNAL, optional=True)}
    OUTPUTS = {"examples": ChannelParameter(A.EXAMPLES)}


class ImageExampleGenExecutor(BaseExecutor):
    def Do(self, input_dict, output_dict, exec_properties):  # noqa: N802
        if input_dict.get("input_base"):
            base = input_dict["input_base"][0].uri
            imgs = np.load(os.path.join(base, "images.npy"), allow_pickle=False)
            labels = np.load(os.path.join(base, "labels.npy"), allow_pickle=False)
        else:
            from ..trainer.resnet_trainer import synthetic_imagenet

            t_imgs, t_labels = synthetic_imagenet(int(exec_properties["num_synthetic"]),
                                                  int(exec_properties["image_size"]),
                                                  int(exec_properties["num_classes"]), int(exec_properties["seed"]))
            imgs, labels = t_imgs.numpy(), t_labels.numpy()
        tr, ev = _split_ids(len(labels))
        for art in output_dict["examples"]:
            sel = tr if art.split == "train" else ev
            os.makedirs(art.uri, exist_ok=True)
            np.save(os.path.join(art.uri, "images.npy"), np.ascontiguousarray(imgs[sel]))
            np.save(os.path.join(art.uri, "labels.npy"), labels[sel].astype(np.int64))
            art.custom_properties["num_examples"] = int(len(sel))


class ImageExampleGen(_KwComponent):
    SPEC_CLASS = ImageExampleGenSpec
    EXECUTOR_CLASS = ImageExampleGenExecutor
    EXECUTION_TYPE = "examples_gen"
    OUTPUT_SPLITS = {"examples": ["train", "eval"]}


class ImageTransformSpec(ComponentSpec):
    INPUTS = {"input_data": ChannelParameter(A.EXAMPLES)}
    OUTPUTS = {"transform_output": ChannelParameter(A.TRANSFORM)}
    PARAMETERS = {"crop": ExecutionParameter(optional=True, default=224),
                  "augment": ExecutionParameter(optional=True), "rrc_scale": ExecutionParameter(optional=True),
                  "rrc_ratio": ExecutionParameter(optional=True), "eval_resize": ExecutionParameter(optional=True)}


class ImageTransformExecutor(BaseExecutor):
    def Do(self, input_dict, output_dict, exec_properties):  # noqa: N802
        train = next(a for a in input_dict["input_data"] if a.split == "train")
        imgs = np.load(os.path.join(train.uri, "images.npy"), mmap_mode="r", allow_pickle=False)
        mean, std = _channel_stats(imgs)
        out = output_dict["transform_output"][0]
        os.makedirs(out.uri, exist_ok=True)
        with open(os.path.join(out.uri, "image_transform.json"), "w") as f:
            json.dump({"mean": mean, "std": std, "crop": int(exec_properties.get("crop") or 224),
                       **resolve_input_config(exec_properties, given_only=True)}, f)


def _channel_stats(imgs: np.ndarray):
    """Per-channel mean / std of pixel/255 over the whole split (fp64; HIP moments kernel on GPU)."""
    from ..ops import analyzers

    dev = None
    try:
        import torch

        dev = "cuda" if torch.cuda.is_available() else None
    except ImportError:
        pass
    C = imgs.shape[-1]
    mean, std = [], []
    for c in range(C):
        col = np.asarray(imgs[..., c], dtype=np.float64).reshape(-1) / 255.0
        m = analyzers.column_moments(col, device=dev)
        mean.append(float(m["mean"]))
        std.append(float(m["std"]))
    return mean, std


class ImageTransform(_KwComponent):
    SPEC_CLASS = ImageTransformSpec
    EXECUTOR_CLASS = ImageTransformExecutor
    EXECUTION_TYPE = "transform"


class ImageTrainerSpec(ComponentSpec):
    INPUTS = {"examples": ChannelParameter(A.EXAMPLES), "transform_output": ChannelParameter(A.TRANSFORM)}
    OUTPUTS = {"output": ChannelParameter(A.MODEL)}
    PARAMETERS = {"train_steps": ExecutionParameter(optional=True, default=100),
                  "batch_size": ExecutionParameter(optional=True, default=64),
                  "learning_rate": ExecutionParameter(optional=True, default=0.1),
                  "num_classes": ExecutionParameter(optional=True, default=1000),
                  "custom_config": ExecutionParameter(optional=True)}


def resolve_optimizer_config(cc: dict, learning_rate: float, train_steps: int) -> dict:
    """custom_config -> the ResNetTrainer optimizer arguments (what the result records under "optimizer"). With
    lr_schedule unset the learning rate is the linear warmup over train_steps // 10 steps, then constant."""
    kind = cc.get("lr_schedule") or "constant"
    if kind not in ("constant", "cosine", "poly"):
        raise ValueError(f'lr_schedule must be "constant", "cosine" or "poly", got {kind!r}')
    decays = kind != "constant"
    if not decays and cc.get("end_lr"):
        raise ValueError('end_lr needs lr_schedule="cosine" or "poly"')
    lars = bool(cc.get("lars", False))
    if not lars and (cc.get("lars_eta") is not None or cc.get("lars_clip")):
        raise ValueError("lars_eta / lars_clip need lars")
    return {"learning_rate": float(learning_rate), "lr_schedule": kind, "warmup_steps": max(1, train_steps // 10),
            "total_steps": int(train_steps) if decays else None, "end_lr": float(cc.get("end_lr", 0.0) or 0.0),
            "lars": lars, "lars_eta": float(cc.get("lars_eta", 0.001) if lars else 0.001),
            "lars_clip": bool(cc.get("lars_clip", False)), "label_smoothing": float(cc.get("label_smoothing", 0.0))}


def resolve_input_config(tf: dict, given_only: bool = False) -> dict:
    """The input recipe keys of ImageTransform's parameters / image_transform.json -> the ResNetTrainer arguments
    (what the result records under "input"). given_only: just the keys that are set (what the Transform writes: a
    JSON without them behaves as before)."""
    from ..ops.image_ops import RRC_RATIO, RRC_SCALE, check_rrc_ranges

    aug = tf.get("augment") or None
    if aug == "none":
        aug = None
    if aug not in (None, "random_resized_crop"):
        raise ValueError(f'augment must be "random_resized_crop" or unset, got {aug!r}')
    if aug is None and (tf.get("rrc_scale") is not None or tf.get("rrc_ratio") is not None):
        raise ValueError("rrc_scale / rrc_ratio need augment")
    scale = tuple(float(v) for v in (tf.get("rrc_scale") or RRC_SCALE))
    ratio = tuple(float(v) for v in (tf.get("rrc_ratio") or RRC_RATIO))
    check_rrc_ranges(scale, ratio)
    ev = tf.get("eval_resize")
    out = {"augment": aug, "rrc_scale": list(scale), "rrc_ratio": list(ratio),
           "eval_resize": None if ev is None else int(ev)}
    if given_only:
        out = {k: v for k, v in out.items() if tf.get(k) is not None and (k != "augment" or aug is not None)}
    return out


def run_image_rank(spec: dict) -> dict:
    """One rank (or the only process) of the image Trainer: ResNet-50 v2 on the examples of `spec`, resuming
    from the latest checkpoint in <out>/serving_model_dir, checkpointing every `checkpoint_every` steps (rank 0
    writes, every rank resumes from the same file), evaluating and exporting on rank 0. `batch_size` is per
    replica (W ranks train W x batch_size images per step); `accum_steps` micro-batches per replica and step."""
    import numpy as np
    import torch

    from ..serving.saved_model import save_module
    from ..trainer.resnet_trainer import ResNetTrainer

    pg = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
    rank = torch.distributed.get_rank() if pg is not None else 0
    world = torch.distributed.get_world_size() if pg is not None else 1
    cc = spec.get("custom_config") or {}
    with open(os.path.join(spec["transform_uri"], "image_transform.json")) as f:
        tf = json.load(f)
    # every rank maps the whole split; each step's global sample is drawn from (seed, step) (ResNetTrainer)
    imgs = torch.from_numpy(np.load(os.path.join(spec["train_uri"], "images.npy"), allow_pickle=False))
    labels = torch.from_numpy(np.load(os.path.join(spec["train_uri"], "labels.npy"), allow_pickle=False))
    dev = spec.get("device") or ("cuda" if torch.cuda.is_available() else "cpu")
    if dev == "cuda" and world > 1:
        dev = f"cuda:{0 if os.environ.get('MIFX_SHARED_GPU') == '1' else int(os.environ.get('LOCAL_RANK', 0))}"
    steps = int(spec["train_steps"])
    oc = resolve_optimizer_config(cc, float(spec["learning_rate"]), steps)
    ic = resolve_input_config(tf)
    tr = ResNetTrainer(int(spec["batch_size"]), dev, imgs, labels, num_classes=int(spec["num_classes"]),
                       lr=oc["learning_rate"], warmup_steps=oc["warmup_steps"], mean=tuple(tf["mean"]),
                       std=tuple(tf["std"]), crop=int(tf["crop"]), process_group=pg, seed=int(cc.get("seed", 0)),
                       accum_steps=int(cc.get("accum_steps", 1)), lr_schedule=oc["lr_schedule"],
                       total_steps=oc["total_steps"], end_lr=oc["end_lr"], lars=oc["lars"], lars_eta=oc["lars_eta"],
                       lars_clip=oc["lars_clip"], label_smoothing=oc["label_smoothing"], augment=ic["augment"],
                       rrc_scale=tuple(ic["rrc_scale"]), rrc_ratio=tuple(ic["rrc_ratio"]),
                       eval_resize=ic["eval_resize"])
    model_dir = os.path.join(spec["out_dir"], "serving_model_dir")
    ck = ResNetTrainer.latest_checkpoint(model_dir)
    if ck:
        tr.restore(ck)
    every = int(cc.get("checkpoint_every", 0) or 0)
    loss = torch.tensor(float("nan"))
    import time

    t0, s0 = time.time(), tr.step_idx
    while tr.step_idx < steps:
        loss = tr.step()
        if every and tr.step_idx % every == 0 and tr.step_idx < steps:
            if rank == 0:
                tr.save_checkpoint(model_dir)
            if pg is not None:
                torch.distributed.barrier()
    if tr.device.type == "cuda":
        torch.cuda.synchronize(tr.device)
    tr.check()
    secs = time.time() - t0
    res = {"final_loss": float(loss), "world": world, "steps": tr.step_idx, "resumed_from": ck,
           "train_images_per_sec": (tr.step_idx - s0) * tr.batch * tr.accum * world / max(secs, 1e-9),
           "optimizer": dict(oc, final_lr=tr.last_lr()), "input": tr.input_recipe()}
    if rank == 0:
        tr.save_checkpoint(model_dir)
        ev_imgs = torch.from_numpy(np.load(os.path.join(spec["eval_uri"], "images.npy"), allow_pickle=False))
        ev_labels = torch.from_numpy(np.load(os.path.join(spec["eval_uri"], "labels.npy"), allow_pickle=False))
        res["eval_accuracy"] = tr.evaluate(ev_imgs, ev_labels)
        save_module(os.path.join(model_dir, "export", "1"), tr.model.cpu().float(), "mifx.models.resnet:ResNetV2",
                    {"num_classes": int(spec["num_classes"])}, [3, tf["crop"], tf["crop"]])
    if pg is not None:
        torch.distributed.barrier()
    return res


class ImageTrainerExecutor(BaseExecutor):
    """custom_config: num_gpus (> 1: one rank per GPU launched by the component itself, mifx.trainer.distributed;
    the reference runs its ResNet-50 workers as a hand-written TFJob, `tf-job-simple-v1beta2.jsonnet:22-40`),
    checkpoint_every (steps; resume from the latest checkpoint like the reference's Saver,
    `research/pate_2017/deep_cnn.py:489,541-542`), accum_steps, seed, timeout_s. Optimizer recipe
    (`resolve_optimizer_config`; recorded in metrics.json under "optimizer" and in the output's custom properties):
    lr_schedule ("constant" | "cosine" | "poly", decaying to end_lr at train_steps), lars, lars_eta, lars_clip,
    label_smoothing. The input recipe (augment, rrc_scale, rrc_ratio, eval_resize) comes from the Transform's
    image_transform.json; the resolved settings are recorded in metrics.json under "input" and in the output's custom
    properties (input_augment, input_rrc_scale_lo / _hi, input_rrc_ratio_lo / _hi, input_eval_resize)."""

    def Do(self, input_dict, output_dict, exec_properties):  # noqa: N802
        ex = {a.split: a.uri for a in input_dict["examples"]}
        out = output_dict["output"][0]
        cc = dict(exec_properties.get("custom_config") or {})
        spec = {"train_uri": ex["train"], "eval_uri": ex.get("eval", ex["train"]), "out_dir": out.uri,
                "transform_uri": input_dict["transform_output"][0].uri,
                "train_steps": int(exec_properties["train_steps"]), "batch_size": int(exec_properties["batch_size"]),
                "learning_rate": float(exec_properties["learning_rate"]),
                "num_classes": int(exec_properties["num_classes"]), "custom_config": cc,
                "device": self.context.device or self.context.extra.get("device"),
                "hparams": {"device": self.context.device or self.context.extra.get("device")}}
        n = int(cc.get("num_gpus", 1) or 1)
        if n > 1:
            from ..trainer import distributed

            work = os.path.join(out.uri, "dp_run")
            res = distributed.launch(dict(spec, target="mifx.components.image:run_image_rank", work_dir=work), n, work,
                                     timeout=cc.get("timeout_s"))
        else:
            res = run_image_rank(spec)
        with open(os.path.join(out.uri, "metrics.json"), "w") as f:
            json.dump(res, f, default=float)
        out.custom_properties.update({"eval_accuracy": float(res["eval_accuracy"]),
                                      "final_loss": float(res["final_loss"]), "num_replicas": int(res["world"]),
                                      "train_images_per_sec": float(res["train_images_per_sec"])})
        # the resolved optimizer recipe (bools as 0 / 1, unset values left out: MLMD properties are int / float / str)
        out.custom_properties.update({k: int(v) if isinstance(v, bool) else v
                                      for k, v in (res.get("optimizer") or {}).items() if v is not None})
        inp = res.get("input") or {}
        if inp:
            out.custom_properties["input_augment"] = str(inp["augment"])
            for k in ("rrc_scale", "rrc_ratio"):
                out.custom_properties[f"input_{k}_lo"], out.custom_properties[f"input_{k}_hi"] = map(float, inp[k])
            if inp.get("eval_resize") is not None:
                out.custom_properties["input_eval_resize"] = int(inp["eval_resize"])
        self.context.logger.info("ImageTrainer: %d replica(s), loss %.4f eval accuracy %.4f", res["world"],
                                 res["final_loss"], res["eval_accuracy"])


class ImageTrainer(_KwComponent):
    SPEC_CLASS = ImageTrainerSpec
    EXECUTOR_CLASS = ImageTrainerExecutor
    EXECUTION_TYPE = "trainer"
