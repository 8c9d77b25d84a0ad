"""Device-resident, hipGraph-captured Wide&Deep trainer on the GENERAL fused gfx950 kernel (csrc/wd_general.hip):
any DNN tower of 1..6 hidden layers and widths 2..256, single GPU.

One training step = ``wdg_fused`` (forward + loss + backward, one fp32 gradient slab per workgroup) ->
``wdg_reduce_opt`` (slab rows summed in row order + Adagrad / FTRL / Adam / SGD + both bf16 weight images). The
master weights and optimizer slots live in slab-column order (models.wide_deep.general_layout); the step and the
data offset advance through a device-side counter, so a step (or S steps) replays as one hipGraph. Slower than the
chained kernel, which is compiled for the taxi tower and stays the default for it (trainer.dispatch); this is the
path for every other `hidden_units`. The surface is FusedWideDeepTrainer's, as the estimator and serving use it.

dp=DPSpec(...): differentially private training, per example. The fused kernel measures every example's gradient
norm through the exact layer-wise factorisation, clips by c_i = min(1, s C / n_i) inside the step (no per-example
gradient is ever materialised) and the reduce / optimizer pass adds the Gaussian noise from a Philox stream keyed by
(seed, optimizer step): graph replays draw fresh noise without host state, a resumed run continues the stream.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from ..models import wide_deep as wdm
from ..ops import wd_general as wdg
from ..privacy.spec import DPSpec
from .fused_wide_deep import OptSpec, default_dnn_opt, default_wide_opt


class GeneralWideDeepTrainer:
    def __init__(self, model: wdm.WideDeepModel | None = None, batch: int = 40, device="cuda",
                 dnn_opt: OptSpec | None = None, wide_opt: OptSpec | None = None, loss_reduction: str = "sum",
                 grid: int | None = None, process_group=None, max_grid: int = 256, shuffle_seed: int = 0,
                 feed_stride: int | None = None, feed_offset: int = 0, dp: DPSpec | None = None):
        """grid: workgroups of the fused launch (default: one per 64-example tile, at most max_grid and at most what
        keeps grid x slab bytes inside the kernel's slab bound). shuffle_seed / feed_stride / feed_offset: the record
        stream of csrc/feed.h, as FusedWideDeepTrainer. dp: per-example DP-SGD (privacy.DPSpec); None launches
        exactly the non-private step."""
        self.device = torch.device(device)
        self.model = model or wdm.WideDeepModel()
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.dp = dp
        if dp is not None and self.world > 1:
            raise ValueError(f"DP training is single-GPU: the clipped, noised step runs on the general fused kernel, "
                             f"which has no data-parallel path (world = {self.world})")
        if self.world > 1:
            raise ValueError(f"general towers are single-GPU: hidden_units {list(self.model.cfg.hidden_units)} train "
                             f"on the general fused kernel, which has no data-parallel path (world = {self.world})")
        self.layout = lay = wdm.general_layout(self.model.cfg)  # ValueError names the limit it breaks
        c = wdg.constants()
        self.T = c["T"]
        self.kernel = "general"
        self.batch = int(batch)
        if dp is not None:
            dp.check_batch(self.batch)
        self.shuffle_seed = int(shuffle_seed)
        self.feed_stride = int(feed_stride) if feed_stride is not None else self.batch
        self.feed_offset = int(feed_offset)
        if not (self.feed_stride >= self.batch and 0 <= self.feed_offset <= self.feed_stride - self.batch):
            raise ValueError("need feed_stride >= batch and 0 <= feed_offset <= feed_stride - batch")
        self.stride, self.wtot = lay.stride, lay.wtot
        ntiles = (self.batch + self.T - 1) // self.T
        self.grid = int(min(grid or ntiles, ntiles, max_grid, wdg.max_grid(self.stride)))
        self.dnn_opt = dnn_opt or default_dnn_opt()
        self.wide_opt = wide_opt or default_wide_opt(len(self.model.cfg.wide))
        self.loss_reduction = loss_reduction
        dev = self.device
        self.gidx_np = lay.pidx  # flat parameter -> slab column
        self._pidx = torch.from_numpy(lay.pidx).to(dev)
        self.kind = torch.from_numpy(lay.kind).to(dev)
        self.desc_dev = torch.from_numpy(lay.desc).to(dev)
        self.param_sc = torch.zeros(self.stride, device=dev)
        self.s0_sc = torch.zeros(self.stride, device=dev)
        self.s1_sc = torch.zeros(self.stride, device=dev)
        self.wt = torch.zeros(2 * self.wtot, dtype=torch.int16, device=dev)
        s0 = np.zeros(wdm.flat_size(self.model.cfg), np.float32)
        nd = s0.size - wdm.NWIDE
        for sl, spec in ((slice(0, nd), self.dnn_opt), (slice(nd, None), self.wide_opt)):
            if spec.kind in ("adagrad", "ftrl"):
                s0[sl] = spec.initial_accumulator_value
        self._set_flat(wdm.pack_flat(self.model), s0, np.zeros_like(s0))
        self.step_ctr = torch.zeros(c["SLOTS"], dtype=torch.int64, device=dev)
        self.slab = torch.zeros(self.grid, self.stride, device=dev)
        self.slab_loss = torch.zeros(self.grid, device=dev)
        self.scratch = torch.zeros(self.grid * lay.scratch, dtype=torch.int16, device=dev)
        self.grad = torch.empty(self.stride, device=dev)
        self.norms = torch.zeros(self.batch, device=dev) if dp is not None else None
        self.h_dnn = self.dnn_opt.encode()
        self.h_wide = self.wide_opt.encode()
        self.records = None
        self.n_data = 0
        self.graph = None
        self.graph_multi, self.graph_multi_steps = None, 1

    # ---------------------------------------------------------------- master state
    def _set_flat(self, param=None, s0=None, s1=None) -> None:
        """Overwrite weights / slots from flat-order vectors; re-emits both bf16 images."""
        for name, v in (("param", param), ("s0", s0), ("s1", s1)):
            if v is None:
                continue
            v = torch.as_tensor(np.asarray(v, dtype=np.float32)).to(self.device)
            getattr(self, name + "_sc")[self._pidx] = v
        if param is not None:
            self.param_sc[torch.from_numpy(self.layout.ones).to(self.device)] = 1.0  # the constant-1 producers
            self.wt.copy_(self._weight_image())

    def _flat(self, v_sc: torch.Tensor) -> np.ndarray:
        return v_sc[self._pidx].cpu().numpy()

    def _weight_image(self) -> torch.Tensor:
        """bf16 (as int16) [2 * WTOT]: per layer W^T [N][K], then per layer W [K][N]."""
        p = self.param_sc[: self.wtot].to(torch.bfloat16)
        tr = [p[o:o + k * n].reshape(n, k).t().reshape(-1) for k, n, o in zip(self.layout.K, self.layout.N,
                                                                             self.layout.off)]
        return torch.cat([p] + tr).view(torch.int16).contiguous()

    @property
    def wide_weights(self) -> torch.Tensor:
        return self.param_sc[self.wtot:self.wtot + wdm.NWIDE]

    def _state_vec(self, v_sc: torch.Tensor) -> torch.Tensor:
        """A slab-order state vector in the checkpoint layout (models.wide_deep.pack_state)."""
        m = copy.deepcopy(self.model).cpu()
        wdm.unpack_flat(self._flat(v_sc), m)
        return torch.from_numpy(wdm.pack_state(m))

    def _from_state_vec(self, vec) -> np.ndarray:
        m = copy.deepcopy(self.model).cpu()
        wdm.unpack_state(vec, m)
        return wdm.pack_flat(m)

    @property
    def param(self) -> torch.Tensor:
        """fp32 master weights in the checkpoint layout (a copy)."""
        return self._state_vec(self.param_sc)

    # ---------------------------------------------------------------- data
    def set_data(self, records: torch.Tensor) -> None:
        """records: uint8 [N, 32] packed taxi records (see models.wide_deep.RECORD_DTYPE)."""
        if records.dim() != 2 or records.shape[1] != 32 or records.dtype != torch.uint8:
            raise ValueError("records must be uint8 [N, 32]")
        if records.shape[0] < self.batch:
            raise ValueError(f"{records.shape[0]} records < one batch of {self.batch}")
        self.records = records.to(self.device).contiguous()
        self.n_data = self.records.shape[0]
        self.graph, self.graph_multi, self.graph_multi_steps = None, None, 1

    @property
    def grad_scale(self) -> float:
        return 1.0 if self.loss_reduction == "sum" else 1.0 / self.batch

    def feed_args(self) -> tuple[int, int, int]:
        return self.feed_stride, self.feed_offset, self.shuffle_seed & (2**64 - 1)

    # ---------------------------------------------------------------- step
    def _fwd_bwd(self) -> None:
        wdg.fused(self.records, self.n_data, self.batch, 0, self.step_ctr, self.wt, self.wide_weights, self.slab,
                  self.slab_loss, None, self.grad_scale, self.grid, True, self.layout.desc, self.desc_dev,
                  self.scratch, self.layout.scratch, feed=self.feed_args(),
                  **({} if self.dp is None else {"l2_norm_clip": self.dp.l2_norm_clip, "norms_out": self.norms}))

    def _dp_reduce(self, noise: bool):
        """The dp argument of ops.wd_general.reduce_*: (noise stddev or None, grad_scale, seed)."""
        if self.dp is None:
            return None
        return (self.dp.stddev if noise and self.dp.noise_multiplier > 0 else None, self.grad_scale, self.dp.seed)

    def _step_impl(self) -> None:
        self._fwd_bwd()
        wdg.reduce_apply(self.slab, self.grid, self.kind, self.param_sc, self.s0_sc, self.s1_sc, self.wt,
                         self.step_ctr, self.h_dnn, self.h_wide, dp=self._dp_reduce(True))

    def step(self) -> None:
        if self.records is None:
            raise RuntimeError("call set_data() first")
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step_impl()

    def run(self, n: int) -> None:
        """n training steps; with a multi-step graph (capture(steps_per_graph=S)) n // S replays of it first."""
        if self.graph_multi is not None and n >= self.graph_multi_steps:
            reps, n = divmod(n, self.graph_multi_steps)
            for _ in range(reps):
                self.graph_multi.replay()
        for _ in range(n):
            self.step()

    def capture(self, warmup: int = 2, steps_per_graph: int = 1) -> None:
        """Capture the step as a hipGraph (plus an S-step graph when steps_per_graph > 1) after `warmup` eager
        steps on a side stream."""
        if self.records is None:
            raise RuntimeError("call set_data() first")
        self.predict_logits(self.records[:1])  # first launch (module load, LDS limit) outside the capture
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step_impl()
        torch.cuda.current_stream(self.device).wait_stream(s)
        self.graph, self.graph_multi, self.graph_multi_steps = None, None, 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_impl()
        self.graph = g
        if steps_per_graph > 1:
            gm = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gm):
                for _ in range(steps_per_graph):
                    self._step_impl()
            self.graph_multi, self.graph_multi_steps = gm, int(steps_per_graph)

    # ---------------------------------------------------------------- introspection
    def last_loss(self) -> float:
        """Sum of per-example losses of the most recent step."""
        return float(self.slab_loss.sum().item())

    @property
    def steps_done(self) -> int:
        return int(self.step_ctr[0].item())

    def set_step(self, step: int) -> None:
        self.step_ctr.fill_(int(step))

    def last_norms(self) -> torch.Tensor:
        """DP: the [batch] device buffer of per-example gradient L2 norms (before clipping) of the latest step or
        gradients_once(), by position in the batch."""
        if self.dp is None:
            raise RuntimeError("last_norms() needs a trainer built with dp=DPSpec(...)")
        return self.norms

    def gradients_once(self, noise: bool = False) -> np.ndarray:
        """Forward / backward on the current batch WITHOUT updating; the summed slab row (index it with
        `self.gidx_np` for the flat parameter order of models.wide_deep.pack_flat). DP: the sum of the clipped
        per-example gradients, with noise=True plus the noise the optimizer step at the current step would add."""
        if self.records is None:
            raise RuntimeError("call set_data() first")
        if noise and self.dp is None:
            raise ValueError("gradients_once(noise=True) needs a trainer built with dp=DPSpec(...)")
        self._fwd_bwd()
        wdg.reduce_sum(self.slab, self.grid, self.grad, dp=self._dp_reduce(noise), kind=self.kind,
                       step_ctr=self.step_ctr)
        return self.grad.cpu().numpy()

    @torch.no_grad()
    def predict_logits(self, records: torch.Tensor) -> torch.Tensor:
        records = records.to(self.device).contiguous()
        n = records.shape[0]
        out = torch.empty(n, device=self.device)
        if n == 0:
            return out
        grid = min((n + self.T - 1) // self.T, 1024)
        wdg.fused(records, n, n, 0, None, self.wt, self.wide_weights, None, None, out, 1.0, grid, False,
                  self.layout.desc, self.desc_dev, None)
        return out

    def sync_to_model(self) -> wdm.WideDeepModel:
        return wdm.unpack_flat(self._flat(self.param_sc), self.model)

    def state_dict(self) -> dict:
        return {"param": self._state_vec(self.param_sc), "s0": self._state_vec(self.s0_sc),
                "s1": self._state_vec(self.s1_sc), "step": self.step_ctr[:1].cpu()}

    def load_state_dict(self, sd: dict) -> None:
        """param / s0 / s1 in the checkpoint layout (None: keep); step."""
        vecs = {k: (self._from_state_vec(sd[k]) if sd.get(k) is not None else None) for k in ("param", "s0", "s1")}
        self._set_flat(vecs["param"], vecs["s0"], vecs["s1"])
        if sd.get("step") is not None:
            self.set_step(int(torch.as_tensor(sd["step"]).reshape(-1)[0]))
