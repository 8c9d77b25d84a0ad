"""DPSpec: what a Wide&Deep trainer needs to train with per-example DP-SGD (clip, noise, seed)."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class DPSpec:
    """Per-example DP-SGD: every example's gradient is clipped to L2 norm `l2_norm_clip`, the clipped sum gets
    N(0, (noise_multiplier * l2_norm_clip)^2) per trainable entry and is then scaled as the loss reduction asks
    (GaussianAverageQuery for "mean"). seed keys the Philox noise stream (offset: the optimizer step), so a run is
    reproducible and a resumed run continues the stream. num_microbatches exists for the TF-Privacy signature only:
    the Wide&Deep trainers clip per example, so it must be None or the batch size."""
    l2_norm_clip: float
    noise_multiplier: float
    seed: int = 0
    num_microbatches: int | None = None

    def __post_init__(self):
        if not float(self.l2_norm_clip) > 0.0:
            raise ValueError("DPSpec: l2_norm_clip must be > 0")
        if not float(self.noise_multiplier) >= 0.0:
            raise ValueError("DPSpec: noise_multiplier must be >= 0")

    def check_batch(self, batch: int) -> None:
        if self.num_microbatches is not None and int(self.num_microbatches) != int(batch):
            raise ValueError(f"DP Wide&Deep training clips per example only: num_microbatches must be None or the "
                             f"batch size {batch}, got {self.num_microbatches}")

    @property
    def stddev(self) -> float:
        return float(self.noise_multiplier) * float(self.l2_norm_clip)
