"""Times the image input kernels (csrc/image_ops.hip) at the ResNet-50 step's geometry: B images 256^2 uint8 ->
224^2 bf16. Three variants in one process, alternating after a warm-up:

  crop      the fixed-size crop kernel (crop_flip_normalize)
  rrc       box kernel + resample kernel (random_resized_crop_normalize, train mode, the defaults)
  identity  the resample kernel alone on a table of 224 x 224 boxes (the crop kernel's work through the new path)
  sampled   the resample kernel alone on the tables rrc samples, computed beforehand (rrc minus this = the box kernel
            and the second launch)
  full      the resample kernel on the whole image as the box (256^2 -> 224^2, the largest downscale of the geometry)

Each variant is captured once into a hipGraph of --calls calls, every call with its own sample of the dataset and
its own step (so successive calls read different images: with the default 8192 images the calls of one replay touch
far more than the 256 MiB Infinity Cache holds), and timed by device events over enough replays to fill --ms of
device time. Captured, the host's launch cost stays out of the figure.

Prints one JSON line per variant and round: microseconds per call, the bytes the variant must move (output
B x 224 x 224 x C x 2; input: the boxes' area x C, from the tables the variant used) and the resulting GB/s.

usage: python tools/bench_image_input.py [--batch 256] [--rounds 5] [--ms 300]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mifx.ops.image_ops import crop_flip_normalize, crop_params, random_resized_crop_normalize  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--calls", type=int, default=16, help="calls per captured graph")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ms", type=float, default=300.0, help="device time per variant and round")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_input needs a GPU")
    dev = torch.device("cuda")
    B, S, O, C, K = a.batch, a.size, a.crop, 3, a.calls
    g = torch.Generator(device=dev).manual_seed(0)
    imgs = torch.randint(0, 256, (a.images, S, S, C), dtype=torch.uint8, device=dev, generator=g)
    idxs = [torch.randint(0, a.images, (B,), device=dev, generator=g).to(torch.int32) for _ in range(K)]
    idents = []
    for k in range(K):
        oy, ox, flip = crop_params(B, S, S, O, O, True, 0, k)
        idents.append(torch.from_numpy(np.stack([ox, oy, np.full(B, O), np.full(B, O), flip], 1)).to(dev, torch.int32))

    def crop(k):
        return crop_flip_normalize(imgs, idxs[k], (O, O), True, 0, k)

    def rrc(k):
        return random_resized_crop_normalize(imgs, idxs[k], (O, O), True, 0, k)

    def identity(k):
        return random_resized_crop_normalize(imgs, idxs[k], (O, O), boxes=idents[k])

    tables = [random_resized_crop_normalize(imgs, idxs[k], (O, O), True, 0, k, return_boxes=True)[1] for k in range(K)]

    def sampled(k):
        return random_resized_crop_normalize(imgs, idxs[k], (O, O), boxes=tables[k])

    whole = torch.tensor([[0, 0, S, S, 0]] * B, dtype=torch.int32, device=dev)

    def full(k):
        return random_resized_crop_normalize(imgs, idxs[k], (O, O), boxes=whole)

    variants = {"crop": crop, "rrc": rrc, "identity": identity, "sampled": sampled, "full": full}
    out_bytes = B * O * O * C * 2
    area = int(C * np.mean([float((t[:, 2] * t[:, 3]).double().sum()) for t in tables]))
    in_bytes = {"crop": B * O * O * C, "identity": B * O * O * C, "rrc": area, "sampled": area,
                "full": B * S * S * C}

    graphs, keep = {}, []  # (keep: the captured calls' outputs stay allocated)
    for name, fn in variants.items():
        for k in range(K):  # warm-up: code objects, the cached constants
            fn(k)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for k in range(K):
                keep.append(fn(k))

    def timed(gr, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            gr.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / (n * K)  # ms per call

    reps = {}
    for name, gr in graphs.items():  # the replay count that fills --ms
        timed(gr, 3)
        reps[name] = max(5, int(a.ms / max(timed(gr, 5) * K, 1e-3)))
    for r in range(a.rounds):
        for name, gr in graphs.items():
            ms = timed(gr, reps[name])
            moved = out_bytes + in_bytes[name]
            print(json.dumps({"bench": "image_input", "variant": name, "round": r, "batch": B,
                              "calls": reps[name] * K, "us_per_call": 1e3 * ms, "out_bytes": out_bytes,
                              "in_bytes": in_bytes[name], "gb_per_s": moved / (ms * 1e-3) / 1e9}), flush=True)


if __name__ == "__main__":
    main()
