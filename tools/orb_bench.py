"""Times the sparse-feature kernels (csrc/orb.hip) with device events, warm, median of 20 - recorded, not gated (DESIGN.md
section 4 item 39; the output is kept as profiles/orb.txt):
  prepare + detect + describe of one level at 640 x 480 and 1920 x 1080 (a seeded blocky texture, per_cell 4, threshold 20);
  gsr_hamming_vote of 2000 query descriptors against 100 frames x 2000 descriptors.
Next to every time the bytes or popcounts it implies: per pixel the image kernels read 3 floats and write 1 + 2 bytes (the u8
and box planes), then read the u8 plane once more; a vote compares Q x N pairs of 8 words, 8 popcounts each.

    python tools/orb_bench.py [--repeat 20]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))


def timed(fn, repeat):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    import scene_utils as S
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    print(f"orb_bench on {torch.cuda.get_device_name(0)}: median (min .. max) of {args.repeat} warm calls, device events")
    for W, H in ((640, 480), (1920, 1080)):
        blocks = torch.randint(0, 6, ((H + 4) // 5, (W + 4) // 5), generator=g).float() / 5.0
        grey = (0.1 + 0.8 * blocks).repeat_interleave(5, 0).repeat_interleave(5, 1)[:H, :W]
        img = grey.expand(3, H, W).contiguous().to(dev)
        state = {}

        def prepare():
            state["u8"], state["box"] = S.orb_prepare(img)

        def detect():
            state["slots"] = S.orb_detect(state["u8"], 20, 4)

        def describe():
            state["desc"] = S.orb_describe(state["u8"], state["box"], state["slots"].reshape(-1, 3))

        def all_three():
            prepare(), detect(), describe()
        px = W * H
        all_three()
        found = int((state["slots"][..., 2] > 0).sum())
        for name, fn, nbytes in (("prepare", prepare, px * (12 + 1 + 2 + 1)), ("detect", detect, px + state["slots"].numel() * 4),
                                 ("describe", describe, None), ("prepare + detect + describe", all_three, None)):
            med, lo, hi = timed(fn, args.repeat)
            note = "" if nbytes is None else f"   {nbytes / 1e6:.2f} MB moved at least = {nbytes / med / 1e6:.1f} GB/s"
            print(f"  {W} x {H}  {name:28s} {med:8.4f} ms ({lo:.4f} .. {hi:.4f}){note}")
        print(f"  {W} x {H}  {found} keypoints in {state['slots'].shape[0]} cells; describe: one wave per slot, 709 byte loads + 8 box loads "
              f"per lane group")
    Q, K, per = 2000, 100, 2000
    q = torch.randint(-2 ** 31, 2 ** 31 - 1, (Q, 8), generator=g, dtype=torch.int64).int().to(dev)
    db = S.PlaceDatabase(device=dev)
    for k in range(K):
        d = torch.randint(-2 ** 31, 2 ** 31 - 1, (per, 8), generator=g, dtype=torch.int64).int().to(dev)
        z = torch.zeros(per, dtype=torch.int32, device=dev)
        db.add(k, S.OrbFeatures(torch.zeros(per, 2, device=dev), z, z, z, d))
    med, lo, hi = timed(lambda: db.votes(q), args.repeat)
    pairs = Q * K * per
    print(f"  hamming_vote {Q} x ({K} x {per})       {med:8.4f} ms ({lo:.4f} .. {hi:.4f})   {pairs / 1e6:.0f} M pairs, {8 * pairs / 1e9:.1f} G "
          f"popcounts = {8 * pairs / med / 1e9:.2f} T popcounts/s; the database is {K * per * 32 / 1e6:.1f} MB, read once per 64 queries")
    med, lo, hi = timed(lambda: S.hamming_match(q, db._desc[:per]), args.repeat)
    print(f"  hamming_match {Q} x {per}             {med:8.4f} ms ({lo:.4f} .. {hi:.4f})")


if __name__ == "__main__":
    main()
