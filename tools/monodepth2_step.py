#!/usr/bin/env python3
"""Step time of the monodepth2 fine-tuning (the `--configure kitti` model) on one GPU, outside bench.py (whose --model choices are fixed).

    python tools/monodepth2_step.py [--steps 20] [--warmup 3] [--frames 48] [--batch-size 4] [--height 384] [--width 224]

Synthetic clip of the BASELINE configs[2] frame shape resident on the device (PairStore.synthetic_device), batches of BS pairs from a
seeded shuffle, the model at feed 320 x 1024 (random init, seed 0), lambda_view_baseline and lr of the class.  Times `--steps` eager steps
(FineTuneStep) and then `--steps` graph replays (GraphedFineTuneStep) after their warm-up, and prints ONE JSON line: ms per step of
both and pairs/s of the graphed step.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=224)
    args = ap.parse_args()

    import torch
    from consistent_depth_amd import _native, build_native, parallel
    from consistent_depth_amd.engine import FineTuneStep, GraphedFineTuneStep
    from consistent_depth_amd.loaders.pair_store import PairStore
    from consistent_depth_amd.monodepth.depth_model_registry import get_depth_model
    build_native.build()
    _native.lib()
    dev = torch.device("cuda", 0)
    cls = get_depth_model("monodepth2")
    model = cls(seed=0)
    model.train()
    params = argparse.Namespace(lambda_reprojection=1.0, lambda_view_baseline=float(cls.lambda_view_baseline), lambda_parameter=0,
                                learning_rate=cls.learning_rate, optimizer="Adam")
    store = PairStore.synthetic_device(args.frames, args.height, args.width, seed=0, device=dev)
    B = args.batch_size
    plan = [ids for ids in parallel.shard_indices(len(store), 0, 0, 0, 1, B) if len(ids) == B]
    plan_dev = parallel.plan_to_device(plan, dev)
    pos = [0]

    def ids():
        pos[0] += 1
        return plan_dev[(pos[0] - 1) % len(plan_dev)]

    def timed(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = [step.step_from_store(store, ids())[0] for _ in range(n)]
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / n
        return ms, int(torch.isfinite(torch.stack([l.reshape(()) for l in losses])).sum())

    eager = FineTuneStep(model, params, world=1)
    timed(eager, args.warmup)
    eager_ms, eager_finite = timed(eager, args.steps)
    graphed = GraphedFineTuneStep(eager)
    timed(graphed, max(args.warmup, 3))          # 2 eager steps + the capture
    graph_ms, graph_finite = timed(graphed, args.steps)
    print(json.dumps({
        "tool": "monodepth2_step", "model": "monodepth2", "frame_hw": [args.height, args.width], "feed_hw": [model.feed_height, model.feed_width],
        "batch_size": B, "pairs": len(store), "steps": args.steps, "eager_ms_per_step": round(eager_ms, 3),
        "graphed_ms_per_step": round(graph_ms, 3), "graphed": graphed.graphed is True, "pairs_per_s": round(1e3 * B / graph_ms, 2),
        "finite_steps": [eager_finite, graph_finite], "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
