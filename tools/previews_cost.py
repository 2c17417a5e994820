#!/usr/bin/env python3
"""Wall time of ONE validation sweep (eval_and_save: 715 pairs of 384x224 in 179 batches) and of ONE save_depth (244 frames) on the
device-resident synthetic clip, with the colour-mapped previews on and off (CD_AMD_PREVIEWS), alternating, `--repeats` times each.
`--repo DIR` imports the package from another checkout (the parent commit, which knows no previews: both modes are then the same code).

    python tools/previews_cost.py [--frames 244] [--repeats 3] [--repo DIR]      -> profiles/previews.txt
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=244)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.repo)

import torch  # noqa: E402
from consistent_depth_amd.depth_fine_tuning import DepthFineTuner  # noqa: E402
from consistent_depth_amd.engine import FineTuneStep  # noqa: E402
from consistent_depth_amd.loaders.pair_store import PairStore  # noqa: E402
from consistent_depth_amd.params import Video3dParamsParser  # noqa: E402

tmp = tempfile.mkdtemp()
params = Video3dParamsParser().parse(["--path", tmp, "--batch_size", "4", "--print_freq", "0"])
store = PairStore.synthetic(args.frames, 384, 224, seed=0, device=torch.device("cuda", 0))
ft = DepthFineTuner(os.path.join(tmp, "run"), list(range(args.frames)), params, store=store)
os.makedirs(os.path.join(ft.out_dir, "eval"), exist_ok=True)
ft.model.train()
step = FineTuneStep(ft.model, params, world=1)
os.environ["CD_AMD_PREVIEWS"] = "1"
ft.eval_and_save(step, "_warm")            # plans, launch shapes, graph capture, the previews' range
ft.save_depth(os.path.join(tmp, "warm"))
ft.model.train()
torch.cuda.synchronize()
print(f"package from {args.repo}; {len(store)} pairs, {args.frames} frames, 384x224, BS4", flush=True)
times = {}
for r in range(args.repeats):
    for mode in ("1", "0"):
        os.environ["CD_AMD_PREVIEWS"] = mode
        out = os.path.join(tmp, f"d{r}{mode}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ft.eval_and_save(step, f"_r{r}m{mode}")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ft.save_depth(out)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ft.model.train()
        n_png = len([f for f in os.listdir(os.path.join(out, "depth")) if f.endswith(".png")])
        times.setdefault(mode, []).append((t1 - t0, t2 - t1))
        print(f"repeat {r} previews {'on ' if mode == '1' else 'off'}: validation sweep {t1 - t0:.3f} s, save_depth {t2 - t1:.3f} s ({n_png} PNGs)", flush=True)
        shutil.rmtree(out)
for mode, name in (("1", "on "), ("0", "off")):
    sweeps, saves = sorted(t[0] for t in times[mode]), sorted(t[1] for t in times[mode])
    print(f"previews {name}: validation sweep median {sweeps[len(sweeps) // 2]:.3f} s (min {sweeps[0]:.3f}, max {sweeps[-1]:.3f}); "
          f"save_depth median {saves[len(saves) // 2]:.3f} s (min {saves[0]:.3f}, max {saves[-1]:.3f})")
shutil.rmtree(tmp)
