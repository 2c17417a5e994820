"""The mask stage of a resident store, 256 pairs of 384x224 over 129 frames: PairStore.rebuild_masks' inner loop (framework gathers of
the colours + cd_flow_consistency_masks + fp32 -> u8 + the mask sums) against cd_flow_stage_masks (frames through pair_frames, byte
masks, counts from the same launch).  Wall time of the device work between two events, median of 9 repeats after a warm-up."""
import os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from consistent_depth_amd.utils import consistency
P, F, H, W = 256, 129, 384, 224
g = torch.Generator(device="cuda").manual_seed(0)
yy, xx = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
f0 = torch.stack([3.3 + 2 * torch.sin(yy / 60), -1.7 + 1.5 * torch.cos(xx / 45)])[None].repeat(P, 1, 1, 1) + torch.randn(P, 2, 1, 1, device="cuda", generator=g)
f1 = -f0 + torch.randn(P, 2, H, W, device="cuda", generator=g) * 0.3
flows = torch.stack([f0, f1], 1).contiguous()
color = torch.rand(F, 3, H, W, device="cuda", generator=g)
pf = torch.stack([torch.arange(P, device="cuda") // 2, torch.arange(P, device="cuda") // 2 + 1], 1).contiguous()
masks = torch.empty(P, 2, 1, H, W, dtype=torch.uint8, device="cuda")


def old():
    m0, m1 = consistency.consistent_flow_masks_batch(flows[:, 0].contiguous(), flows[:, 1].contiguous(), color[pf[:, 0]], color[pf[:, 1]])
    masks[:, 0] = (m0 > 0).to(torch.uint8)
    masks[:, 1] = (m1 > 0).to(torch.uint8)
    return masks.float().sum((2, 3, 4))


def new():
    return consistency.flow_stage_masks(flows, color, pf, masks=masks)[1]


def timed(fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts), out


a = timed(old); ref = masks.clone()
b = timed(new)
assert torch.equal(ref, masks) and torch.equal(a[3], b[3].float())
print(f"{P} pairs {H}x{W}, {F} frames (same masks and counts from both)")
print(f"rebuild_masks' loop (gather + fp32 masks + u8 + sums): median {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f})")
print(f"cd_flow_stage_masks (incl. the range check's sync):    median {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f})")
