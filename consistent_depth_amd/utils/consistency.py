"""Flow-consistency masks on the HIP device.

Mirrors the reference's utils/consistency.py (/root/reference/utils/consistency.py:53-67, used by
flow.py:199-228 `mask_valid_correspondences`): `consistent_flow_masks(flows, colors, flow_thresh, color_thresh)` takes
the two flows (H, W, 2) and the two colour images (H, W, C) of a pair as numpy arrays and returns the two boolean masks.
`consistent_flow_masks_batch` is the device-resident form for many pairs (NCHW tensors in, (B,1,H,W) 0/1 masks out --
what the loss consumes; see loaders/pair_store.py).  One fused kernel (cd_flow_consistency_masks) replaces the reference's
4 grid_sample calls + numpy reductions per pair; results are bit-identical to the reference's masks."""
from __future__ import annotations

import numpy as np
import torch

from .. import _native


def consistent_flow_masks_batch(flow_fwd, flow_bwd, color0, color1, flow_thresh=1.0, color_thresh=1.0):
    """flow_* (B,2,H,W), color* (B,C,H,W) fp32 on the HIP device -> (mask_fwd, mask_bwd), each (B,1,H,W) fp32 in {0,1}."""
    B, two, H, W = flow_fwd.shape
    if two != 2 or flow_bwd.shape != flow_fwd.shape or color0.shape != color1.shape or color0.shape[0] != B or \
            tuple(color0.shape[2:]) != (H, W):
        raise ValueError("expected flows (B,2,H,W) and colours (B,C,H,W) of the same pairs")
    f0, f1, c0, c1 = (t.float().contiguous() for t in (flow_fwd, flow_bwd, color0, color1))
    m0 = torch.empty(B, 1, H, W, dtype=torch.float32, device=f0.device)
    m1 = torch.empty_like(m0)
    rc = _native.lib().cd_flow_consistency_masks(
        _native.dev_ptr(f0, "flow_fwd"), _native.dev_ptr(f1, "flow_bwd"), _native.dev_ptr(c0, "color0"), _native.dev_ptr(c1, "color1"),
        c0.shape[1], float(flow_thresh), float(color_thresh), B, H, W, _native.dev_ptr(m0), _native.dev_ptr(m1), _native.stream_ptr(f0.device))
    _native.check(rc, "cd_flow_consistency_masks")
    return m0, m1


def consistent_flow_masks(flows, colors, flow_thresh, color_thresh, device=None):
    """The reference's call: flows = [fwd, bwd] (H,W,2), colors = [c0, c1] (H,W,C) numpy -> [mask_fwd, mask_bwd] bool (H,W)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).permute(2, 0, 1)[None].to(dev)  # noqa: E731
    colors = [np.asarray(c).reshape(c.shape[0], c.shape[1], -1) for c in colors]
    m0, m1 = consistent_flow_masks_batch(t(flows[0]), t(flows[1]), t(colors[0]), t(colors[1]), flow_thresh, color_thresh)
    return [m0[0, 0].cpu().numpy() > 0.5, m1[0, 0].cpu().numpy() > 0.5]


def flow_stage_masks(flows, color, pair_frames, flow_thresh=1.0, color_thresh=1.0, reverse_channels=False, masks=None, chunk=256):
    """The masks of P pairs in the pair store's layout, with their valid-pixel counts (cd_flow_stage_masks).

    flows (P,2,2,H,W) fp32 [pair, direction, (dx,dy)], color (F,C,H,W) fp32, pair_frames (P,2) int64 rows of `color` -- all on
    the HIP device, contiguous -> (masks (P,2,1,H,W) uint8 in {0,1}, counts (P,2) int32).  `masks`: an existing uint8 array of
    that shape to fill (PairStore.masks); every byte is overwritten.  reverse_channels: sum the colour differences from the
    last channel to the first -- for an R,G,B array this is the B,G,R order of the reference's files, and its masks bit for
    bit.  Frames are read in place through pair_frames; `chunk` pairs per launch."""
    for name, t, dt in (("flows", flows, torch.float32), ("color", color, torch.float32), ("pair_frames", pair_frames, torch.int64)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
        if not t.is_cuda:
            raise RuntimeError(f"{name}: must live on the HIP device (got {t.device}); consistent_depth_amd has no CPU path")
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"{name}: must be a contiguous {dt} tensor (got {t.dtype})")
    if flows.dim() != 5 or tuple(flows.shape[1:3]) != (2, 2) or color.dim() != 4 or tuple(color.shape[2:]) != tuple(flows.shape[3:]):
        raise ValueError("expected flows (P,2,2,H,W) and colours (F,C,H,W) of the same size")
    P, _, _, H, W = flows.shape
    F, C = color.shape[:2]
    if P <= 0 or F <= 0 or C <= 0 or tuple(pair_frames.shape) != (P, 2):
        raise ValueError(f"expected P > 0 pairs, F > 0 frames and pair_frames (P,2); got P={P}, F={F}, pair_frames {tuple(pair_frames.shape)}")
    if H < 2 or W < 2 or int(chunk) <= 0:
        raise ValueError(f"images of at least 2x2 and a positive chunk; got {H}x{W}, chunk={chunk}")
    lo, hi = int(pair_frames.min()), int(pair_frames.max())
    if lo < 0 or hi >= F:
        raise ValueError(f"pair_frames holds rows {lo}..{hi} of a colour array with {F} frames")
    dev = flows.device
    if masks is None:
        masks = torch.empty(P, 2, 1, H, W, dtype=torch.uint8, device=dev)
    elif not (isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dtype == torch.uint8 and masks.is_contiguous()
              and tuple(masks.shape) == (P, 2, 1, H, W)):
        raise ValueError(f"masks: expected a contiguous uint8 tensor of shape {(P, 2, 1, H, W)} on the HIP device")
    counts = torch.empty(P, 2, dtype=torch.int32, device=dev)
    chunk = min(int(chunk), 65535)
    for s in range(0, P, chunk):
        n = min(chunk, P - s)
        out = masks[s:s + n]
        aligned = out.data_ptr() % 4 == 0       # (an odd chunk of odd-sized planes starts off the word grid: staged and copied)
        buf = out if aligned else torch.empty_like(out)
        rc = _native.lib().cd_flow_stage_masks(
            flows[s:s + n].data_ptr(), color.data_ptr(), pair_frames[s:s + n].data_ptr(), C, int(bool(reverse_channels)),
            float(flow_thresh), float(color_thresh), n, F, H, W, buf.data_ptr(), counts[s:s + n].data_ptr(), _native.stream_ptr(dev))
        _native.check(rc, "cd_flow_stage_masks")
        if not aligned:
            out.copy_(buf)
    return masks, counts
