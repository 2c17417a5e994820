"""`monodepth2` depth model plugin, the model of `--configure kitti` (reference: monodepth/monodepth2_model.py:15-93).

Class attributes (:17-19), the steps of `estimate_depth` (:61-91: bicubic resize to the feed size, encoder with its own (x - 0.45) / 0.225,
decoder's disp_0, bicubic resize back, reciprocal) and the no-op `save()` (:93; the fine-tuning therefore writes no checkpoint files) follow
the reference.  The network is restated in consistent_depth_amd/monodepth/monodepth2_net.py (ResNet-18 encoder + DepthDecoder) on the
hand-written kernels; the reciprocal is fused into the loss (depth_mode = DEPTH_RECIPROCAL), as for midas2.

Weights: upstream's format -- `encoder.pth` (the encoder's state dict plus `height`, `width`, `use_stereo`; filtered to the encoder's own
keys, :38-41) and `depth.pth` (the decoder's, loaded strictly) -- from the directory $CD_AMD_MONODEPTH2_WEIGHTS, else from the reference's
local path checkpoints/monodepth2_mono+stereo_1024x320/.  The feed size is read from `encoder.pth` (320 x 1024 for those weights).  Without
weights: a seeded random initialisation at feed 320 x 1024 (or `feed=`).  Nothing is ever downloaded.
"""
from __future__ import annotations

import os

import torch

from ..loss.consistency_loss import DEPTH_RECIPROCAL
from .depth_model import DepthModel

DEFAULT_WEIGHTS = os.path.join("checkpoints", "monodepth2_mono+stereo_1024x320")


class Monodepth2Model(DepthModel):
    align = 1
    learning_rate = 0.00004
    lambda_view_baseline = 1
    depth_mode = DEPTH_RECIPROCAL  # depth = 1 / disparity, :85

    def __init__(self, seed: int = 0, feed=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise RuntimeError("Monodepth2Model needs the HIP device (no CPU path in consistent_depth_amd)")
        from .monodepth2_net import FEED, Monodepth2Net
        self.device = torch.device("cuda", torch.cuda.current_device())
        wdir = os.environ.get("CD_AMD_MONODEPTH2_WEIGHTS") or DEFAULT_WEIGHTS
        files = [os.path.join(wdir, f) for f in ("encoder.pth", "depth.pth")]
        self.pretrained = all(os.path.isfile(f) for f in files)
        if not self.pretrained and os.environ.get("CD_AMD_MONODEPTH2_WEIGHTS"):
            raise FileNotFoundError(f"CD_AMD_MONODEPTH2_WEIGHTS={wdir}: encoder.pth and depth.pth expected there")
        enc = dec = None
        if self.pretrained:
            enc, dec = (torch.load(f, map_location="cpu") for f in files)
            stored = (int(enc["height"]), int(enc["width"]))
            if feed is not None and tuple(feed) != stored:
                raise ValueError(f"Monodepth2Model: feed {tuple(feed)} differs from the weights' {stored}")
            feed = stored
            print(f"Model was trained at {stored[1]} x {stored[0]}.")
        st = torch.random.get_rng_state()
        torch.manual_seed(seed)
        self.model = Monodepth2Net(feed if feed is not None else FEED)
        torch.random.set_rng_state(st)
        if self.pretrained:
            own = self.model.encoder.state_dict()
            self.model.encoder.load_state_dict({k: v for k, v in enc.items() if k in own})
            self.model.depth_decoder.load_state_dict(dec)
        self.model.to(self.device)

    @property
    def feed_height(self):
        return self.model.feed[0]

    @property
    def feed_width(self):
        return self.model.feed[1]

    def estimate_raw(self, images):
        """Disparity at frame size: (..., 3, H, W) -> (..., H, W)."""
        shape = images.shape
        C, H, W = shape[-3:]
        disp = self.model(images.reshape(-1, C, H, W).to(self.device))
        return disp.reshape(shape[:-3] + disp.shape[-2:])

    def estimate_depth(self, images):
        return self.estimate_raw(images).reciprocal()

    def weights_updated(self):
        """Called by the fine-tuning step after every optimiser update: the packed copies of the filters are stale."""
        self.model._pack_pool.invalidate()

    def save(self, file_name):
        pass
