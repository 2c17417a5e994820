"""The flow stage in front of fine-tuning: masks of valid correspondences and the list of good frame pairs.

Mirrors the reference's `Flow` (/root/reference/flow.py:36-228) by method name.  The optical flow itself (FlowNet2,
`compute_flow`) is an INPUT here: `<path>/flow/flow_%06d_%06d.raw` must exist.  From those files and
`<path>/color_down/frame_%06d.raw` this class writes what the reference's pipeline writes next (process.py:73-80):

    <path>/mask/mask_%06d_%06d.png          8-bit 0 / 255, both directions of every pair    (mask_valid_correspondences)
    <out_path>/flow_list_%.2f.json          [[i,j],[j,i], ...] of the pairs whose two masks keep at least `overlap_ratio`
                                            of the pixels                                    (check_good_flow_pairs)

The masks come from cd_flow_stage_masks (csrc/flow_stage.hip) on colours in FILE channel order (B,G,R), `chunk` pairs per launch,
bit-identical to the reference's; the kernel also counts the valid pixels, so the pair filter does not read the PNGs back.
Importing this module needs no GPU; only `mask_valid_correspondences` touches the device.
"""
from __future__ import annotations

import json
import os
from os.path import join as pjoin

import numpy as np

from .utils import image_io


def _pair_key(pair):
    return (int(pair[0]), int(pair[1]))


class Flow:
    def __init__(self, path, out_path):
        self.path = path
        self.out_path = out_path
        self.flow_fmt = pjoin(path, "flow", "flow_{:06d}_{:06d}.raw")
        self.mask_fmt = pjoin(path, "mask", "mask_{:06d}_{:06d}.png")
        self.color_fmt = pjoin(path, "color_down", "frame_{:06d}.raw")
        self._ratios = {}        # (i, j) -> (valid pixels, H * W) of mask_i_j, for the masks this object computed

    @staticmethod
    def max_size():
        """Largest image side the flow network is run at (flow.py:41-44)."""
        return 1024

    def check_flow_files(self, index_pairs):
        return all(os.path.exists(self.flow_fmt.format(i, j)) for i, j in index_pairs)

    def compute_flow(self, index_pairs, checkpoint):
        raise NotImplementedError("optical flow is an input of this engine: put the reference's FlowNet2 output into "
                                  f"{os.path.dirname(self.flow_fmt)} (flow_%06d_%06d.raw); this stage starts from those files")

    def flow_pairs(self):
        """The unordered pairs (i < j) that have a flow file in either direction, ascending."""
        pairs = set()
        for name in os.listdir(os.path.dirname(self.flow_fmt)):
            stem, ext = os.path.splitext(name)
            if ext == ".raw" and stem.startswith("flow_"):
                i, j = (int(s) for s in stem.split("_")[1:3])
                pairs.add((min(i, j), max(i, j)))
        return sorted(pairs)

    def mask_valid_correspondences(self, flow_thresh=1, color_thresh=1, chunk=256):
        """Write both mask PNGs of every pair in flow/ that does not have both yet (the end state of the reference's loop)."""
        todo = []
        for i, j in self.flow_pairs():
            if all(os.path.isfile(self.mask_fmt.format(a, b)) for a, b in ((i, j), (j, i))):
                continue
            for a, b in ((i, j), (j, i)):
                if not os.path.isfile(self.flow_fmt.format(a, b)):
                    raise FileNotFoundError(f"{self.flow_fmt.format(a, b)}: pair ({i}, {j}) has the flow of one direction only")
            todo.append((i, j))
        os.makedirs(os.path.dirname(self.mask_fmt), exist_ok=True)
        if not todo:
            return
        import torch
        from .utils import consistency
        dev = torch.device("cuda", torch.cuda.current_device())
        colors = {}                                    # frame -> (C,H,W) host array in file channel order
        with image_io.AsyncRawWriter(device=dev, threads=image_io.PNG_ENCODER_THREADS) as writer:
            for s in range(0, len(todo), int(chunk)):
                part = todo[s:s + int(chunk)]
                frames = sorted({f for p in part for f in p})
                colors = {f: colors[f] if f in colors else self._load_color(f) for f in frames}
                row = {f: r for r, f in enumerate(frames)}
                flows = np.stack([np.stack([self._load_flow(a, b) for a, b in ((i, j), (j, i))]) for i, j in part])
                masks, counts = consistency.flow_stage_masks(
                    torch.from_numpy(flows).to(dev), torch.from_numpy(np.stack([colors[f] for f in frames])).to(dev),
                    torch.tensor([[row[i], row[j]] for i, j in part], dtype=torch.int64, device=dev),
                    flow_thresh, color_thresh, reverse_channels=False, chunk=len(part))
                images = masks * 255                   # the encoders of this chunk run while the next one is loaded and computed
                for n, (i, j) in enumerate(part):
                    for k, (a, b) in enumerate(((i, j), (j, i))):
                        writer.submit_png(self.mask_fmt.format(a, b), images[n, k, 0])
                hw = flows.shape[-2] * flows.shape[-1]
                for (i, j), c in zip(part, counts.cpu().tolist()):
                    self._ratios[(i, j)], self._ratios[(j, i)] = (c[0], hw), (c[1], hw)

    def _load_color(self, frame):
        im = image_io.load_raw_float32_image(self.color_fmt.format(frame))
        return np.ascontiguousarray(im.reshape(im.shape[:2] + (-1,)).transpose(2, 0, 1))

    def _load_flow(self, a, b):
        f = image_io.load_raw_float32_image(self.flow_fmt.format(a, b))
        if f.ndim != 3 or f.shape[-1] != 2:
            raise ValueError(f"{self.flow_fmt.format(a, b)}: flow must have 2 channels, got shape {f.shape}")
        return np.ascontiguousarray(f.transpose(2, 0, 1))

    def mask_ratio(self, i, j):
        """Valid fraction of mask_i_j as a Python float: from the stage's own count, else from the PNG (`> 0`)."""
        if (i, j) in self._ratios:
            count, hw = self._ratios[(i, j)]
        else:
            m = image_io.load_mask_png(self.mask_fmt.format(i, j))
            count, hw = int(np.count_nonzero(m)), m.shape[0] * m.shape[1]
        return count / hw

    def good_pairs(self, frame_pairs, overlap_ratio, ratio=None):
        """[pair, reversed pair, ...] of the pairs of `frame_pairs`, each visited once in order, whose two masks both keep at least
        `overlap_ratio` of the pixels.  ratio(i, j): the valid fraction of mask_i_j (default: `mask_ratio`)."""
        ratio = ratio or self.mask_ratio
        good, seen = [], set()
        for pair in frame_pairs:
            pair = _pair_key(pair)
            if pair in seen:
                continue
            both = [pair, pair[::-1]]
            seen.update(both)
            ratios = [ratio(*p) for p in both]
            if all(r >= overlap_ratio for r in ratios):
                good.extend(both)
            else:
                print(f"Bad frame pair({pair[0]}, {pair[1]}). Overlap_ratio=", ratios)
        print(f"Filtered {len(good)} / {len(frame_pairs)} good frame pairs")
        return good

    def check_good_flow_pairs(self, frame_pairs, overlap_ratio):
        flow_list_path = pjoin(self.out_path, "flow_list_%.2f.json" % overlap_ratio)
        if os.path.isfile(flow_list_path):
            return flow_list_path
        good = self.good_pairs(frame_pairs, overlap_ratio)
        if not good:
            raise Exception("No good frame pairs are found.")
        dists = np.array([abs(i - j) for i, j in good])
        print("Frame distance statistics: max = %d, mean = %d, median = %d" % (dists.max(), dists.mean(), np.median(dists)))
        with open(flow_list_path, "w") as f:
            json.dump([list(p) for p in good], f)
        return flow_list_path
