"""Entry into the fine-tuning stage on precomputed inputs.

The reference's DatasetProcessor.pipeline (/root/reference/process.py:38-99) runs ten stages;
everything before "Compute flow masks" (:73) is offline CPU/third-party work whose outputs are
inputs here.  This class keeps `create_output_path` (:22-29) so directories line up, checks that
the precomputed inputs exist, writes the flow masks and the good-pair list from the flows when
they are not there yet (:73-80, flow.py), then runs the two hot-path stages: fine_tune (:88) and
save_depth (:93).
"""
from __future__ import annotations

import glob
import os
import shutil
from os.path import join as pjoin

from . import parallel
from .depth_fine_tuning import DepthFineTuner
from .flow import Flow
from .loaders.video_dataset import read_pair_list
from .utils.frame_range import FrameRange
from .utils.frame_sampling import sample_pairs


class DatasetProcessor:
    def __init__(self, writer=None):
        self.writer = writer

    def create_output_path(self, params):
        name = f"R{params.frame_range.name}_{'-'.join(params.flow_ops)}_{params.model_type}"
        out_dir = pjoin(self.path, name)
        os.makedirs(out_dir, exist_ok=True)
        return out_dir

    def flow_stage_pairs(self, params):
        """The sampled frame pairs (process.py:50-70 without the scale stage's frame filter) that have flow files, in the
        sampler's order -- the `frame_pairs` of the reference's flow stage."""
        n_frames = len(glob.glob(pjoin(self.path, "color_down", "frame_*.raw")))
        flow = Flow(self.path, self.out_dir)
        return [p for p in sample_pairs(FrameRange(params.frame_range.set, n_frames), params.flow_ops)
                if flow.check_flow_files([p, p[::-1]])]

    def compute_flow_masks(self, params):
        """process.py:73-80 when its outputs are not there yet: mask PNGs of the pairs in flow/, the list of the sampled pairs with
        enough overlap, copied to <path>/flow_list.json.  A clip that has all of it is left alone (nothing is written)."""
        frame_pairs = self.flow_stage_pairs(params)
        if not frame_pairs:      # (nothing this stage could build from: the checks below report what is missing)
            return
        mask_fmt = pjoin(self.path, "mask", "mask_{:06d}_{:06d}.png")
        if os.path.isfile(pjoin(self.path, "flow_list.json")) and all(os.path.isfile(mask_fmt.format(*p)) for p in frame_pairs):
            return
        rank, _, world = parallel.env_world()
        if world > 1:
            parallel.init()
        if rank == 0:
            flow = Flow(self.path, self.out_dir)
            flow.mask_valid_correspondences()
            shutil.copyfile(flow.check_good_flow_pairs(frame_pairs, params.overlap_ratio), pjoin(self.path, "flow_list.json"))
        parallel.barrier()

    def process(self, params):
        self.path = params.path
        if params.op != "all":
            raise RuntimeError(f"operation '{params.op}' is an offline stage outside this engine")
        self.out_dir = self.create_output_path(params)
        required = (pjoin(self.path, "color_down"), pjoin(self.path, "flow"), pjoin(self.path, "mask"),
                    pjoin(self.out_dir, "metadata_scaled.npz"))
        if all(os.path.exists(p) for p in required if p != required[2]):
            self.compute_flow_masks(params)
        missing = [p for p in required if not os.path.exists(p)]
        if missing:
            raise FileNotFoundError("precomputed inputs missing (run the reference's offline stages or "
                                    f"tools/make_synthetic_dataset.py): {missing}")
        pairs = read_pair_list(self.path)
        frames = sorted({f for p in pairs for f in p})
        if params.frame_range.set.set is not None:
            frames = [f for f in frames if f in params.frame_range.set.set]
        print(f"Output directory: {self.out_dir}")
        ft = DepthFineTuner(self.out_dir, frames, params)
        ft.fine_tune(writer=self.writer)
        # one writer: rank 0 holds the checkpointed weights AND running statistics the exported depth must come from
        # (BatchNorm running statistics are rank-local during training, like nn.DataParallel's replica 0)
        if ft.rank == 0:
            ft.save_depth(ft.out_dir, frames)
        parallel.barrier()
        return None, ft.out_dir, frames
