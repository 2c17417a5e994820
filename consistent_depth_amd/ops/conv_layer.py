"""`HipConv2d`: an nn.Conv2d whose forward, input gradient and weight gradient run on the hand-written gfx950 MFMA kernels
(cd_conv2d_fwd / cd_conv2d_wgrad) -- the layer the MiDaS v2 backbone (BASELINE configs[4]) is built from.

Same parameters and state_dict keys as nn.Conv2d (a checkpoint loads unchanged).  Supported: square kernels 1/3/5/7/11,
"same" padding (k-1)/2, stride 1 or 2, any `groups`:
  * groups (ResNeXt's 32 x 8d 3x3): every group is a dense convolution on a channel slice of the SAME input / output
    buffers (the kernels address (tensor, channel offset, channels)); ALL groups run in ONE launch per pass
    (cd_conv2d_fwd_grouped / cd_conv2d_wgrad_grouped: the group is a grid dimension of the split-bf16 kernels) -- round 2
    issued one launch per group (32 x 33 bottlenecks x {forward, input gradient, weight gradient + unpack} = 4224 launches
    per step, which made the MiDaS step host-bound: 222 ms of enqueue for a 243 ms step).  At 8 channels per group a
    16-wide MFMA column tile is half empty;
  * stride 2: native kernels (csrc/conv_strided.hip) wherever cd_conv2d_strided_supported says yes -- 3x3 with >= 8 input channels per
    group, dense and grouped, on cd_conv2d_fwd_strided / _dgrad_strided / _wgrad_strided (no full-resolution output, no zero-stuffed
    gradient); 1x1 on cd_subsample2_fwd / _bwd around the stride-1 1x1 kernels; the 7x7 / 2 RGB stem (<= 4 input channels, dense) on
    cd_conv2d_stem_fwd / cd_conv2d_stem_wgrad (csrc/conv_stem.hip), which read the PLAIN filter -- such a layer has no packed filter
    and a PackPool skips it.  The stem kernels have NO input gradient (an image needs none, and 3 output channels would waste the
    matrix tile): if x.requires_grad, dx alone keeps the zero-stuffed dy + stride-1 path (and the layer its transposed pack), y and
    dw stay native and the other layers of a PackPool are not touched.  Elsewhere (arithmetic mode 0, CD_AMD_CONV_STRIDED=0 or, for the stem alone, CD_AMD_CONV_STEM=0 for A/B runs)
    the stride-1 "same" output sampled at even positions: identical values, 4x the MACs of a strided kernel and framework copy /
    fill kernels around it.
  * 1x1, dense (the bottleneck entry / exit convolutions: 2/3 of ResNeXt-101's multiply-adds, at 12x12 .. 96x96 images with
    256 .. 2048 channels): a plain GEMM  Y[n] = W [Cout x Cin] . X[n] [Cin x HW]  -- not a stencil.  On the hand-written kernels like
    everything else (no library GEMM on the path; rounds 3-5 carried a torch.matmul / bmm route behind CD_AMD_MIDAS_1X1=gemm, removed in
    round 6): >= 512 channels on the chunked split-bf16 kernel csrc/conv1x1_split.hip::conv1x1_split_kc_kernel (~100 TFLOP/s
    fp32-equivalent where the staged fp32-MFMA kernel reached 40-77) and wgrad1x1_split, 96x96 planes with <= 384 input channels on
    the LDS-resident 1x1 kernel.
Filters are re-packed once per forward (weights move under the optimiser): a `PackPool` shared by the layers of a network
packs EVERY filter of the network, forward and transposed layouts, in ONE table launch (round 2: two launches of 16 workgroups
per layer and pass -- 53 ms of a 211 ms MiDaS step); a layer outside a pool packs its own filters.
"""
from __future__ import annotations

import numpy as np
import torch


from .. import _native
from . import conv as C


class PackPool:
    """All HipConv2d layers of one network: their filters (forward + transposed layouts, every group) are packed by ONE
    cd_conv2d_pack_weights_table launch per `run()` -- call it once per forward, before the first layer."""

    def __init__(self):
        self.layers, self._table, self._key, self.fresh = [], None, None, False

    def register(self, layer):
        self.layers.append(layer)
        layer._pool = self

    def run(self):
        layers = [l for l in self.layers if l._uses_packed()]
        if not layers:      # (a pool of stem layers only: nothing to pack)
            self._key, self.fresh = (), True
            return
        key = tuple(l.weight.data_ptr() for l in layers)
        if key != self._key:      # first use, or the optimiser re-homed the parameters: rebuild the descriptors
            tabs = []
            for l in layers:
                w = l.weight
                if not (w.is_cuda and w.is_contiguous() and w.dtype == torch.float32):
                    raise RuntimeError("HipConv2d: weights must be contiguous fp32 on the HIP device (no CPU path)")
                l._pk, tab, l._arena = l._build(w, False)
                l._pkT, tabT, l._arenaT = l._build(w, True)
                l._wptr = w.data_ptr()
                tabs += [tab, tabT]
            self._table = torch.cat(tabs).contiguous()
            self._n = sum(2 * l.groups for l in layers)
            self._key = key
        if self._n > 65535:
            raise RuntimeError("PackPool: too many filters for one table launch")
        lib = _native.lib()
        _native.check(lib.cd_conv2d_pack_weights_table(self._table.data_ptr(), self._n, _native.stream_ptr(self._table.device)),
                      "cd_conv2d_pack_weights_table")
        self.fresh = True

    def invalidate(self):
        """The weights moved (an optimiser step): the packed copies are stale until the next run()."""
        self.fresh = False


def _dense_cfg(groups, ks, Cin, Cout, N, H, W, device):
    """(tile_rows, co_tiles) of the fastest launch shape of a DENSE k x k convolution (ops.conv.tuned_config: timed once per shape on
    scratch tensors, cached; the result does not depend on it), or None: grouped / 1x1 / tuning disabled (CD_AMD_MIDAS_CONV_TUNE=0) ->
    the library's rule.  Round 6: configs[4]'s decoder 3x3 convolutions had run on the rule's shape only."""
    import os
    if groups != 1 or ks < 3 or Cin < 8 or os.environ.get("CD_AMD_MIDAS_CONV_TUNE", "1") == "0":
        return None
    return C.tuned_config(ks, Cin, Cout, N, H, W, device)


_WGRAD_SIDE = {}


def _wgrad_side_stream(device):
    """The side stream of the weight gradients (one per device), or None under CD_AMD_MIDAS_WGRAD_STREAM=0."""
    import os
    if os.environ.get("CD_AMD_MIDAS_WGRAD_STREAM", "1") == "0":
        return None
    key = torch.device(device).index
    if key not in _WGRAD_SIDE:
        _WGRAD_SIDE[key] = torch.cuda.Stream(device=device)
    return _WGRAD_SIDE[key]


class _HipConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, layer):
        Cout, cin_g, ks, _ = weight.shape
        G, s = layer.groups, layer.stride[0]
        cout_g = Cout // G
        ctx.full_hw = None
        # stride 2 on the native kernels wherever the library has them (CD_AMD_CONV_STRIDED=0, arithmetic mode 0: the
        # stride-1-plus-sub-sampling path below)
        ctx.native_s2 = s == 2 and C.strided_enabled() and all(C.strided_supported(p, ks, 2, cin_g, cout_g) for p in (0, 1, 2))
        if ctx.native_s2 and ks == 3:
            x = x.contiguous()
            layer._packed(weight)
            y = C.conv2d_strided(x, layer._arena, cin_g, cout_g, ks, groups=G, bias=bias)
            ctx.layer, ctx.hw, ctx.s = layer, tuple(x.shape[2:]), s
            ctx.save_for_backward(x, weight)
            ctx.has_bias = bias is not None
            return y
        ctx.stem = layer._stem_now()
        if ctx.stem:               # the 7x7 / 2 RGB stem: y at output resolution from the plain filter
            if not (weight.is_cuda and weight.is_contiguous() and weight.dtype == torch.float32):
                raise RuntimeError("HipConv2d: weights must be contiguous fp32 on the HIP device (no CPU path)")
            x = x.contiguous()
            y = C.conv2d_stem(x, weight, bias)
            ctx.layer, ctx.hw, ctx.s = layer, tuple(x.shape[2:]), s
            ctx.save_for_backward(x, weight)
            ctx.has_bias = bias is not None
            return y
        if ks == 1 and s > 1:      # a strided 1x1 reads only the sampled pixels: sub-sample FIRST (exact, s^2 fewer multiply-adds)
            ctx.full_hw = tuple(x.shape[2:])
            x, s = (C.subsample2(x.contiguous()) if ctx.native_s2 else x[:, :, ::s, ::s]), 1
        x = x.contiguous()
        N, Cin, H, W = x.shape
        pk, _ = layer._packed(weight)
        y = torch.empty(N, Cout, H, W, dtype=torch.float32, device=x.device)
        cfg = _dense_cfg(G, ks, Cin, Cout, N, H, W, x.device)
        if cfg is not None:     # dense k x k (the decoder): the launch shape timed once per shape, like the hourglass engine does
            C.conv2d(x, pk[0], Cin, Cout, ks, bias=bias, out=y, cfg=cfg)
        else:
            C.conv2d_grouped(x, layer._arena, cin_g, cout_g, ks, G, bias=bias, out=y)      # (the arena: pk[0] .. pk[G-1] side by side)
        ctx.layer, ctx.hw, ctx.s = layer, (H, W), s
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y[:, :, ::s, ::s].contiguous() if s > 1 else y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        layer, (H, W) = ctx.layer, ctx.hw
        N, Cin = x.shape[:2]
        Cout, cin_g, ks, _ = weight.shape
        G, s = layer.groups, ctx.s
        cout_g = Cout // G
        if ctx.native_s2 and ks == 3:
            return _HipConvFn._backward_strided(ctx, dy)
        dyc = dy.contiguous() if ctx.stem else None
        if ctx.stem and not ctx.needs_input_grad[0]:
            dyf = None      # the stem's weight gradient reads dy at its own resolution: no full-resolution tensor
        elif s > 1:   # adjoint of the sub-sampling: zeros between the samples
            dyf = torch.zeros(N, Cout, H, W, dtype=torch.float32, device=dy.device)
            dyf[:, :, ::s, ::s] = dy
        else:
            dyf = dy.contiguous()

        def wgrad(dw):
            if ctx.stem:
                C.conv2d_stem_wgrad(x, dyc, dw, layer._stem_workspace(Cout, cin_g, ks, x.device))
                return
            ws, _ = layer._wgrad_workspace(cout_g, cin_g, ks, x.device)
            C.conv2d_wgrad_grouped(x, dyf, cin_g, cout_g, ks, dw, ws, G)

        def dgrad():
            # (the stem's dx: a transposed pack of the layer's own -- a stem layer is no member of a PackPool)
            pkT = layer._stem_packT(weight) if ctx.stem else layer._packed(weight, transposed_too=True)[1]
            dx = torch.empty_like(x)
            cfg = _dense_cfg(G, ks, Cout, Cin, N, H, W, x.device)
            if cfg is not None:
                C.conv2d(dyf, pkT[0], Cout, Cin, ks, out=dx, cfg=cfg)
            else:
                C.conv2d_grouped(dyf, pkT[0] if ctx.stem else layer._arenaT, cout_g, cin_g, ks, G, out=dx)
            if ctx.full_hw is not None:      # (strided 1x1: the input was sub-sampled first)
                st = layer.stride[0]
                if ctx.native_s2:      # the whole plane in one pass: values at even positions, zeros elsewhere
                    dx = C.subsample2_bwd(dx, torch.empty((N, Cin) + ctx.full_hw, dtype=dx.dtype, device=dx.device))
                else:
                    full = torch.zeros((N, Cin) + ctx.full_hw, dtype=dx.dtype, device=dx.device)
                    full[:, :, ::st, ::st] = dx
                    dx = full
            return dx

        return _HipConvFn._run_backward(ctx, dy, wgrad, dgrad)

    @staticmethod
    def _backward_strided(ctx, dy):
        """3x3 / 2 on cd_conv2d_dgrad_strided / cd_conv2d_wgrad_strided: no zero-stuffed dy."""
        x, weight = ctx.saved_tensors
        layer = ctx.layer
        Cout, cin_g, ks, _ = weight.shape
        G = layer.groups
        cout_g = Cout // G
        dyc = dy.contiguous()

        def wgrad(dw):
            ws, _ = layer._wgrad_workspace(cout_g, cin_g, ks, x.device)
            C.conv2d_wgrad_strided(x, dyc, cin_g, cout_g, ks, dw, ws, groups=G)

        def dgrad():
            layer._packed(weight, transposed_too=True)
            return C.conv2d_dgrad_strided(dyc, layer._arenaT, cin_g, cout_g, ks, torch.empty_like(x), groups=G)

        return _HipConvFn._run_backward(ctx, dyc, wgrad, dgrad)

    @staticmethod
    def _run_backward(ctx, dy, wgrad, dgrad):
        """The skeleton of both backward paths: `wgrad(dw)` fills dw, `dgrad()` returns dx, both enqueue on the current stream."""
        x, weight = ctx.saved_tensors
        dx = db = None
        dw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        # The weight gradient and the input gradient of a layer are independent: the weight gradient is enqueued on a side stream forked
        # here and joined before this function returns, so that its workgroups fill the compute units the input gradient's last round of
        # workgroups leaves idle (288 workgroups of the 24x24 planes on 256 CUs).  Round 6, two alternations on one box: 72.9 / 73.1 ->
        # 73.6 / 73.7 pairs/s on BASELINE configs[4] (CD_AMD_MIDAS_WGRAD_STREAM=0: one stream).  Same results either way.
        side = _wgrad_side_stream(x.device) if (ctx.needs_input_grad[0] and ctx.needs_input_grad[1]) else None
        if side is not None:
            fork = torch.cuda.Event()
            fork.record(torch.cuda.current_stream(x.device))
            side.wait_event(fork)
            with torch.cuda.stream(side):
                wgrad(dw)
        if ctx.needs_input_grad[0]:
            dx = dgrad()
        if side is not None:
            done = torch.cuda.Event()
            done.record(side)
            torch.cuda.current_stream(x.device).wait_event(done)
        elif ctx.needs_input_grad[1]:
            wgrad(dw)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            from .layers import channel_sum      # (hand-written reduction: cd_channel_sum)
            dyc = dy.contiguous()
            db = torch.empty(weight.shape[0], dtype=torch.float32, device=dyc.device)
            channel_sum(dyc, 0, weight.shape[0], db)
        return dx, dw, db, None


class HipConv2d(torch.nn.Conv2d):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        k, s, p = self.kernel_size, self.stride, self.padding
        if not (k[0] == k[1] and k[0] in C.KERNEL_SIZES and s[0] == s[1] and s[0] in (1, 2) and p[0] == p[1] == (k[0] - 1) // 2
                and self.dilation == (1, 1) and self.padding_mode == "zeros"):
            raise ValueError(f"HipConv2d: unsupported geometry kernel {k} stride {s} padding {p}")
        self._pk = self._pkT = self._table = self._tableT = self._wptr = self._ws = self._pool = self._stem_ws = None
        self._stem_pkT = self._stem_tableT = self._stem_wptr = None

    def _stem_now(self):
        """This call runs on the stem kernels (forward and weight gradient): the geometry, the switches and the arithmetic mode agree."""
        k, cin, cout = self.kernel_size[0], self.in_channels, self.out_channels
        return (self.stride[0] == 2 and self.groups == 1 and C.strided_enabled() and C.stem_enabled()
                and all(C.stem_supported(p, k, 2, cin, cout) for p in (0, 2)))

    def _uses_packed(self):
        """False for a layer on the stem kernels: they read the plain filter.  (Evaluated per call, not once: the arithmetic mode and
        the A/B switches may change between calls, and the stride-1 path they select needs the packs.)"""
        return not self._stem_now()

    def _stem_packT(self, weight):
        """The transposed pack behind the dx of a stem layer whose input asked for a gradient, packed here and now.  It is the layer's
        own, never a PackPool's: asking for dx changes nothing for the other layers of a network."""
        if self._stem_pkT is None or self._stem_wptr != weight.data_ptr():
            self._stem_pkT, self._stem_tableT, _ = self._build(weight, True)
            self._stem_wptr = weight.data_ptr()
        _native.check(_native.lib().cd_conv2d_pack_weights_table(self._stem_tableT.data_ptr(), self.groups, _native.stream_ptr(weight.device)),
                      "cd_conv2d_pack_weights_table")
        return self._stem_pkT

    def _stem_workspace(self, cout, cin, ks, device):
        if self._stem_ws is None:
            self._stem_ws = torch.empty(C.stem_wgrad_workspace_floats(cout, cin, ks), dtype=torch.float32, device=device)
        return self._stem_ws

    def _build(self, weight, transposed):
        """Packed buffers of every group (zeroed once: padding elements are never written) + the pack table."""
        lib = _native.lib()
        Cout, cin_g, ks, _ = weight.shape
        cout_g = Cout // self.groups
        oc, ic = (cin_g, cout_g) if transposed else (cout_g, cin_g)
        n = (lib.cd_conv2d_packed_weight_floats(oc, ic, ks, 0) + 63) // 64 * 64
        arena = torch.zeros(self.groups * n, dtype=torch.float32, device=weight.device)
        views = [arena[g * n:(g + 1) * n] for g in range(self.groups)]
        tab = np.zeros(self.groups, np.dtype(C.PackTable._DT))
        for g in range(self.groups):
            tab[g] = (weight.data_ptr() + 4 * g * cout_g * cin_g * ks * ks, views[g].data_ptr(), cout_g, cin_g, ks, int(transposed), oc, ic, 0, 0)
        if transposed:
            self._pack_strideT = n
        else:
            self._pack_stride = n
        return views, torch.from_numpy(tab.view(np.uint8).copy()).to(weight.device), arena

    def _packed(self, weight, transposed_too=False):
        if not (weight.is_cuda and weight.is_contiguous() and weight.dtype == torch.float32):
            raise RuntimeError("HipConv2d: weights must be contiguous fp32 on the HIP device (no CPU path)")
        if self._pool is not None:
            # packed by the pool's single launch at the start of this forward.  The pool is fresh from that launch until the
            # optimiser moves the weights (engine.FineTuneStep -> model.weights_updated() -> PackPool.invalidate()); a pooled layer
            # called outside the network's forward after an update (a sub-module, a feature extractor, a test) re-packs the pool.
            if not (self._pool.fresh and self._wptr == weight.data_ptr()):
                self._pool.run()
            return self._pk, self._pkT
        if self._wptr != weight.data_ptr():       # first use, or the optimiser re-homed the parameter
            self._pk, self._table, self._arena = self._build(weight, False)
            self._pkT = self._tableT = None
            self._wptr = weight.data_ptr()
        lib, stream = _native.lib(), _native.stream_ptr(weight.device)
        if transposed_too:
            if self._pkT is None:
                self._pkT, self._tableT, self._arenaT = self._build(weight, True)
            _native.check(lib.cd_conv2d_pack_weights_table(self._tableT.data_ptr(), self.groups, stream), "cd_conv2d_pack_weights_table")
        else:
            _native.check(lib.cd_conv2d_pack_weights_table(self._table.data_ptr(), self.groups, stream), "cd_conv2d_pack_weights_table")
        return self._pk, self._pkT

    def _wgrad_workspace(self, cout_g, cin_g, ks, device):
        """(buffer, floats per group): every group's per-workgroup partial sums side by side."""
        if self._ws is None:
            n = (_native.lib().cd_conv2d_wgrad_workspace_floats(cout_g, cin_g, ks) + 63) // 64 * 64
            self._ws = (torch.empty(self.groups * n, dtype=torch.float32, device=device), n)
        return self._ws

    def forward(self, x):
        return _HipConvFn.apply(x, self.weight, self.bias, self)
