"""Autograd faces of csrc/resample.hip -- the monodepth2 path's memory-bound pieces around the MFMA convolutions:

    bicubic_resize(x, size, norm=None)      F.interpolate(x, size, mode="bicubic", align_corners=False) [then (y - sub) / div]
                                            cd_bicubic_fwd / cd_bicubic_bwd (the adjoint as two gathers, no atomics)
    pad_cat(x, up, skip=None)               reflect_pad1(cat([nearest_x2(x) if up == 2 else x, skip], 1))    cd_pad_cat_fwd / _bwd
    crop_act(y_padded, act)                 act(y_padded[:, :, 1:-1, 1:-1]), act "elu" | "sigmoid"         cd_crop_act_fwd / _bwd
    HipReflectConv3x3(cin, cout)            ReflectionPad2d(1) + Conv2d(3x3, bias) as pad -> "same" HipConv2d -> crop: the decoder's
                                            `Conv3x3` (state-dict keys `conv.weight` / `conv.bias`)

The bicubic tables are computed on the host per (in, out) pair of an axis -- in the arithmetic of the tensor's dtype, as ATen does -- and
cached on the device; the first (eager) steps build them, so a captured step graph never uploads one.  fp32 NCHW on the HIP device, no CPU
path (the fp64 twins live in the tests).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from .blocks import _chk

_p = _native.dev_ptr
_A = -0.75          # ATen's cubic convolution constant

_TAP_DT = np.dtype([("i", "<i4", 4), ("w", "<f4", 4)])      # struct Tap4 of csrc/resample.hip
_INV_DT = np.dtype([("o", "<i4"), ("w", "<f4")])           # struct InvTap


def bicubic_taps(n_in: int, n_out: int, dtype=np.float32):
    """Per output index: the four source indices (clamped to [0, n_in - 1]) and weights of ATen's bicubic, align_corners=False, explicit
    size -- scale n_in / n_out, source coordinate scale * (dst + 0.5) - 0.5 (not clamped), all in `dtype` arithmetic.  -> (idx (n_out, 4)
    int64, w (n_out, 4) dtype)."""
    dt = np.dtype(dtype).type
    scale = dt(n_in) / dt(n_out)
    dst = np.arange(n_out, dtype=dt)
    src = scale * (dst + dt(0.5)) - dt(0.5)
    i0 = np.floor(src)
    t = src - i0
    A = dt(_A)

    def cc1(x):
        return ((A + dt(2)) * x - (A + dt(3))) * x * x + dt(1)

    def cc2(x):
        return ((A * x - dt(5) * A) * x + dt(8) * A) * x - dt(4) * A

    x2 = dt(1) - t
    w = np.stack([cc2(t + dt(1)), cc1(t), cc1(x2), cc2(x2 + dt(1))], 1).astype(dt)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, w


def bicubic_inverse(n_in: int, n_out: int, dtype=np.float32):
    """The adjoint's gather lists: for every input index i, the output indices o that read it (ascending) with the summed weight of all
    of o's taps that land on i (clamped taps coincide at the borders).  -> (off (n_in + 1,) int64, o (nnz,) int64, w (nnz,) dtype)."""
    idx, w = bicubic_taps(n_in, n_out, dtype)
    lists = [dict() for _ in range(n_in)]
    for o in range(n_out):
        for k in range(4):
            d = lists[idx[o, k]]
            d[o] = d[o] + w[o, k] if o in d else w[o, k]
    off = np.zeros(n_in + 1, np.int64)
    off[1:] = np.cumsum([len(d) for d in lists])
    oo = np.array([o for d in lists for o in sorted(d)], np.int64)
    ww = np.array([d[o] for d in lists for o in sorted(d)], dtype=dtype)
    return off, oo, ww


_TABLES: dict = {}


def _tables(n_in, n_out, device):
    """(forward table, inverse offsets, inverse entries) of one axis on `device`, built once."""
    key = (n_in, n_out, str(device))
    tab = _TABLES.get(key)
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"bicubic_resize: the tables of {n_in} -> {n_out} must be built before a graph capture (run one eager call)")
        idx, w = bicubic_taps(n_in, n_out, np.float32)
        fwd = np.zeros(n_out, _TAP_DT)
        fwd["i"], fwd["w"] = idx, w
        off, oo, ww = bicubic_inverse(n_in, n_out, np.float32)
        inv = np.zeros(len(oo), _INV_DT)
        inv["o"], inv["w"] = oo, ww
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(device)  # noqa: E731
        tab = _TABLES[key] = (up(fwd), torch.from_numpy(off.astype(np.int32)).to(device), up(inv))
    return tab


class _Bicubic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, norm):
        x = _chk(x, "bicubic_resize")
        N, C, Hin, Win = x.shape
        Hout, Wout = size
        ty, tx = _tables(Hin, Hout, x.device), _tables(Win, Wout, x.device)
        y = torch.empty(N, C, Hout, Wout, dtype=x.dtype, device=x.device)
        sub, div = norm if norm is not None else (0.0, 1.0)
        rc = _native.lib().cd_bicubic_fwd(_p(x), _p(y), N * C, Hin, Win, Hout, Wout, ty[0].data_ptr(), tx[0].data_ptr(),
                                          int(norm is not None), float(sub), float(div), _native.stream_ptr(x.device))
        _native.check(rc, "cd_bicubic_fwd")
        ctx.shape, ctx.tabs, ctx.div = (N, C, Hin, Win, Hout, Wout), (ty, tx), float(div)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, Hin, Win, Hout, Wout = ctx.shape
        ty, tx = ctx.tabs
        dy = _chk(dy, "bicubic_resize backward")
        if ctx.div != 1.0:
            dy = dy / ctx.div
        dx = torch.empty(N, C, Hin, Win, dtype=dy.dtype, device=dy.device)
        tmp = torch.empty(N * C * Hout * Win, dtype=dy.dtype, device=dy.device)
        rc = _native.lib().cd_bicubic_bwd(_p(dy), _p(dx), _p(tmp), N * C, Hin, Win, Hout, Wout, ty[1].data_ptr(), ty[2].data_ptr(),
                                          tx[1].data_ptr(), tx[2].data_ptr(), _native.stream_ptr(dy.device))
        _native.check(rc, "cd_bicubic_bwd")
        return dx, None, None


def bicubic_resize(x, size, norm=None):
    """F.interpolate(x, size=size, mode="bicubic", align_corners=False); with norm=(sub, div) the result is (y - sub) / div in the same
    pass (the monodepth2 encoder's input normalisation)."""
    return _Bicubic.apply(x, (int(size[0]), int(size[1])), None if norm is None else (float(norm[0]), float(norm[1])))


class _PadCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, up):
        x = _chk(x, "pad_cat")
        N, C1, h, w = x.shape
        H, W = h * up, w * up
        C2 = 0
        if skip is not None:
            skip = _chk(skip, "pad_cat")
            if skip.shape[0] != N or tuple(skip.shape[2:]) != (H, W):
                raise ValueError(f"pad_cat: skip {tuple(skip.shape)} does not match the up-sampled input {(N, C1, H, W)}")
            C2 = skip.shape[1]
        out = torch.empty(N, C1 + C2, H + 2, W + 2, dtype=x.dtype, device=x.device)
        rc = _native.lib().cd_pad_cat_fwd(_p(x), C1, up, _p(skip) if skip is not None else None, C2, _p(out), N, H, W,
                                          _native.stream_ptr(x.device))
        _native.check(rc, "cd_pad_cat_fwd")
        ctx.dims = (N, C1, C2, H, W, up)
        return out

    @staticmethod
    def backward(ctx, dout):
        N, C1, C2, H, W, up = ctx.dims
        dout = _chk(dout, "pad_cat backward")
        dx = torch.empty(N, C1, H // up, W // up, dtype=dout.dtype, device=dout.device)
        dskip = torch.empty(N, C2, H, W, dtype=dout.dtype, device=dout.device) if C2 else None
        rc = _native.lib().cd_pad_cat_bwd(_p(dout), _p(dx), C1, up, _p(dskip) if C2 else None, C2, N, H, W,
                                          _native.stream_ptr(dout.device))
        _native.check(rc, "cd_pad_cat_bwd")
        return dx, dskip, None


def pad_cat(x, up=1, skip=None):
    """ReflectionPad2d(1)(cat([x if up == 1 else nearest x2 of x, skip], 1)) -> (N, C1 + C2, H + 2, W + 2); H, W >= 2."""
    if up not in (1, 2):
        raise ValueError("pad_cat: up is 1 or 2")
    return _PadCat.apply(x, skip, up)


_ACTS = {"elu": 0, "sigmoid": 1}


class _CropAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xp, act):
        xp = _chk(xp, "crop_act")
        N, C, Hp, Wp = xp.shape
        y = torch.empty(N, C, Hp - 2, Wp - 2, dtype=xp.dtype, device=xp.device)
        rc = _native.lib().cd_crop_act_fwd(_p(xp), _p(y), act, N * C, Hp - 2, Wp - 2, _native.stream_ptr(xp.device))
        _native.check(rc, "cd_crop_act_fwd")
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _chk(dy, "crop_act backward")
        N, C, H, W = y.shape
        dxp = torch.empty(N, C, H + 2, W + 2, dtype=dy.dtype, device=dy.device)
        rc = _native.lib().cd_crop_act_bwd(_p(dy), _p(y), _p(dxp), ctx.act, N * C, H, W, _native.stream_ptr(dy.device))
        _native.check(rc, "cd_crop_act_bwd")
        return dxp, None


def crop_act(xp, act):
    """act(xp[:, :, 1:-1, 1:-1]) with act "elu" (alpha 1; the backward reads the output, like an in-place ELU) or "sigmoid"."""
    if xp.dim() != 4 or xp.shape[2] < 3 or xp.shape[3] < 3:
        raise ValueError("crop_act: (N, C, H + 2, W + 2) with H, W >= 1")
    return _CropAct.apply(xp, _ACTS[act])


class HipReflectConv3x3(torch.nn.Module):
    """ReflectionPad2d(1) + Conv2d(cin, cout, 3, bias=True) (monodepth2's `Conv3x3`, same key `conv.weight`) on the hand-written kernels:
    the padded input comes from `pad_cat` (fused with the up-sampling and the skip concat), the convolution is the tuned "same" HipConv2d
    over the padded tensor, and the caller crops its interior (`crop_act`, fused with the activation).  `forward(xp)` takes the padded
    input and returns the padded-size output."""

    def __init__(self, cin, cout):
        super().__init__()
        from .conv_layer import HipConv2d
        self.conv = HipConv2d(cin, cout, 3, 1, 1, bias=True)

    def forward(self, xp):
        return self.conv(xp)
