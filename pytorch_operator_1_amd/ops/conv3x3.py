"""ResNet-50's 3x3 convolutions on the package's MFMA implicit-GEMM kernel
(``csrc/kernels/conv3x3.hip``), channels-last bf16, pad 1, stride 1 or 2.

Forward: ``k_conv3x3_fwd`` -- and, when the consumer is a fused BatchNorm
(``ops/bn.py``), the per-channel sums / sums of squares of the rounded
outputs come out of the conv epilogue (:class:`ConvStats`), so the BN
forward skips its statistics pass (a full read of the conv output).
Backward (:func:`conv3x3_backward_plan`): the input gradient of a stride-1
conv is the SAME kernel run on dY with the filter flipped and transposed
(``k_conv3x3_wflip``) where that swapped launch meets the forward tile
rules; the weight gradient is the package's split-reduction MFMA kernel
(``csrc/kernels/conv3x3_wgrad.hip``, :func:`conv3x3_wgrad`: fp32, any C and
K that are multiples of 64, bitwise repeatable) for the shapes
``PTO_CONV3X3_WGRAD`` selects.  What is left -- the stride-2 input gradient,
a C != K input gradient the tiles do not take, weight gradients not selected
-- is MIOpen's (``aten.convolution_backward``).  CPU / unsupported shapes:
the stock conv.

Reference parity: the reference's workload is the MNIST ``Net``
(``examples/mnist/mnist.py:17-33``); ResNet-50 is BASELINE.json config 3,
whose convolutions SURVEY §2.9 K3 asks to own as an implicit GEMM with a
fused epilogue.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

_CL = torch.channels_last


class ConvStats:
    """Holder for the BN statistics partials a conv epilogue produced:
    ``part`` ([tiles][2][C] fp32: per-tile channel sums, sums of squares)
    and ``nblk`` (tiles).  Filled by :func:`conv3x3` in the forward, read
    (and cleared) by ``BatchNormAct``."""

    __slots__ = ("part", "nblk")

    def __init__(self):
        self.part, self.nblk = None, 0

    def take(self):
        p, n = self.part, self.nblk
        self.part, self.nblk = None, 0
        return p, n


def _compute_dtype(x):
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else x.dtype


def conv3x3_supported(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """Shapes and dtypes the kernel takes: bf16 compute (autocast or a bf16
    input), 3x3 / pad 1 / stride 1 or 2, channels multiples of the tiles,
    fp32 channels-last filter."""
    if not (x.is_cuda and x.dim() == 4 and _compute_dtype(x) == torch.bfloat16 and conv.kernel_size == (3, 3)
            and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.stride in ((1, 1), (2, 2)) and os.environ.get("PTO_CONV3X3", "1") == "1"):
        return False
    if conv.in_channels % 64 or not _fwd_tiles_ok(conv.out_channels):
        return False
    w = conv.weight
    return w.dtype == torch.float32 and w.is_contiguous(memory_format=_CL)


def _fwd_tiles_ok(K: int) -> bool:
    """The forward kernel's tile rules on its output channels: 64, or a
    multiple of 128 up to 256, or a multiple of 256 above."""
    return K >= 64 and not (K % 64 or (K > 64 and K % 128) or (K > 256 and K % 256))


# (C, K, stride) whose weight gradient goes to the kernel under
# PTO_CONV3X3_WGRAD=auto: the shapes where it was not slower than MIOpen's in
# two separate runs at batch 256 (profiles/conv3x3_wgrad.md).
WGRAD_AUTO = frozenset({(128, 128, 1), (256, 256, 2), (256, 256, 1), (512, 512, 1)})


def conv3x3_backward_plan(C: int, K: int, stride: int) -> dict:
    """Who computes each gradient of a supported conv: ``"kernel"`` or
    ``"library"`` (MIOpen).  dx: the forward kernel on dY with C and K
    swapped, so stride 1 only and C must meet the forward's rules on output
    channels (and K, now the reduction, be a multiple of 64).  dw: the
    ``PTO_CONV3X3_WGRAD`` switch, read at call time -- ``1`` the kernel for
    every shape it takes, ``0`` the library, ``auto`` (default) the kernel
    for the entries of :data:`WGRAD_AUTO`."""
    dx = "kernel" if stride == 1 and K % 64 == 0 and _fwd_tiles_ok(C) else "library"
    mode = os.environ.get("PTO_CONV3X3_WGRAD", "auto")
    if mode not in ("auto", "0", "1"):
        raise ValueError(f"PTO_CONV3X3_WGRAD must be auto, 0 or 1, not {mode!r}")
    takes = C >= 64 and K >= 64 and C % 64 == 0 and K % 64 == 0 and stride in (1, 2)
    dw = "kernel" if takes and (mode == "1" or (mode == "auto" and (C, K, stride) in WGRAD_AUTO)) else "library"
    return {"dx": dx, "dw": dw}


def _out_hw(h: int, s: int) -> int:
    return (h + 2 - 3) // s + 1


def _fwd(L, x, wb, stride, part=None):
    N, C, H, W = x.shape
    K = wb.shape[0]
    OH, OW = _out_hw(H, stride), _out_hw(W, stride)
    y = torch.empty(N, K, OH, OW, device=x.device, dtype=torch.bfloat16, memory_format=_CL)
    _lib.check(L.pto_conv3x3_fwd(x.data_ptr(), wb.data_ptr(), y.data_ptr(), None if part is None else part.data_ptr(),
                                 N, H, W, C, K, stride, _lib.stream_ptr(x.device)), "conv3x3_fwd")
    return y


def stats_tiles(N: int, OH: int, OW: int, K: int) -> int:
    tm = _lib.lib().pto_conv3x3_tile_m(K)
    return (N * OH * OW + tm - 1) // tm


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, stride: int, workspace: torch.Tensor | None = None):
    """Weight gradient of a 3x3 / pad-1 conv: ``x`` [N,C,H,W] and ``dy``
    [N,K,OH,OW], bf16 channels-last, to fp32 (K,C,3,3) channels-last, sums
    in fp32 and nothing rounded to bf16.  ``workspace``: fp32 scratch of at
    least ``splits * K * 9 * C`` elements (any content; allocated if not
    given).  Raises on a shape the kernel does not take."""
    N, C, H, W = x.shape
    K = dy.shape[1]
    if not (x.is_cuda and x.dtype == dy.dtype == torch.bfloat16 and x.is_contiguous(memory_format=_CL)
            and dy.is_contiguous(memory_format=_CL) and dy.device == x.device
            and dy.shape == (N, K, _out_hw(H, stride), _out_hw(W, stride))):
        raise ValueError("conv3x3_wgrad: x, dy must be bf16 channels-last CUDA tensors of matching conv shapes")
    L = _lib.lib()
    splits = L.pto_conv3x3_wgrad_splits(N, H, W, C, K, stride)
    if splits < 1:
        raise RuntimeError(f"conv3x3_wgrad: unsupported shape N={N} H={H} W={W} C={C} K={K} stride={stride}")
    need = splits * K * 9 * C
    if workspace is None:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    elif not (workspace.dtype == torch.float32 and workspace.device == x.device and workspace.is_contiguous()
              and workspace.numel() >= need):
        raise ValueError(f"conv3x3_wgrad: workspace must be contiguous fp32 with at least {need} elements")
    dw = torch.empty(K, C, 3, 3, device=x.device, dtype=torch.float32, memory_format=_CL)
    _lib.check(L.pto_conv3x3_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), workspace.data_ptr(), N, H, W, C, K,
                                   stride, _lib.stream_ptr(x.device)), "conv3x3_wgrad")
    return dw


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, wb, stride, stats):
        L = _lib.lib()
        x = x.to(torch.bfloat16).contiguous(memory_format=_CL)
        # the bf16 image of the fp32 master filter (same channels-last layout),
        # rebuilt every call into the module's persistent buffer
        _lib.check(L.pto_conv3x3_wcast(weight.data_ptr(), wb.data_ptr(), wb.numel(), _lib.stream_ptr(x.device)),
                   "conv3x3_wcast")
        part = None
        if stats is not None:
            N, _, H, W = x.shape
            K = weight.shape[0]
            nblk = stats_tiles(N, _out_hw(H, stride), _out_hw(W, stride), K)
            part = torch.empty(nblk * 2 * K, device=x.device, dtype=torch.float32)
            stats.part, stats.nblk = part, nblk
        y = _fwd(L, x, wb, stride, part)
        ctx.save_for_backward(x, wb)
        ctx.stride = stride
        ctx.wshape, ctx.wstride, ctx.wdtype = weight.shape, weight.stride(), weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        s = ctx.stride
        dy = dy.to(torch.bfloat16).contiguous(memory_format=_CL)
        K, C = wb.shape[0], wb.shape[1]
        plan = conv3x3_backward_plan(C, K, s)
        dx = dw = None
        if ctx.needs_input_grad[0] and plan["dx"] == "kernel":
            L = _lib.lib()
            wf = torch.empty(C, K, 3, 3, device=x.device, dtype=torch.bfloat16, memory_format=_CL)
            _lib.check(L.pto_conv3x3_wflip(None, wb.data_ptr(), wf.data_ptr(), K, C, _lib.stream_ptr(x.device)),
                       "conv3x3_wflip")
            dx = _fwd(L, dy, wf, 1)
        if ctx.needs_input_grad[1] and plan["dw"] == "kernel":
            dw = conv3x3_wgrad(x, dy, s)  # fp32, the master filter's layout
        need_dx_lib = ctx.needs_input_grad[0] and dx is None
        need_dw_lib = ctx.needs_input_grad[1] and dw is None
        if need_dx_lib or need_dw_lib:
            dxl, dwl, _ = torch.ops.aten.convolution_backward(dy, x, wb, None, [s, s], [1, 1], [1, 1], False, [0, 0], 1,
                                                              [need_dx_lib, need_dw_lib, False])
            if need_dx_lib:
                dx = dxl
            if need_dw_lib:
                dw = dwl.to(ctx.wdtype)
        if dw is not None and dw.stride() != ctx.wstride:
            dw = torch.empty_strided(ctx.wshape, ctx.wstride, dtype=dw.dtype, device=dw.device).copy_(dw)
        return dx, dw, None, None, None


def conv3x3(x: torch.Tensor, conv: nn.Conv2d, stats: ConvStats | None = None) -> torch.Tensor:
    """``conv(x)`` for a 3x3 / pad-1 / bias-free conv: the HIP kernel on
    supported shapes (bf16 channels-last output, as under autocast; with
    ``stats`` the BN partials of the output too), the stock module otherwise
    (``stats`` then stays empty and the BN computes its own)."""
    if not conv3x3_supported(x, conv):
        return conv(x)
    wb = getattr(conv, "_pto_c3_wb", None)
    if wb is None or wb.device != x.device or wb.shape != conv.weight.shape:
        wb = torch.empty(conv.weight.shape, device=x.device, dtype=torch.bfloat16, memory_format=_CL)
        conv._pto_c3_wb = wb
    with torch.autocast("cuda", enabled=False):
        return _Conv3x3.apply(x, conv.weight, wb, conv.stride[0], stats)


def reference_conv3x3(x: torch.Tensor, w: torch.Tensor, stride: int) -> torch.Tensor:
    """fp32 reference of the kernel's math: bf16 operands, fp32 sums."""
    return F.conv2d(x.float(), w.to(torch.bfloat16).float(), stride=stride, padding=1)
