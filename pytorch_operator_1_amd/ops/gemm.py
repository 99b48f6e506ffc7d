"""The package's own bf16 MFMA GEMM (``csrc/kernels/gemm_bf16.hip``) and the
linear layer built on it.

Three products, each from the layouts a bias-free linear layer already
stores, so none needs a transposed copy of a weight or an activation:

* :func:`gemm_nt` ``C[M,N] = A[M,K] B[N,K]^T``: forward ``x W^T`` (and the
  input gradient from a ``W^T`` copy, where one is kept);
* :func:`gemm_nn` ``C[M,K] = A[M,N] B[N,K]``: input gradient ``dY W``;
* :func:`gemm_tn` ``C[N,K] = A[M,N]^T B[M,K]``: weight gradient ``dY^T X``.

On HIP tensors they launch the kernel and raise on a shape it refuses (no
fallback); on CPU tensors they compute the same product with torch, which is
what the CPU tests of the wiring run.

Who computes each GEMM of :func:`linear` is :func:`gemm_plan`'s answer, under
the ``PTO_GEMM`` switch (read at call time): ``1`` the kernel wherever it takes
the shape, ``0`` never, ``auto`` (default) the kernel for the entries of
:data:`GEMM_AUTO` -- the shapes where it measured faster than the library
GEMM plus the transposes that one needs (profiles/gemm_bf16.md).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib

NT, NN, TN = 0, 1, 2
_NAMES = {NT: "gemm_nt", NN: "gemm_nn", TN: "gemm_tn"}

# (kind, n_out, k_in) of a linear layer [n_out, k_in] whose GEMM of that kind
# ("fwd", "dgrad", "wgrad") goes to the kernel under PTO_GEMM=auto: only what
# beat the library in both runs of tools/gemm_bench.py (profiles/gemm_bf16.md).
# Nothing did.
GEMM_AUTO: frozenset = frozenset()

KINDS = ("fwd", "dgrad", "wgrad")


def kernel_takes(kind: str, rows: int, n_out: int, k_in: int) -> bool:
    """The kernel's shape rules for the GEMM ``kind`` of a linear layer
    ``[n_out, k_in]`` on ``rows`` tokens (contiguous operands): output columns
    and the contraction multiples of 64; the weight gradient's output rows
    (``n_out``) a multiple of 8."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    if rows < 1 or n_out < 1 or k_in < 1:
        return False
    if kind == "fwd":  # [rows, n_out], contraction k_in
        return n_out % 64 == 0 and k_in % 64 == 0
    if kind == "dgrad":  # [rows, k_in], contraction n_out
        return k_in % 64 == 0 and n_out % 64 == 0
    return k_in % 64 == 0 and rows % 64 == 0 and n_out % 8 == 0  # [n_out, k_in], contraction rows


def gemm_plan(kind: str, rows: int, n_out: int, k_in: int) -> str:
    """``"hip"`` (the package's kernel) or ``"lib"`` (hipBLASLt through
    torch) for the GEMM ``kind`` of a linear layer ``[n_out, k_in]`` applied
    to ``rows`` tokens."""
    mode = os.environ.get("PTO_GEMM", "auto")
    if mode not in ("auto", "0", "1"):
        raise ValueError(f"PTO_GEMM must be auto, 0 or 1, not {mode!r}")
    takes = kernel_takes(kind, rows, n_out, k_in)
    if takes and (mode == "1" or (mode == "auto" and (kind, n_out, k_in) in GEMM_AUTO)):
        return "hip"
    return "lib"


def _dims(form: int, a: torch.Tensor, b: torch.Tensor):
    """(M, N, K) in the naming of the module docstring, and the output shape."""
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f"{_NAMES[form]}: 2-D operands required")
    if form == NT:
        (M, K), (N, K2) = a.shape, b.shape
        ok, out = K == K2, (M, N)
    elif form == NN:
        (M, N), (N2, K) = a.shape, b.shape
        ok, out = N == N2, (M, K)
    else:
        (M, N), (M2, K) = a.shape, b.shape
        ok, out = M == M2, (N, K)
    if not ok:
        raise ValueError(f"{_NAMES[form]}: operand shapes {tuple(a.shape)} and {tuple(b.shape)} do not match")
    return M, N, K, out


def _cpu(form: int, a, b):
    if form == NT:
        return a.mm(b.t())
    if form == NN:
        return a.mm(b)
    return a.t().mm(b)


def _gemm(form: int, a: torch.Tensor, b: torch.Tensor, out=None, out_dtype=None):
    name = _NAMES[form]
    M, N, K, oshape = _dims(form, a, b)
    if out is not None:
        if tuple(out.shape) != oshape or out.device != a.device:
            raise ValueError(f"{name}: out must be {oshape} on {a.device}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"{name}: out_dtype {out_dtype} != out.dtype {out.dtype}")
        out_dtype = out.dtype
    if not a.is_cuda:
        r = _cpu(form, a, b)
        if out_dtype is not None:
            r = r.to(out_dtype)
        if out is None:
            return r
        out.copy_(r)
        return out
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or b.device != a.device:
        raise TypeError(f"{name}: bf16 operands on one HIP device required (got {a.dtype}, {b.dtype})")
    out_dtype = out_dtype or torch.bfloat16
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{name}: output must be bf16 or fp32, not {out_dtype}")
    if out is None:
        out = torch.empty(oshape, device=a.device, dtype=out_dtype)
    for t, what in ((a, "a"), (b, "b"), (out, "out")):
        if t.stride(1) != 1:
            raise RuntimeError(f"{name}: {what} must have unit inner stride (strides {t.stride()})")
    # the row stride of a one-row matrix is arbitrary and never used
    lda, ldb, ldc = (t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in (a, b, out))
    rc = _lib.lib().pto_gemm_bf16(form, a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(), ldc,
                                  int(out_dtype == torch.float32), M, N, K, _lib.stream_ptr(a.device))
    if rc == -1:
        raise RuntimeError(f"{name}: unsupported shape or layout: a {tuple(a.shape)} strides {a.stride()}, "
                           f"b {tuple(b.shape)} strides {b.stride()}, out strides {out.stride()} (contraction and "
                           "output columns multiples of 64, row strides multiples of 8, 16-byte aligned pointers)")
    _lib.check(rc, name)
    return out


def gemm_nt(a, b, out=None, out_dtype=None):
    """``a[M,K] @ b[N,K].T`` -> ``[M,N]`` (bf16 in, fp32 sums, bf16 or fp32 out)."""
    return _gemm(NT, a, b, out, out_dtype)


def gemm_nn(a, b, out=None, out_dtype=None):
    """``a[M,N] @ b[N,K]`` -> ``[M,K]``."""
    return _gemm(NN, a, b, out, out_dtype)


def gemm_tn(a, b, out=None, out_dtype=None):
    """``a[M,N].T @ b[M,K]`` -> ``[N,K]``."""
    return _gemm(TN, a, b, out, out_dtype)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` as a 2-D matrix with unit inner stride."""
    t2 = t.reshape(-1, t.shape[-1])
    return t2 if t2.stride(1) == 1 and (t2.shape[0] == 1 or t2.stride(0) % 8 == 0) else t2.contiguous()


def _on_kernel(kind: str, x2: torch.Tensor, n_out: int) -> bool:
    return x2.is_cuda and x2.dtype == torch.bfloat16 and gemm_plan(kind, x2.shape[0], n_out, x2.shape[1]) == "hip"


class _Linear(torch.autograd.Function):
    """``y = x W^T`` with each of its three GEMMs on the kernel or on the
    library as :func:`gemm_plan` says; on the library it is
    :class:`..ops.llm._LinearTW` (``wt`` given) or ``F.linear`` call for call."""

    @staticmethod
    def forward(ctx, x, w, wt, dw_kcontig, tstash=None):
        ctx.save_for_backward(x, w, wt)
        ctx.dw_kcontig, ctx.tstash = dw_kcontig, tstash
        x2 = _rows(x) if x.is_cuda else x
        if _on_kernel("fwd", x2, w.shape[0]) and w.dtype == x.dtype:
            # the returned tensor is the allocation itself, not a view of it: a
            # consumer may modify it in place (RoPE on the QKV projection)
            y = torch.empty(*x.shape[:-1], w.shape[0], device=x.device, dtype=x.dtype)
            gemm_nt(x2, w, out=y.view(-1, w.shape[0]))
            return y
        return F.linear(x, w)

    @staticmethod
    def backward(ctx, dy):
        from . import llm

        x, w, wt = ctx.saved_tensors
        n_out, k_in = w.shape
        x2 = x.reshape(-1, k_in)
        dy2 = dy.reshape(-1, n_out)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if _on_kernel("dgrad", x2, n_out) and dy.dtype == w.dtype:
                d2 = _rows(dy2)
                dx = (gemm_nt(d2, wt) if wt is not None else gemm_nn(d2, w)).view(x.shape)
            elif wt is not None:
                dx = F.linear(dy, wt)
            else:
                dx = dy2.mm(w).view(x.shape)
        if ctx.needs_input_grad[1]:
            if _on_kernel("wgrad", x2, n_out) and dy.dtype == x.dtype:
                if ctx.tstash is not None:
                    ctx.tstash.take()  # a transpose the kernel has no use for
                dw = gemm_tn(_rows(dy2), _rows(x2))
            elif ctx.dw_kcontig and x2.is_cuda:
                # as _LinearTW: both operands token-contiguous for the library
                xt = llm.transpose_into(x2.contiguous(), torch.empty(x2.shape[1], x2.shape[0], device=x2.device,
                                                                      dtype=x2.dtype))
                dyt = ctx.tstash.take() if ctx.tstash is not None else None
                if dyt is None or dyt.shape != (dy2.shape[1], dy2.shape[0]):
                    dyt = llm.transpose_into(dy2.contiguous(), torch.empty(dy2.shape[1], dy2.shape[0],
                                                                            device=dy2.device, dtype=dy2.dtype))
                dw = dyt.mm(xt.t())
            else:
                dw = dy2.t().mm(x2)
        return dx, dw, None, None, None


def linear(x, w, wt=None, dw_kcontig: bool = False, tstash=None):
    """Bias-free ``F.linear(x, w)`` with :func:`..ops.llm.linear_tw`'s
    contract: ``wt`` (== ``w.t()``, kept current by the caller) serves the
    input gradient when given, ``dw_kcontig`` asks the library's weight
    gradient to run from transposed activations, ``tstash`` may hold the
    output gradient's transpose.  Each GEMM follows :func:`gemm_plan`; a
    weight gradient on the kernel uses ``dy`` and ``x`` as stored and drops a
    stashed transpose.  A layer with no GEMM on the kernel IS ``F.linear`` /
    ``linear_tw``: the same library calls in the same order."""
    if x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16:
        rows = x.numel() // x.shape[-1]
        if any(gemm_plan(kind, rows, w.shape[0], w.shape[1]) == "hip" for kind in KINDS):
            return _Linear.apply(x, w, wt, dw_kcontig, tstash)
    elif not x.is_cuda:
        return _Linear.apply(x, w, wt, dw_kcontig, tstash)  # CPU: the wiring, on torch products
    if wt is None:
        return F.linear(x, w)
    from . import llm

    return llm.linear_tw(x, w, wt, dw_kcontig, tstash)
