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


# ---------------------------------------------------------------- skinny GEMM (decode)
# csrc/kernels/gemm_skinny.hip: y[M,N] = x[M,K] W[N,K]^T for 1 <= M <= 16, the
# linear layers of a decode step, optionally with the SwiGLU of a fused
# gate|up weight in the epilogue.

# (n_out, k_in) of the linear layers whose decode-time product goes to the
# skinny kernel under PTO_SKINNY=auto.  Empty: generation's default bits stay
# what the library gives; profiles/decode_linear.md lists the candidates.
SKINNY_AUTO: frozenset = frozenset()

SKINNY_MAX_ROWS = 16
_skinny_ws: dict = {}  # device -> uint8 workspace for the split-K partials


def skinny_takes(rows: int, n_out: int, k_in: int, swiglu: bool = False) -> bool:
    """The skinny kernel's shape rules for a linear layer ``[n_out, k_in]`` on
    ``rows`` tokens (contiguous operands): 1..16 rows, output rows of the
    weight a multiple of 16 (of 32 with ``swiglu``: ``F = n_out / 2`` a
    multiple of 16), contraction a multiple of 32."""
    if not 1 <= rows <= SKINNY_MAX_ROWS or n_out < 1 or k_in < 1:
        return False
    return n_out % (32 if swiglu else 16) == 0 and k_in % 32 == 0


def skinny_plan(rows: int, n_out: int, k_in: int) -> str:
    """``"hip"`` (the skinny kernel) or ``"lib"`` (hipBLASLt through torch)
    for the decode-time product of a linear layer ``[n_out, k_in]`` with
    ``rows`` tokens, under the ``PTO_SKINNY`` switch (read at call time)."""
    mode = os.environ.get("PTO_SKINNY", "auto")
    if mode not in ("auto", "0", "1"):
        raise ValueError(f"PTO_SKINNY must be auto, 0 or 1, not {mode!r}")
    takes = skinny_takes(rows, n_out, k_in)
    if takes and (mode == "1" or (mode == "auto" and (n_out, k_in) in SKINNY_AUTO)):
        return "hip"
    return "lib"


def skinny_splits(n_out: int, k_in: int) -> int:
    """The kernel's default K split across workgroups: a function of the
    layer shape alone, never of the row count."""
    return int(_lib.lib().pto_gemm_skinny_splits(n_out, k_in))


def _skinny_workspace(device, nbytes: int) -> torch.Tensor:
    ws = _skinny_ws.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _skinny_ws[device] = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
    return ws


def skinny_nt(x, w, out=None, out_dtype=None, swiglu: bool = False, n_splits: int | None = None):
    """``x[M,K] @ w[N,K].T`` for ``1 <= M <= 16`` (bf16 in, fp32 sums, bf16
    or fp32 out).  ``swiglu``: ``w`` is a fused gate|up weight ``[2F, K]`` and
    the result is ``silu(g) * u`` as bf16 ``[M, F]``, bitwise
    :func:`..ops.llm.swiglu` of the plain bf16 result with the same
    ``n_splits`` (default :func:`skinny_splits`).  Row ``m`` of the result
    depends on ``x[m]``, ``w`` and ``n_splits`` only.  HIP tensors launch the
    kernel and raise on a refused shape; CPU tensors compute the same with
    torch."""
    M, N, K, _ = _dims(NT, x, w)
    if swiglu and N % 2:
        raise ValueError(f"skinny_nt: swiglu needs an even number of weight rows, got {N}")
    oshape = (M, N // 2) if swiglu else (M, N)
    if out is not None:
        if tuple(out.shape) != oshape or out.device != x.device:
            raise ValueError(f"skinny_nt: out must be {oshape} on {x.device}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"skinny_nt: out_dtype {out_dtype} != out.dtype {out.dtype}")
        out_dtype = out.dtype
    if not x.is_cuda:
        r = x.mm(w.t())
        if swiglu:
            g, u = r.float().chunk(2, dim=-1)
            r = (g * torch.sigmoid(g)).to(x.dtype).float() * u
        r = r.to(out_dtype or x.dtype)
        if out is None:
            return r
        out.copy_(r)
        return out
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or w.device != x.device:
        raise TypeError(f"skinny_nt: bf16 operands on one HIP device required (got {x.dtype}, {w.dtype})")
    out_dtype = out_dtype or torch.bfloat16
    if out_dtype not in (torch.bfloat16, torch.float32) or (swiglu and out_dtype != torch.bfloat16):
        raise TypeError(f"skinny_nt: output must be bf16{'' if swiglu else ' or fp32'}, not {out_dtype}")
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=out_dtype)
    for t, what in ((x, "x"), (w, "w"), (out, "out")):
        if t.stride(1) != 1:
            raise RuntimeError(f"skinny_nt: {what} must have unit inner stride (strides {t.stride()})")
    lda, ldb, ldc = (t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in (x, w, out))
    L = _lib.lib()
    ns = int(L.pto_gemm_skinny_splits(N, K)) if n_splits is None else int(n_splits)
    nbytes = L.pto_gemm_skinny_workspace(M, N, ns) if ns > 1 else 0
    ws = _skinny_workspace(x.device, nbytes) if nbytes > 0 else None
    rc = L.pto_gemm_skinny(x.data_ptr(), lda, w.data_ptr(), ldb, out.data_ptr(), ldc, int(out_dtype == torch.float32),
                           int(bool(swiglu)), M, N, K, ns, _lib.ptr(ws), nbytes if ws is not None else 0,
                           _lib.stream_ptr(x.device))
    if rc == -1:
        raise RuntimeError(f"skinny_nt: unsupported shape or layout: x {tuple(x.shape)} strides {x.stride()}, "
                           f"w {tuple(w.shape)} strides {w.stride()}, out strides {out.stride()}, n_splits {ns} "
                           "(1..16 rows, weight rows a multiple of 16 (32 with swiglu), contraction a multiple of "
                           "32, row strides multiples of 8, 16-byte aligned pointers, 1..64 splits)")
    _lib.check(rc, "skinny_nt")
    return out


# ---------------------------------------------------------------- MX weight-only skinny GEMM (decode)
# csrc/kernels/gemm_skinny_mx.hip: the skinny product against a weight held in
# an OCP microscaling format -- blocks of 32 consecutive K elements of a row
# share one E8M0 scale byte e (2^(e-127)); elements are e2m1 ("mxfp4", two per
# byte, element 2i in the low nibble of byte i) or e4m3fn ("mxfp8").

MX_FORMATS = {"mxfp4": 0, "mxfp8": 1}
MX_BLOCK = 32
_MX_EMAX = {"mxfp4": 2, "mxfp8": 8}  # exponent of the largest element: 6 = 1.5 * 2^2, 448 = 1.75 * 2^8
_FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# midpoints between neighbouring e2m1 magnitudes and whether a tie goes up (to the even code)
_FP4_MIDPOINTS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


class MXWeight:
    """A weight ``[N, K]`` in an MX format: ``data`` uint8 ``[N, K/2]``
    (``"mxfp4"``) or ``[N, K]`` (``"mxfp8"``), ``scales`` uint8 ``[N, K/32]``,
    both contiguous."""

    def __init__(self, data: torch.Tensor, scales: torch.Tensor, fmt: str, shape):
        if fmt not in MX_FORMATS:
            raise ValueError(f"fmt must be one of {tuple(MX_FORMATS)}, not {fmt!r}")
        N, K = (int(s) for s in shape)
        want = (N, K // 2 if fmt == "mxfp4" else K)
        if K % MX_BLOCK or tuple(data.shape) != want or tuple(scales.shape) != (N, K // MX_BLOCK):
            raise ValueError(f"MXWeight: data {tuple(data.shape)} / scales {tuple(scales.shape)} do not hold a {fmt} "
                             f"weight of shape {(N, K)}")
        if data.dtype != torch.uint8 or scales.dtype != torch.uint8 or data.device != scales.device:
            raise TypeError("MXWeight: data and scales must be uint8 tensors on one device")
        self.data, self.scales, self.fmt, self.shape = data.contiguous(), scales.contiguous(), fmt, (N, K)

    @property
    def device(self):
        return self.data.device

    def to(self, device):
        return MXWeight(self.data.to(device), self.scales.to(device), self.fmt, self.shape)


def _quantize_mx_torch(w: torch.Tensor, fmt: str):
    N, K = w.shape
    v = w.detach().float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = v.abs().amax(-1)
    # floor(log2(amax)) + 127 is the exponent field of amax (a subnormal clamps to e = 1 either way)
    e = (((amax.view(torch.int32) >> 23) & 0xff) - _MX_EMAX[fmt]).clamp(1, 254)
    e = torch.where(amax == 0, torch.full_like(e, 127), e)
    v = v * ((254 - e) << 23).view(torch.float32)[..., None]  # times 2^(127 - e), exact
    sign = torch.signbit(v)
    if fmt == "mxfp4":
        a = v.abs()
        code = torch.zeros_like(a, dtype=torch.uint8)
        for mid, tie_up in _FP4_MIDPOINTS:
            code += (a >= mid) if tie_up else (a > mid)
        nib = (code | (sign.to(torch.uint8) << 3)).reshape(N, K // 2, 2)
        data = nib[..., 0] | (nib[..., 1] << 4)
    else:
        q = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        data = ((q & 0x7f) | (sign.to(torch.uint8) << 7)).reshape(N, K)
    return data.contiguous(), e.to(torch.uint8).contiguous()


def quantize_mx(w: torch.Tensor, fmt: str = "mxfp4") -> MXWeight:
    """Quantise a weight ``[N, K]`` (``K % 32 == 0``, finite values) by the
    OCP MX v1.0 rule: per block of 32 along K, ``e = clamp(floor(log2(amax)) -
    emax + 127, 1, 254)`` (127 for an all-zero block), each element ``w /
    2^(e-127)`` rounded to nearest, ties to even on the element grid,
    saturating at the largest element.  bf16 HIP tensors run the kernel
    (``k_quant_mx``); everything else the same rule in torch."""
    if fmt not in MX_FORMATS:
        raise ValueError(f"fmt must be one of {tuple(MX_FORMATS)}, not {fmt!r}")
    if w.dim() != 2 or w.shape[1] % MX_BLOCK or not w.is_floating_point():
        raise ValueError(f"quantize_mx: a floating-point [N, K] weight with K % {MX_BLOCK} == 0 required, got "
                         f"{w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if not (w.is_cuda and w.dtype == torch.bfloat16):
        return MXWeight(*_quantize_mx_torch(w, fmt), fmt, (N, K))
    w = _rows(w.detach())
    data = torch.empty(N, K // 2 if fmt == "mxfp4" else K, device=w.device, dtype=torch.uint8)
    scales = torch.empty(N, K // MX_BLOCK, device=w.device, dtype=torch.uint8)
    rc = _lib.lib().pto_quant_mx(w.data_ptr(), w.stride(0) if N > 1 else K, data.data_ptr(), scales.data_ptr(),
                                 MX_FORMATS[fmt], N, K, _lib.stream_ptr(w.device))
    if rc == -1:
        raise RuntimeError(f"quantize_mx: unsupported shape or layout: w {tuple(w.shape)} strides {w.stride()} "
                           "(row stride a multiple of 8, 16-byte aligned pointer)")
    _lib.check(rc, "quantize_mx")
    return MXWeight(data, scales, fmt, (N, K))


def dequantize_mx(q: MXWeight, dtype=torch.bfloat16) -> torch.Tensor:
    """The ``[N, K]`` weight ``q`` stands for; exact in bf16 and wider."""
    N, K = q.shape
    scale = (q.scales.to(torch.int32) << 23).view(torch.float32)  # 2^(e - 127)
    if q.fmt == "mxfp4":
        nib = torch.stack((q.data & 0xf, q.data >> 4), dim=-1).reshape(N, K).long()
        lut = torch.tensor(_FP4_VALUES + tuple(-v for v in _FP4_VALUES), device=q.device)
        v = lut[nib]
    else:
        v = q.data.view(torch.float8_e4m3fn).float()
    return (v.reshape(N, K // MX_BLOCK, MX_BLOCK) * scale[..., None]).reshape(N, K).to(dtype)


def skinny_mx_takes(rows: int, n_out: int, k_in: int, swiglu: bool = False) -> bool:
    """The MX skinny kernel's shape rules: 1..16 rows, weight rows a multiple
    of 16 (of 32 with ``swiglu``), contraction a multiple of 128."""
    if not 1 <= rows <= SKINNY_MAX_ROWS or n_out < 1 or k_in < 1:
        return False
    return n_out % (32 if swiglu else 16) == 0 and k_in % 128 == 0


def skinny_mx_splits(n_out: int, k_in: int, fmt: str = "mxfp4") -> int:
    """The MX kernel's default K split across workgroups: a function of the
    layer shape and the format, never of the row count."""
    return int(_lib.lib().pto_gemm_skinny_mx_splits(n_out, k_in, MX_FORMATS[fmt]))


def skinny_mx_nt(x, q: MXWeight, out=None, out_dtype=None, swiglu: bool = False, n_splits: int | None = None):
    """:func:`skinny_nt` against a quantised weight: ``x[M,K] @
    dequantize_mx(q).T`` for ``1 <= M <= 16`` (bf16 ``x``, fp32 sums, bf16 or
    fp32 out), the weight read in its packed form.  ``swiglu`` as in
    :func:`skinny_nt`, bitwise :func:`..ops.llm.swiglu` of the plain bf16
    result with the same ``n_splits`` (default :func:`skinny_mx_splits`).  Row
    ``m`` of the result depends on ``x[m]``, ``q`` and ``n_splits`` only.  HIP
    tensors launch the kernel and raise on a refused shape; CPU tensors
    compute ``skinny_nt(x, dequantize_mx(q))``."""
    if not isinstance(q, MXWeight):
        raise TypeError(f"skinny_mx_nt: q must be an MXWeight, not {type(q).__name__}")
    if x.dim() != 2 or x.shape[1] != q.shape[1]:
        raise ValueError(f"skinny_mx_nt: operand shapes {tuple(x.shape)} and {q.shape} do not match")
    (M, K), N = x.shape, q.shape[0]
    if swiglu and N % 2:
        raise ValueError(f"skinny_mx_nt: swiglu needs an even number of weight rows, got {N}")
    oshape = (M, N // 2) if swiglu else (M, N)
    if out is not None:
        if tuple(out.shape) != oshape or out.device != x.device:
            raise ValueError(f"skinny_mx_nt: out must be {oshape} on {x.device}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"skinny_mx_nt: out_dtype {out_dtype} != out.dtype {out.dtype}")
        out_dtype = out.dtype
    if not x.is_cuda:
        return skinny_nt(x, dequantize_mx(q, x.dtype), out=out, out_dtype=out_dtype, swiglu=swiglu)
    if x.dtype != torch.bfloat16 or q.device != x.device:
        raise TypeError(f"skinny_mx_nt: bf16 x and the weight on one HIP device required (got {x.dtype} on "
                        f"{x.device}, weight on {q.device})")
    out_dtype = out_dtype or torch.bfloat16
    if out_dtype not in (torch.bfloat16, torch.float32) or (swiglu and out_dtype != torch.bfloat16):
        raise TypeError(f"skinny_mx_nt: output must be bf16{'' if swiglu else ' or fp32'}, not {out_dtype}")
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=out_dtype)
    for t, what in ((x, "x"), (out, "out")):
        if t.stride(1) != 1:
            raise RuntimeError(f"skinny_mx_nt: {what} must have unit inner stride (strides {t.stride()})")
    lda, ldc = (t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in (x, out))
    L = _lib.lib()
    fmt = MX_FORMATS[q.fmt]
    ns = int(L.pto_gemm_skinny_mx_splits(N, K, fmt)) if n_splits is None else int(n_splits)
    nbytes = L.pto_gemm_skinny_mx_workspace(M, N, ns) if ns > 1 else 0
    ws = _skinny_workspace(x.device, nbytes) if nbytes > 0 else None
    rc = L.pto_gemm_skinny_mx(x.data_ptr(), lda, q.data.data_ptr(), q.scales.data_ptr(), out.data_ptr(), ldc,
                              int(out_dtype == torch.float32), int(bool(swiglu)), fmt, M, N, K, ns, _lib.ptr(ws),
                              nbytes if ws is not None else 0, _lib.stream_ptr(x.device))
    if rc == -1:
        raise RuntimeError(f"skinny_mx_nt: unsupported shape or layout: x {tuple(x.shape)} strides {x.stride()}, "
                           f"{q.fmt} weight {q.shape}, out strides {out.stride()}, n_splits {ns} (1..16 rows, weight "
                           "rows a multiple of 16 (32 with swiglu), contraction a multiple of 128, row strides "
                           "multiples of 8, 16-byte aligned pointers, 1..64 splits)")
    _lib.check(rc, "skinny_mx_nt")
    return out


# ---------------------------------------------------------------- MX weight-only GEMM for any row count
# csrc/kernels/gemm_mx.hip: the product against a packed MX weight with no
# limit on the rows, so that a model can run from its packed weights alone.


def mx_takes(rows: int, n_out: int, k_in: int, swiglu: bool = False) -> bool:
    """The MX GEMM's shape rules: any ``rows >= 1``, weight rows a multiple
    of 32 (of 64 with ``swiglu``), contraction a multiple of 128."""
    if rows < 1 or n_out < 1 or k_in < 1:
        return False
    return n_out % (64 if swiglu else 32) == 0 and k_in % 128 == 0


def mx_splits(rows: int, n_out: int, k_in: int, fmt: str = "mxfp4") -> int:
    """The MX GEMM's default K split across workgroups, a function of the
    shape: small row counts with few weight rows split K to fill the device."""
    return int(_lib.lib().pto_gemm_mx_splits(rows, n_out, k_in, MX_FORMATS[fmt]))


def mx_nt(x, q: MXWeight, out=None, out_dtype=None, swiglu: bool = False, n_splits: int | None = None):
    """:func:`skinny_mx_nt` with no limit on the rows: ``x[M,K] @
    dequantize_mx(q).T`` for any ``M >= 1`` (bf16 ``x``, fp32 sums, bf16 or
    fp32 out), the weight read in its packed form.  ``swiglu``: bitwise
    :func:`..ops.llm.swiglu` of the plain bf16 result with the same
    ``n_splits`` (default :func:`mx_splits`).  Row ``m`` of the result depends
    on ``x[m]``, ``q`` and ``n_splits`` only.  HIP tensors launch the kernel
    and raise on a refused shape; CPU tensors compute against
    ``dequantize_mx(q)``."""
    if not isinstance(q, MXWeight):
        raise TypeError(f"mx_nt: q must be an MXWeight, not {type(q).__name__}")
    if x.dim() != 2 or x.shape[1] != q.shape[1]:
        raise ValueError(f"mx_nt: operand shapes {tuple(x.shape)} and {q.shape} do not match")
    (M, K), N = x.shape, q.shape[0]
    if swiglu and N % 2:
        raise ValueError(f"mx_nt: swiglu needs an even number of weight rows, got {N}")
    oshape = (M, N // 2) if swiglu else (M, N)
    if out is not None:
        if tuple(out.shape) != oshape or out.device != x.device:
            raise ValueError(f"mx_nt: out must be {oshape} on {x.device}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"mx_nt: out_dtype {out_dtype} != out.dtype {out.dtype}")
        out_dtype = out.dtype
    if not x.is_cuda:
        return skinny_nt(x, dequantize_mx(q, x.dtype), out=out, out_dtype=out_dtype, swiglu=swiglu)
    if x.dtype != torch.bfloat16 or q.device != x.device:
        raise TypeError(f"mx_nt: bf16 x and the weight on one HIP device required (got {x.dtype} on {x.device}, "
                        f"weight on {q.device})")
    out_dtype = out_dtype or torch.bfloat16
    if out_dtype not in (torch.bfloat16, torch.float32) or (swiglu and out_dtype != torch.bfloat16):
        raise TypeError(f"mx_nt: output must be bf16{'' if swiglu else ' or fp32'}, not {out_dtype}")
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=out_dtype)
    for t, what in ((x, "x"), (out, "out")):
        if t.stride(1) != 1:
            raise RuntimeError(f"mx_nt: {what} must have unit inner stride (strides {t.stride()})")
    lda, ldc = (t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in (x, out))
    L = _lib.lib()
    fmt = MX_FORMATS[q.fmt]
    ns = int(L.pto_gemm_mx_splits(M, N, K, fmt)) if n_splits is None else int(n_splits)
    nbytes = L.pto_gemm_mx_workspace(M, N, ns) if ns > 1 else 0
    ws = _skinny_workspace(x.device, nbytes) if nbytes > 0 else None
    rc = L.pto_gemm_mx(x.data_ptr(), lda, q.data.data_ptr(), q.scales.data_ptr(), out.data_ptr(), ldc,
                       int(out_dtype == torch.float32), int(bool(swiglu)), fmt, M, N, K, ns, _lib.ptr(ws),
                       nbytes if ws is not None else 0, _lib.stream_ptr(x.device))
    if rc == -1:
        raise RuntimeError(f"mx_nt: unsupported shape or layout: x {tuple(x.shape)} strides {x.stride()}, {q.fmt} "
                           f"weight {q.shape}, out strides {out.stride()}, n_splits {ns} (weight rows a multiple of "
                           "32 (64 with swiglu), contraction a multiple of 128, row strides multiples of 8, 16-byte "
                           "aligned pointers, 1..64 splits)")
    _lib.check(rc, "mx_nt")
    return out


def linear_mx(x, q: MXWeight, swiglu: bool = False):
    """The bias-free linear layer ``x [..., k_in]`` against the packed weight
    ``q`` alone (no bf16 copy of it is read), with ``swiglu`` the SwiGLU of a
    fused gate|up weight applied to it.  bf16 HIP tensors go by row count: up
    to :data:`SKINNY_MAX_ROWS` rows :func:`skinny_mx_nt` where it takes the
    shape, otherwise :func:`mx_nt`.  CPU tensors, other dtypes and shapes both
    kernels refuse dequantise ``q`` and call ``F.linear`` (and
    :func:`..ops.llm.swiglu`)."""
    n_out, k_in = q.shape
    rows = x.numel() // max(x.shape[-1], 1)
    if x.is_cuda and x.dtype == torch.bfloat16 and q.device == x.device and x.shape[-1] == k_in and rows >= 1:
        fn = None
        if skinny_mx_takes(rows, n_out, k_in, swiglu):
            fn = skinny_mx_nt
        elif mx_takes(rows, n_out, k_in, swiglu):
            fn = mx_nt
        if fn is not None:
            y = fn(_rows(x), q, swiglu=swiglu)
            return y.view(*x.shape[:-1], y.shape[-1])
    y = F.linear(x, dequantize_mx(q, x.dtype))
    if swiglu and y.is_cuda and y.dtype == torch.bfloat16:
        from . import llm

        y = llm.swiglu(y)
    elif swiglu:  # llm.swiglu's arithmetic in torch, as skinny_nt's CPU path
        g, u = y.float().chunk(2, dim=-1)
        y = ((g * torch.sigmoid(g)).to(x.dtype).float() * u).to(x.dtype)
    return y


def linear_decode(x, w, swiglu: bool = False, mx: MXWeight | None = None):
    """The bias-free linear layer of a decode step, ``x [B, k_in]`` against
    ``w [n_out, k_in]``, with ``swiglu`` the SwiGLU of a fused gate|up weight
    applied to it.  ``mx``: the quantised form of ``w``
    (:func:`quantize_mx`; ``w`` holds its dequantised values); bf16 HIP
    tensors of a shape :func:`skinny_mx_takes` then read it through
    :func:`skinny_mx_nt` whatever ``PTO_SKINNY`` says -- attaching a quantised
    weight is the opt-in.  Otherwise bf16 HIP tensors under a ``"hip"``
    :func:`skinny_plan` take :func:`skinny_nt` (one launch, no ``[B, 2F]``
    intermediate); everything else makes the calls of :func:`linear` and
    :func:`..ops.llm.swiglu`."""
    if mx is not None and x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 \
            and skinny_mx_takes(x.shape[0], mx.shape[0], mx.shape[1], swiglu):
        return skinny_mx_nt(_rows(x), mx, swiglu=swiglu)
    if x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 \
            and skinny_takes(x.shape[0], w.shape[0], w.shape[1], swiglu) \
            and skinny_plan(x.shape[0], w.shape[0], w.shape[1]) == "hip":
        return skinny_nt(_rows(x), w, swiglu=swiglu)
    y = linear(x, w)
    if swiglu:
        from . import llm

        y = llm.swiglu(y)
    return y
