"""Autograd wrappers over the bf16 transformer kernels
(``csrc/kernels/llm_kernels.hip``) used by :mod:`..models.llama`.

The ops take bf16 HIP tensors and raise on anything else (no silent
fallback): :func:`add_rmsnorm` (residual add + RMSNorm, the residual
gradient add fused into the RMSNorm backward), :func:`swiglu`,
:func:`rope_` (in place on the fused QKV projection), and
:func:`cross_entropy` (vocab-wide CE on bf16 logits, gradient written in
place into the logits buffer so no fp32 ``[tokens, 128256]`` tensor ever
exists).  :class:`EvalAccumulator` is the evaluation side of the cross
entropy: plain NLL and top-1 / top-k counts summed on the device.

The generation ops at the end of the file (``csrc/kernels/decode.hip``) --
:func:`rope_kv_append`, :func:`attention_decode`, :func:`sample` -- are
inference only and also run on CPU tensors and unsupported shapes, through
torch implementations of the same rules.
"""
from __future__ import annotations

import torch

from . import _lib


def _req(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: HIP device tensor required")
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name}: bf16 only (got {t.dtype})")
    return t.contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


class _AddRMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, w, eps):
        x = _req(x, "add_rmsnorm")
        w = _req(w, "add_rmsnorm")
        D = x.shape[-1]
        M = x.numel() // D
        y = torch.empty_like(x)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        if r is not None:
            r = _req(r, "add_rmsnorm")
            h = torch.empty_like(x)
        else:
            h = x
        _lib.check(_lib.lib().pto_add_rmsnorm_fwd(x.data_ptr(), _p(r), w.data_ptr(), _p(h if r is not None else None),
                                                   y.data_ptr(), rstd.data_ptr(), M, D, float(eps),
                                                   _lib.stream_ptr(x.device)), "add_rmsnorm_fwd")
        ctx.save_for_backward(h, w, rstd)
        ctx.has_res = r is not None
        ctx.set_materialize_grads(False)  # an unused h output costs no zero tensor
        if r is None:
            return y
        return h, y

    @staticmethod
    def backward(ctx, *grads):
        h, w, rstd = ctx.saved_tensors
        if ctx.has_res:
            dh, dy = grads
        else:
            dh, dy = None, grads[0]
        D = h.shape[-1]
        M = h.numel() // D
        L = _lib.lib()
        dy = torch.zeros_like(h) if dy is None else dy.contiguous()
        if dh is not None:
            dh = dh.contiguous()
        dx = torch.empty_like(h)
        dw = torch.empty_like(w)
        part = torch.empty(L.pto_rmsnorm_bwd_groups(M), D, device=h.device, dtype=torch.float32)
        _lib.check(L.pto_rmsnorm_bwd(dy.data_ptr(), h.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dh), dx.data_ptr(),
                                     dw.data_ptr(), part.data_ptr(), M, D, _lib.stream_ptr(h.device)), "rmsnorm_bwd")
        return dx, (dx if ctx.has_res else None), dw, None


def add_rmsnorm(x, residual, weight, eps: float = 1e-5):
    """``h = x + residual; y = rmsnorm(h) * weight`` -> ``(h, y)``."""
    return _AddRMSNorm.apply(x, residual, weight, eps)


def rmsnorm(x, weight, eps: float = 1e-5):
    return _AddRMSNorm.apply(x, None, weight, eps)


class TStash:
    """A gradient handed TRANSPOSED from one backward node to the next: the
    SwiGLU backward writes d(gate|up)^T while it computes d(gate|up), and the
    gate|up projection's K-contiguous weight gradient (:class:`_LinearTW`)
    takes it instead of transposing the [tokens x 2F] gradient itself."""

    __slots__ = ("t",)

    def __init__(self):
        self.t = None

    def take(self):
        t, self.t = self.t, None
        return t


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu, tstash=None):
        gu = _req(gu, "swiglu")
        F2 = gu.shape[-1]
        M = gu.numel() // F2
        out = torch.empty(*gu.shape[:-1], F2 // 2, device=gu.device, dtype=gu.dtype)
        _lib.check(_lib.lib().pto_swiglu_fwd(gu.data_ptr(), out.data_ptr(), M, F2 // 2, _lib.stream_ptr(gu.device)),
                   "swiglu_fwd")
        ctx.save_for_backward(gu)
        ctx.tstash = tstash
        return out

    @staticmethod
    def backward(ctx, dout):
        (gu,) = ctx.saved_tensors
        F2 = gu.shape[-1]
        M = gu.numel() // F2
        dout = dout.contiguous()
        dgu = torch.empty_like(gu)
        st = ctx.tstash
        if st is not None and M % 8 == 0 and (F2 // 2) % 64 == 0:
            dgu_t = torch.empty(F2, M, device=gu.device, dtype=gu.dtype)
            _lib.check(_lib.lib().pto_swiglu_bwd_t(gu.data_ptr(), dout.data_ptr(), dgu.data_ptr(), dgu_t.data_ptr(),
                                                   M, F2 // 2, _lib.stream_ptr(gu.device)), "swiglu_bwd_t")
            st.t = dgu_t
        else:
            _lib.check(_lib.lib().pto_swiglu_bwd(gu.data_ptr(), dout.data_ptr(), dgu.data_ptr(), M, F2 // 2,
                                                 _lib.stream_ptr(gu.device)), "swiglu_bwd")
        return dgu, None


def swiglu(gu, tstash: TStash | None = None):
    """``silu(gu[..., :F]) * gu[..., F:]`` for the fused gate|up projection.
    ``tstash``: also hand the transposed input gradient to the producer of
    ``gu`` (see :class:`TStash`)."""
    return _SwiGLU.apply(gu, tstash)


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, seq_len, n_rot, head_dim):
        if not qkv.is_contiguous():
            raise ValueError("rope_: qkv must be contiguous")
        _req(qkv, "rope_")
        M = qkv.numel() // qkv.shape[-1]
        _lib.check(_lib.lib().pto_rope(qkv.data_ptr(), None, cos.data_ptr(), sin.data_ptr(), M, seq_len, n_rot, 0,
                                       head_dim, qkv.shape[-1], 0, _lib.stream_ptr(qkv.device)), "rope_fwd")
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (seq_len, n_rot, head_dim)
        return qkv

    @staticmethod
    def backward(ctx, g):
        cos, sin = ctx.saved_tensors
        S, n_rot, D = ctx.cfg
        # out of place: the incoming gradient may be referenced elsewhere
        g = g.contiguous()
        dg = torch.empty_like(g)
        M = g.numel() // g.shape[-1]
        _lib.check(_lib.lib().pto_rope(g.data_ptr(), dg.data_ptr(), cos.data_ptr(), sin.data_ptr(), M, S, n_rot,
                                       g.shape[-1] // D, D, g.shape[-1], 1, _lib.stream_ptr(g.device)), "rope_bwd")
        return dg, None, None, None, None, None


def rope_(qkv, cos, sin, seq_len: int, n_rot: int, head_dim: int):
    """Rotate (HF rotate_half convention) the first ``n_rot`` heads of every
    ``[.., heads*head_dim]`` row of ``qkv`` in place; rows are ordered
    ``(batch, position)`` and ``cos``/``sin`` are fp32 ``[seq_len, head_dim/2]``."""
    return _RoPE.apply(qkv, cos, sin, seq_len, n_rot, head_dim)


def rope_tables(seq_len: int, head_dim: int, theta: float, device, scaling: dict | None = None):
    """fp32 cos/sin tables ``[seq_len, head_dim/2]`` (Llama-3 frequency
    scaling applied when ``scaling`` is given, as in the Llama-3.1 recipe)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling:
        import math

        factor, lo, hi, old = (scaling["factor"], scaling["low_freq_factor"], scaling["high_freq_factor"],
                               scaling["original_max_position_embeddings"])
        wl = 2 * math.pi / inv
        smooth = ((old / wl) - lo) / (hi - lo)
        scaled = torch.where(wl > old / lo, inv / factor, inv)
        mid = (wl <= old / lo) & (wl >= old / hi)
        inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
    ang = torch.outer(torch.arange(seq_len, dtype=torch.float64), inv)
    return ang.cos().float().to(device), ang.sin().float().to(device)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, smoothing, z_coef):
        logits = _req(logits, "cross_entropy")
        V = logits.shape[-1]
        M = logits.numel() // V
        labels = labels.reshape(M).to(torch.int64).contiguous()
        lse = torch.empty(M, device=logits.device, dtype=torch.float32)
        rows = torch.empty(M, device=logits.device, dtype=torch.float32)
        ctx.ex = (smoothing, z_coef) if (smoothing or z_coef) else ()  # both 0: the plain kernels
        fwd = _lib.lib().pto_ce_fwd_ex if ctx.ex else _lib.lib().pto_ce_fwd
        _lib.check(fwd(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), rows.data_ptr(), M, V, ignore_index,
                       *ctx.ex, _lib.stream_ptr(logits.device)), "ce_fwd")
        valid = labels != ignore_index
        count = valid.sum().clamp_min(1).float()
        ctx.save_for_backward(logits, labels, lse, count)
        ctx.ignore_index = ignore_index
        loss = rows.sum() / count
        if not z_coef:
            return loss, None
        # the z part of the loss, z_coef * mean_valid(lse^2), from the kernel's lse: [M] floats, no logits pass
        z_part = z_coef * (lse.square() * valid).sum() / count
        ctx.mark_non_differentiable(z_part)
        return loss, z_part

    @staticmethod
    def backward(ctx, gout, _gz=None):
        logits, labels, lse, count = ctx.saved_tensors
        V = logits.shape[-1]
        M = logits.numel() // V
        scale = (gout.float() / count).reshape(1)
        # logits is an intermediate owned by this op (the producing GEMM's
        # backward needs only its inputs), so the gradient overwrites it.
        bwd = _lib.lib().pto_ce_bwd_ex if ctx.ex else _lib.lib().pto_ce_bwd
        _lib.check(bwd(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), scale.data_ptr(), M, V, ctx.ignore_index,
                       *ctx.ex, _lib.stream_ptr(logits.device)), "ce_bwd")
        return logits, None, None, None, None


def cross_entropy(logits, labels, ignore_index: int = -100, label_smoothing: float = 0.0, z_loss: float = 0.0,
                  return_z: bool = False):
    """Mean token cross-entropy over non-ignored labels on bf16 logits.

    ``label_smoothing`` (eps) and ``z_loss`` (zc) extend the row loss to
    ``(1-eps)*(lse - z[y]) + eps*(lse - mean(z)) + zc*lse^2``: the first two
    terms are ``F.cross_entropy(..., label_smoothing=eps)``, the third is the
    z-loss on the softmax normaliser.  Both at 0 run the plain kernels.
    ``return_z=True`` returns ``(loss, z_part)``, ``z_part`` the detached
    ``zc * mean_valid(lse^2)`` already contained in ``loss`` (a device scalar;
    ``None`` when ``z_loss == 0``)."""
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"cross_entropy: label_smoothing must be in [0, 1), got {label_smoothing}")
    if not z_loss >= 0.0:
        raise ValueError(f"cross_entropy: z_loss must be >= 0, got {z_loss}")
    loss, z_part = _CrossEntropy.apply(logits, labels, ignore_index, float(label_smoothing), float(z_loss))
    return (loss, z_part) if return_z else loss


class EvalAccumulator:
    """Held-out metrics of a language model, accumulated on the device.

    The record is five fp64 numbers ``{loss_sum, tokens, top1, topk,
    bad_labels}``.  :meth:`update` adds the rows of one ``[..., V]`` logits
    tensor to it without a host sync: ``k_ce_eval`` writes each row's plain
    NLL (never smoothing or z-loss) and the rank of its label,
    ``#{z > z[y]} + #{c < y : z[c] == z[y]}`` -- ``rank == 0`` is
    ``argmax == label`` with torch's first-index tie rule, ``rank < k`` a
    top-k hit -- and ``k_eval_accum`` folds the rows in, in an order fixed by
    the row count alone.  Rows labelled ``ignore_index`` are skipped
    (rank -1); rows whose label is otherwise outside ``[0, V)`` are counted
    as bad (rank -2), never dereferenced, and make :meth:`result` raise.

    On HIP tensors the logits must be bf16 (no silent fallback).  On CPU
    tensors the same five quantities come from torch ops on any float dtype:
    the gloo/CPU trainer runs it and the GPU tests use it as the reference."""

    def __init__(self, device, topk: int = 5, ignore_index: int = -100):
        if int(topk) != topk or topk < 1:
            raise ValueError(f"EvalAccumulator: topk must be an integer >= 1, got {topk}")
        self.device = torch.device(device)
        self.k = int(topk)
        self.ignore_index = int(ignore_index)
        self.acc = torch.zeros(5, device=self.device, dtype=torch.float64)

    def reset(self):
        self.acc.zero_()

    @torch.no_grad()
    def update(self, logits, labels, return_rows: bool = False):
        """Add the rows of ``logits`` ``[..., V]`` / ``labels`` ``[...]`` to
        the record; ``return_rows``: also return ``(row_loss, row_rank)``."""
        V = logits.shape[-1]
        M = logits.numel() // V if V else 0
        if labels.numel() != M:
            raise ValueError(f"EvalAccumulator: {M} rows of logits, {labels.numel()} labels")
        if logits.is_cuda:
            logits = _req(logits.detach(), "EvalAccumulator")
            if logits.data_ptr() % 16:  # the kernel's 16-byte loads
                logits = logits.clone()
            labels = labels.reshape(M).to(device=logits.device, dtype=torch.int64).contiguous()
            row_loss = torch.empty(M, device=logits.device, dtype=torch.float32)
            row_rank = torch.empty(M, device=logits.device, dtype=torch.int32)
            L, s = _lib.lib(), _lib.stream_ptr(logits.device)
            _lib.check(L.pto_ce_eval(logits.data_ptr(), labels.data_ptr(), row_loss.data_ptr(), row_rank.data_ptr(),
                                     M, V, self.ignore_index, s), "ce_eval")
            _lib.check(L.pto_eval_accum(row_loss.data_ptr(), row_rank.data_ptr(), M, self.k, self.acc.data_ptr(), s),
                       "eval_accum")
        else:
            row_loss, row_rank = self._rows_torch(logits.detach().reshape(M, V), labels.reshape(M).to(torch.int64))
            ok = row_rank >= 0
            self.acc += torch.stack([row_loss.double().sum(), ok.sum().double(), (row_rank == 0).sum().double(),
                                     (ok & (row_rank < self.k)).sum().double(), (row_rank == -2).sum().double()])
        return (row_loss, row_rank) if return_rows else None

    def _rows_torch(self, z, y):
        M, V = z.shape
        if not z.is_floating_point():
            raise TypeError(f"EvalAccumulator: float logits required (got {z.dtype})")
        ignored = y == self.ignore_index
        valid = (y >= 0) & (y < V) & ~ignored
        yc = torch.where(valid, y, torch.zeros_like(y))[:, None]  # never index with a bad label
        zy = z.gather(1, yc) if V else z.new_zeros(M, 1)
        idx = torch.arange(V, device=z.device)[None, :]
        rank = (z > zy).sum(1) + ((z == zy) & (idx < yc)).sum(1)
        nll = torch.logsumexp(z.float(), dim=-1) - zy[:, 0].float()
        row_loss = torch.where(valid, nll, torch.zeros_like(nll))
        bad = torch.where(ignored, torch.full_like(y, -1), torch.full_like(y, -2))
        return row_loss, torch.where(valid, rank, bad).to(torch.int32)

    def all_reduce(self, group=None):
        """Sum the record over the ranks (one collective); nothing to do
        when torch.distributed is not initialised."""
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.acc, op=dist.ReduceOp.SUM, group=group)

    def result(self) -> dict:
        """The metrics of everything added since :meth:`reset` (the only
        host sync): mean NLL, its exp, top-1 / top-k accuracy as fractions."""
        loss_sum, tokens, top1, topk, bad = self.acc.tolist()
        if bad > 0:
            raise ValueError(f"EvalAccumulator: {int(bad)} labels are neither ignore_index ({self.ignore_index}) "
                             f"nor inside the vocabulary")
        n = int(tokens)
        if n == 0:
            return {"loss": float("nan"), "ppl": float("nan"), "top1": 0.0, "topk": 0.0, "k": self.k, "tokens": 0}
        import math

        loss = loss_sum / n
        try:
            ppl = math.exp(loss)
        except OverflowError:
            ppl = float("inf")
        return {"loss": loss, "ppl": ppl, "top1": top1 / n, "topk": topk / n, "k": self.k, "tokens": n}


def flash_attention_supported(S: int, H: int, Hkv: int, head_dim: int) -> bool:
    """Shapes the HIP kernels cover: head_dim 128, S % 128 == 0, H % Hkv == 0."""
    return head_dim == 128 and S % 128 == 0 and H % Hkv == 0 and ((S // 32) * (H // Hkv)) % 4 == 0


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, B, S, H, Hkv):
        qkv = _req(qkv, "flash_attention")
        D = 128
        rs = qkv.shape[-1]
        if rs != (H + 2 * Hkv) * D or qkv.numel() != B * S * rs:
            raise ValueError("flash_attention: qkv must be [B*S, (H + 2*Hkv)*128]")
        o = torch.empty(B * S, H * D, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, H, S, device=qkv.device, dtype=torch.float32)
        base = qkv.data_ptr()
        esz = qkv.element_size()
        _lib.check(_lib.lib().pto_attn_fwd(base, base + H * D * esz, base + (H + Hkv) * D * esz, o.data_ptr(),
                                           lse.data_ptr(), B, S, H, Hkv, rs, rs, rs, H * D, D ** -0.5,
                                           _lib.stream_ptr(qkv.device)), "attn_fwd")
        ctx.save_for_backward(qkv, o, lse)
        ctx.shape = (B, S, H, Hkv)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        B, S, H, Hkv = ctx.shape
        D = 128
        rs = qkv.shape[-1]
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(B, H, S, device=qkv.device, dtype=torch.float32)
        base, dbase, esz = qkv.data_ptr(), dqkv.data_ptr(), qkv.element_size()
        _lib.check(_lib.lib().pto_attn_bwd(base, base + H * D * esz, base + (H + Hkv) * D * esz, o.data_ptr(),
                                           do.data_ptr(), lse.data_ptr(), delta.data_ptr(), dbase,
                                           dbase + H * D * esz, dbase + (H + Hkv) * D * esz, rs, B, S, H, Hkv,
                                           rs, rs, rs, H * D, D ** -0.5, _lib.stream_ptr(qkv.device)), "attn_bwd")
        return dqkv, None, None, None, None


def flash_attention(qkv, B: int, S: int, H: int, Hkv: int):
    """Causal GQA attention straight from the fused QKV projection
    ``[B*S, (H + 2*Hkv)*128]`` (q heads, then k, then v heads per row) to
    ``O [B*S, H*128]`` — the layout the output projection consumes."""
    return _FlashAttention.apply(qkv, B, S, H, Hkv)


def transpose_into(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """``dst[:] = src.t()`` for 2-D bf16 HIP matrices (LDS-tiled kernel);
    plain copy on CPU tensors (tests)."""
    if src.dim() != 2 or dst.shape != (src.shape[1], src.shape[0]):
        raise ValueError(f"transpose_into: {tuple(src.shape)} -> {tuple(dst.shape)}")
    if not src.is_cuda:
        dst.copy_(src.t())
        return dst
    src, dst_c = _req(src, "transpose_into"), dst
    if not dst.is_contiguous() or dst.dtype != torch.bfloat16:
        raise ValueError("transpose_into: contiguous bf16 destination required")
    _lib.check(_lib.lib().pto_transpose_bf16(src.data_ptr(), dst_c.data_ptr(), src.shape[0], src.shape[1],
                                             src.stride(0), dst_c.stride(0), _lib.stream_ptr(src.device)),
               "transpose_bf16")
    return dst


class _LinearTW(torch.autograd.Function):
    """``y = x W^T`` whose input gradient is computed from the transposed
    copy ``Wt = W^T`` (``dX = dY Wt^T``): both dgrad operands are then
    K-contiguous, the layout the forward GEMM already uses.  hipBLASLt's
    pick for the usual ``dY W`` (B operand N-contiguous) ran at ~1.0
    PFLOP/s in the Llama-3-8B step vs ~1.5 for the K-contiguous one
    (profiles/llama8b_step_rocprof.md)."""

    @staticmethod
    def forward(ctx, x, w, wt, dw_kcontig, tstash=None):
        ctx.save_for_backward(x, wt)
        ctx.dw_kcontig, ctx.tstash = dw_kcontig, tstash
        return torch.nn.functional.linear(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        dx = torch.nn.functional.linear(dy, wt) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            x2 = x.reshape(-1, x.shape[-1])
            dy2 = dy.reshape(-1, dy.shape[-1])
            if ctx.dw_kcontig and x2.is_cuda:
                # dW = (dY^T)(X^T)^T from transposed activations: both operands
                # K(token)-contiguous.  Pays for w13/wo only
                # (tools/dw_layout_bench.py: 3.21 -> 2.39 + 0.51 ms, 0.58 ->
                # 0.38 + 0.14 ms at 4x4096 tokens)
                xt = transpose_into(x2.contiguous(), torch.empty(x2.shape[1], x2.shape[0], device=x2.device,
                                                                  dtype=x2.dtype))
                dyt = ctx.tstash.take() if ctx.tstash is not None else None  # written by the SwiGLU backward
                if dyt is None or dyt.shape != (dy2.shape[1], dy2.shape[0]):
                    dyt = transpose_into(dy2.contiguous(), torch.empty(dy2.shape[1], dy2.shape[0],
                                                                        device=dy2.device, dtype=dy2.dtype))
                dw = dyt.mm(xt.t())
            else:
                dw = dy2.t().mm(x2)
        return dx, dw, None, None, None


def linear_tw(x, w, wt, dw_kcontig: bool = False, tstash: TStash | None = None):
    """``F.linear(x, w)`` with the dgrad taken from ``wt`` (== ``w.t()``,
    kept current by the caller after every weight update); ``dw_kcontig``:
    weight gradient from transposed activations (``tstash``: the output
    gradient's transpose, if the next op's backward provides it)."""
    return _LinearTW.apply(x, w, wt, dw_kcontig, tstash)


# ---------------------------------------------------------------- KV-cache generation
# (csrc/kernels/decode.hip).  Each op runs its HIP kernel on bf16 HIP tensors
# of a supported shape and a torch implementation of the same rules on CPU
# tensors, other dtypes and unsupported shapes (``impl="torch"`` forces it).
# Neither path syncs with the host: lengths, step and flags stay on the device.

DECODE_KEY_TILE = 64


def _rotate_half(x):
    a, b = x.chunk(2, dim=-1)
    return torch.cat((-b, a), dim=-1)


def _hip_bf16(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in ts)


def _i32(t, name: str, n: int):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: contiguous int32 tensor of {n} elements required")
    return t


def rope_kv_append(qkv, cos, sin, k_cache, v_cache, lens, n_heads: int, n_kv_heads: int, impl: str | None = None):
    """Append the new token of every batch row to the KV cache.

    ``qkv`` ``[B, (H + 2*Hkv)*D]`` is the fused QKV projection of ONE new
    token per row, ``p = lens[b]`` (int32, device) its position, ``cos`` /
    ``sin`` the fp32 tables of :func:`rope_tables`.  The ``H`` query heads are
    rotated in place at position ``p``, the rotated K head and the V head are
    written to ``k_cache[b, :, p]`` / ``v_cache[b, :, p]`` (caches are
    ``[B, Hkv, max_len, D]``).  The arithmetic is :func:`rope_`'s, so the
    appended key is bitwise the key prefill produces at that position.  A row
    with ``p >= max_len`` or ``p`` at or past the table length is left alone
    entirely.  Returns ``qkv``."""
    B, Hkv, max_len, D = k_cache.shape
    H = int(n_heads)
    if Hkv != n_kv_heads or v_cache.shape != k_cache.shape:
        raise ValueError("rope_kv_append: caches must both be [B, Hkv, max_len, D]")
    if qkv.shape != (B, (H + 2 * Hkv) * D) or not qkv.is_contiguous():
        raise ValueError(f"rope_kv_append: qkv must be contiguous [B, (H + 2*Hkv)*D], got {tuple(qkv.shape)}")
    if cos.shape != sin.shape or cos.shape[-1] != D // 2:
        raise ValueError("rope_kv_append: cos/sin must be [positions, D/2]")
    _i32(lens, "rope_kv_append: lens", B)
    if impl != "torch" and _hip_bf16(qkv, k_cache, v_cache) and D % 8 == 0 and k_cache.is_contiguous() \
            and v_cache.is_contiguous():
        cos, sin = cos.contiguous(), sin.contiguous()
        if cos.dtype != torch.float32 or sin.dtype != torch.float32:
            raise TypeError("rope_kv_append: fp32 cos/sin tables required")
        _lib.check(_lib.lib().pto_rope_kv_append(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), k_cache.data_ptr(),
                                                 v_cache.data_ptr(), lens.data_ptr(), B, H, Hkv, D, max_len,
                                                 cos.shape[0], _lib.stream_ptr(qkv.device)), "rope_kv_append")
        return qkv
    limit = min(max_len, cos.shape[0])
    ok = ((lens >= 0) & (lens < limit))[:, None, None]
    p = lens.clamp(0, limit - 1).long()
    c = torch.cat([cos[p], cos[p]], -1)[:, None, :].float()
    s = torch.cat([sin[p], sin[p]], -1)[:, None, :].float()
    v3 = qkv.view(B, H + 2 * Hkv, D)
    rot = v3[:, :H + Hkv].float()
    rot = (rot * c + _rotate_half(rot) * s).to(qkv.dtype)
    v3[:, :H] = torch.where(ok, rot[:, :H], v3[:, :H])
    idx = p[:, None, None, None].expand(B, Hkv, 1, D)
    for cache, new in ((k_cache, rot[:, H:]), (v_cache, v3[:, H + Hkv:])):
        cache.scatter_(2, idx, torch.where(ok, new.to(cache.dtype), cache.gather(2, idx)[:, :, 0])[:, :, None])
    return qkv


def attention_decode_supported(H: int, Hkv: int, head_dim: int) -> bool:
    """Shapes the split-KV decode kernel covers: head_dim 64 or 128 and a GQA
    group ``H / Hkv`` of 1, 2, 4 or 8."""
    return Hkv > 0 and H % Hkv == 0 and head_dim in (64, 128) and H // Hkv in (1, 2, 4, 8)


def decode_splits(B: int, Hkv: int, max_len: int) -> int:
    """Default split count of :func:`attention_decode`, from host integers
    alone: about 512 ``(split, kv head, batch row)`` blocks for the 256 CUs,
    but no split shorter than 256 keys.  Within 5 % of the best count of the
    measured sweep at every shape of profiles/decode.md."""
    by_len = -(-int(max_len) // 256)
    by_cus = -(-512 // max(int(B) * int(Hkv), 1))
    return max(1, min(by_len, by_cus))


def decode_chunk(max_len: int, n_splits: int) -> int:
    """Keys per split: ``ceil(max_len / n_splits)`` rounded up to the key tile."""
    c = -(-int(max_len) // int(n_splits))
    return -(-c // DECODE_KEY_TILE) * DECODE_KEY_TILE


def attention_decode(q, k_cache, v_cache, lens, n_heads: int, n_kv_heads: int, n_splits: int | None = None,
                     impl: str | None = None):
    """One query row per head against the cached history: ``O [B, H*D]``.

    ``q`` holds the (rotated) query heads of the new token in its first
    ``H*D`` columns -- the fused QKV row ``[B, (H + 2*Hkv)*D]`` as it is, or
    ``[B, H*D]``.  Row ``b`` attends to the keys ``[0, lens[b])`` of the
    caches ``[B, Hkv, max_len, D]``; nothing past ``lens[b]`` is used, and
    ``lens[b] == 0`` gives zeros.  ``n_splits`` (default
    :func:`decode_splits`) workgroups share one head's history, each taking
    :func:`decode_chunk` keys, and a second launch combines their partial
    softmaxes in split order; the output bits depend on ``(inputs, lens,
    max_len, n_splits)`` only.  ``impl="sdpa"`` / ``"torch"``, CPU tensors
    and shapes outside :func:`attention_decode_supported` use torch's SDPA
    over the valid prefix."""
    B, Hkv, max_len, D = k_cache.shape
    H = int(n_heads)
    if Hkv != n_kv_heads or v_cache.shape != k_cache.shape or H % Hkv:
        raise ValueError("attention_decode: caches must both be [B, Hkv, max_len, D] with H % Hkv == 0")
    if q.dim() != 2 or q.shape[0] != B or q.shape[1] < H * D or q.stride(1) != 1:
        raise ValueError(f"attention_decode: q must be [B, >= H*D] with unit inner stride, got {tuple(q.shape)}")
    _i32(lens, "attention_decode: lens", B)
    if n_splits is not None and (int(n_splits) != n_splits or n_splits < 1):
        raise ValueError(f"attention_decode: n_splits must be an integer >= 1, got {n_splits}")
    if impl not in (None, "hip", "sdpa", "torch"):
        raise ValueError(f"attention_decode: impl must be hip|sdpa|torch, got {impl!r}")
    if impl in (None, "hip") and _hip_bf16(q, k_cache, v_cache) and attention_decode_supported(H, Hkv, D) \
            and k_cache.is_contiguous() and v_cache.is_contiguous():
        if q.stride(0) % 8 or q.data_ptr() % 16:
            q = q[:, :H * D].contiguous()
        ns = decode_splits(B, Hkv, max_len) if n_splits is None else int(n_splits)
        o = torch.empty(B, H * D, device=q.device, dtype=q.dtype)
        ml = po = None
        if ns > 1:
            ml = torch.empty(B, H, ns, 2, device=q.device, dtype=torch.float32)
            po = torch.empty(B, H, ns, D, device=q.device, dtype=torch.float32)
        _lib.check(_lib.lib().pto_attn_decode(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(),
                                              lens.data_ptr(), o.data_ptr(), _p(ml), _p(po), B, H, Hkv, D, max_len, ns,
                                              D ** -0.5, _lib.stream_ptr(q.device)), "attn_decode")
        return o
    valid = (torch.arange(max_len, device=q.device)[None, :] < lens[:, None])[:, None, :, None]  # [B, 1, max_len, 1]
    zero = torch.zeros((), device=q.device, dtype=k_cache.dtype)
    k = torch.where(valid, k_cache, zero)  # whatever the tail holds is discarded, never multiplied
    v = torch.where(valid, v_cache, zero)
    q4 = q[:, :H * D].reshape(B, H, 1, D)
    o = torch.nn.functional.scaled_dot_product_attention(q4, k.to(q.dtype), v.to(q.dtype),
                                                         attn_mask=valid.transpose(2, 3), enable_gqa=Hkv != H)
    o = torch.where((lens > 0)[:, None, None, None], o, torch.zeros((), device=q.device, dtype=o.dtype))
    return o.reshape(B, H * D)


def _sample_torch(z, u, temperature: float, top_k: int):
    """The sampler's rules on torch ops (fp64 CDF): ``z`` [B, V], ``u`` [B]."""
    zf = z.float()
    if temperature <= 0:
        return zf.argmax(-1)  # the first of equal maxima
    V = zf.shape[-1]
    if 0 < top_k < V:
        kept = zf >= zf.topk(top_k, dim=-1).values[:, -1:]  # ties at the k-th largest value are all kept
    else:
        kept = torch.ones_like(zf, dtype=torch.bool)
    zd = zf.double()
    w = torch.where(kept, torch.exp((zd - zd.max(-1, keepdim=True).values) / temperature), torch.zeros_like(zd))
    cdf = w.cumsum(-1)
    hit = kept & (cdf > u.double()[:, None] * cdf[:, -1:])
    first = hit.int().argmax(-1)  # first kept index whose running sum exceeds u * total
    last = V - 1 - kept.flip(-1).int().argmax(-1)
    return torch.where(hit.any(-1), first, last)


def sample(logits, u=None, temperature: float = 0.0, top_k: int = 0, cur=None, out=None, step=None, done=None,
           eos_id: int | None = None, lens=None, advance: bool = False, impl: str | None = None):
    """Pick one token per row of ``logits`` ``[B, V]``; returns ``cur`` ``[B]`` int64.

    * ``temperature == 0``: argmax, the first index among equal maxima.
    * ``temperature > 0``: a draw from ``softmax(z / T)`` over the kept set by
      inverse CDF in index order: the first kept index whose running sum of
      probabilities exceeds ``u[step, b]``.  ``u`` is ``[n_steps, B]`` fp32
      uniforms (``[B]`` counts as one step).
    * ``top_k > 0`` keeps every logit ``>=`` the k-th largest value, ties
      included.  No top-p.

    Bookkeeping, all on the device: with ``st = step[0]`` (int32 ``[1]``; 0
    without ``step``) the token is written to ``cur[b]`` and ``out[b, st]``
    (int64 ``[B, n_steps]``); a row whose ``done[b]`` (int32) is set emits
    ``eos_id``, a row that emits ``eos_id`` sets it; ``advance`` then adds 1
    to ``step[0]`` and to every ``lens[b]`` (either may be None).

    bf16 HIP logits with ``V % 8 == 0`` run ``k_sample`` (no scalar tail: the
    kernel refuses other widths, as ``k_ce_eval`` does); everything else runs
    the same rules on torch ops."""
    if logits.dim() != 2:
        raise ValueError(f"sample: logits must be [B, V], got {tuple(logits.shape)}")
    B, V = logits.shape
    temperature, top_k = float(temperature), int(top_k)
    if not temperature >= 0.0 or top_k < 0:
        raise ValueError(f"sample: temperature and top_k must be >= 0, got {temperature}, {top_k}")
    dev = logits.device
    if temperature > 0:
        if u is None:
            raise ValueError("sample: temperature > 0 needs the uniforms u")
        u = u.reshape(-1, B)
        if u.dtype != torch.float32 or not u.is_contiguous():
            raise TypeError("sample: u must be contiguous fp32")
    n_steps = out.shape[1] if out is not None else (u.shape[0] if u is not None and u.dim() == 2 else 1)
    if u is not None and temperature > 0 and u.shape[0] != n_steps:
        raise ValueError(f"sample: u has {u.shape[0]} steps, out has {n_steps}")
    if cur is None:
        cur = torch.empty(B, device=dev, dtype=torch.int64)
    for t, name, shape in ((cur, "cur", (B,)), (out, "out", (B, n_steps))):
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"sample: {name} must be contiguous int64 {shape}")
    if step is not None:
        _i32(step, "sample: step", 1)
    if done is not None:
        _i32(done, "sample: done", B)
    if lens is not None:
        _i32(lens, "sample: lens", B)
    eos = -1 if eos_id is None else int(eos_id)
    if impl != "torch" and _hip_bf16(logits) and V % 8 == 0 and V >= 8:
        logits = logits.contiguous()
        if logits.data_ptr() % 16:
            logits = logits.clone()
        _lib.check(_lib.lib().pto_sample(logits.data_ptr(), _p(u) if temperature > 0 else None, cur.data_ptr(),
                                         _p(out), n_steps, _p(step), _p(done), B, V, temperature, top_k, eos,
                                         1 if advance else 0, _p(lens), _lib.stream_ptr(dev)), "sample")
        return cur
    st = None if step is None else step.long().clamp(0, n_steps - 1)  # [1], on the device
    urow = None
    if temperature > 0:
        urow = u[0] if st is None else u.index_select(0, st)[0]
    tok = _sample_torch(logits, urow, temperature, top_k)
    if done is not None:
        tok = torch.where(done != 0, torch.full_like(tok, eos), tok)
        if eos >= 0:
            done.copy_(((done != 0) | (tok == eos)).to(done.dtype))
    cur.copy_(tok)
    if out is not None:
        col = torch.zeros(1, device=dev, dtype=torch.int64) if st is None else st
        inside = torch.ones(1, device=dev, dtype=torch.bool) if step is None else (step >= 0) & (step < n_steps)
        idx = col.expand(B)[:, None]
        out.scatter_(1, idx, torch.where(inside, tok, out.gather(1, idx)[:, 0])[:, None])
    if advance:
        if step is not None:
            step += 1
        if lens is not None:
            lens += 1
    return cur
