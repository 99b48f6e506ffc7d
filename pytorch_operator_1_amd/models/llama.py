"""Llama-3 decoder (BASELINE config 4: "Llama-3-8B DDP 8 replicas,
grad-bucket all-reduce stress, 288 GB HBM sizing").

The reference has no transformer workload (its only model is the MNIST
``Net`` of ``examples/mnist/mnist.py:12-28``); this is the framework's
large-model DDP config, built MI355X-first:

* bf16 parameters / activations; GEMMs on hipBLASLt through ``F.linear``
  with the projections fused to cut launches and re-reads: one QKV GEMM
  (``wqkv = [wq; wk; wv]``), one gate|up GEMM (``w13 = [w1; w3]``).
  ``PTO_GEMM=1`` (``auto``: per measured shape, none so far) puts them on
  the package's own MFMA GEMM instead (:mod:`..ops.gemm`), which needs
  neither the ``W^T`` copies nor the activation transposes.
* Everything between GEMMs is one HIP kernel per boundary
  (:mod:`..ops.llm`): residual-add + RMSNorm (its backward also adds the
  residual-stream gradient), RoPE in place on the QKV output, SwiGLU, and
  the vocab-wide cross entropy on bf16 logits.
* Attention: ``F.scaled_dot_product_attention`` (causal, GQA) — the ROCm
  flash-attention path; q/k/v are strided views of the QKV output, so no
  transposes are materialised.
* Sizing: 8.03e9 params x (2 bf16 param + 2 bf16 grad + 12 fp32
  master/m/v) = 128 GB per GPU, leaving ~150 GB of the 288 GB HBM3E for
  activations (~4.4 MB/token without checkpointing), so a DDP replica
  holds 16-32k tokens per step with no sharding at all.

* Generation: :class:`KVCache`, :meth:`Llama.prefill`,
  :meth:`Llama.decode_step` and :meth:`Llama.generate` -- one new token per
  row against cached K/V, on the kernels of ``csrc/kernels/decode.hip``
  (cache append, split-KV decode attention, sampler), every length and
  counter on the device so a step replays from a captured graph.

``impl="torch"`` is a plain PyTorch implementation of the same math used as
the numerics reference (and for CPU tests).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field

import torch
import torch.nn as nn
import torch.nn.functional as F

# impl="hip" attention: "hip" = csrc/kernels/attention.hip (head_dim 128,
# S % 128 == 0; other shapes fall back to SDPA), "sdpa" = ROCm SDPA.  The
# decode step follows the same switch (csrc/kernels/decode.hip or SDPA).
ATTN_IMPL = os.environ.get("PTO_ATTN", "hip")


@dataclass
class LlamaConfig:
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    vocab_size: int = 128256
    ffn_dim: int = 14336
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    max_seq_len: int = 8192
    rope_scaling: dict | None = field(default=None)
    tie_embeddings: bool = False

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    def num_params(self) -> int:
        hd = self.head_dim
        attn = self.dim * (self.n_heads + 2 * self.n_kv_heads) * hd + self.n_heads * hd * self.dim
        mlp = 3 * self.dim * self.ffn_dim
        per_layer = attn + mlp + 2 * self.dim
        emb = self.vocab_size * self.dim * (1 if self.tie_embeddings else 2)
        return self.n_layers * per_layer + emb + self.dim

    def train_flops_per_token(self, seq_len: int) -> float:
        """6N (dense) + causal attention 6 * L * S * dim (fwd+bwd)."""
        n_dense = self.num_params() - self.vocab_size * self.dim  # embedding lookup is not a GEMM
        return 6.0 * n_dense + 6.0 * self.n_layers * seq_len * self.dim


CONFIGS = {
    "llama3-8b": LlamaConfig(),
    "llama3-1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_dim=8192),
    "llama3-tiny": LlamaConfig(dim=256, n_layers=2, n_heads=8, n_kv_heads=2, vocab_size=1024, ffn_dim=512,
                               max_seq_len=256),
    # head_dim 128: small enough for CLI tests, yet on the owned attention kernels (training and decode)
    "llama3-mini": LlamaConfig(dim=256, n_layers=2, n_heads=2, n_kv_heads=1, vocab_size=1024, ffn_dim=512,
                               max_seq_len=512),
}


def _rotate_half(x):
    a, b = x.chunk(2, dim=-1)
    return torch.cat((-b, a), dim=-1)


class LlamaBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig, device=None, dtype=None):
        super().__init__()
        kw = dict(device=device, dtype=dtype)
        hd = cfg.head_dim
        self.cfg = cfg
        self.attn_norm = nn.Parameter(torch.ones(cfg.dim, **kw))
        self.wqkv = nn.Linear(cfg.dim, (cfg.n_heads + 2 * cfg.n_kv_heads) * hd, bias=False, **kw)
        self.wo = nn.Linear(cfg.n_heads * hd, cfg.dim, bias=False, **kw)
        self.ffn_norm = nn.Parameter(torch.ones(cfg.dim, **kw))
        self.w13 = nn.Linear(cfg.dim, 2 * cfg.ffn_dim, bias=False, **kw)
        self.w2 = nn.Linear(cfg.ffn_dim, cfg.dim, bias=False, **kw)

    # -- attention core shared by both impls (qkv already rotated) --
    def _attend(self, qkv, B, S):
        c = self.cfg
        hd = c.head_dim
        v4 = qkv.view(B, S, c.n_heads + 2 * c.n_kv_heads, hd)
        q = v4[:, :, :c.n_heads].transpose(1, 2)
        k = v4[:, :, c.n_heads:c.n_heads + c.n_kv_heads].transpose(1, 2)
        v = v4[:, :, c.n_heads + c.n_kv_heads:].transpose(1, 2)
        # GQA without materialising repeated K/V (measured 0.70 vs 0.87 ms fwd
        # at 2x4096 tokens, plus no expand copies: profiles/llama8b_ops_r1.json)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=c.n_kv_heads != c.n_heads)
        return o.transpose(1, 2).reshape(B * S, c.n_heads * hd)

    def forward_hip(self, h, delta, rope, B, S, kv=None):
        from ..ops import llm

        c = self.cfg
        if delta is None:
            y = llm.rmsnorm(h, self.attn_norm, c.norm_eps)
        else:
            h, y = llm.add_rmsnorm(h, delta, self.attn_norm, c.norm_eps)
        qkv = _lin(y, self.wqkv)
        qkv = llm.rope_(qkv, rope[0], rope[1], S, c.n_heads + c.n_kv_heads, c.head_dim)
        if kv is not None:  # prefill: the rotated K and the V of this layer
            kv.append(qkv)
        if ATTN_IMPL == "hip" and llm.flash_attention_supported(S, c.n_heads, c.n_kv_heads, c.head_dim):
            ctx = llm.flash_attention(qkv, B, S, c.n_heads, c.n_kv_heads)  # [B*S, H*128], no transposes
        else:
            ctx = self._attend(qkv, B, S)
        attn = _lin(ctx, self.wo)
        h, y = llm.add_rmsnorm(h, attn, self.ffn_norm, c.norm_eps)
        # the SwiGLU backward hands w13's weight gradient its output
        # gradient already transposed (ops/llm.py TStash)
        # (a weight gradient on the package's GEMM reads dY as stored: no stash)
        st = llm.TStash() if getattr(self.w13, "dw_kcontig", False) and os.environ.get("PTO_SWIGLU_T", "1") == "1" \
            and _plan("wgrad", y, self.w13) == "lib" else None
        mlp = _lin(llm.swiglu(_lin(y, self.w13, st), st), self.w2)
        return h, mlp

    def forward_torch(self, h, delta, rope, B, S, kv=None):
        c = self.cfg
        if delta is not None:
            h = h + delta
        y = _rmsnorm_ref(h, self.attn_norm, c.norm_eps)
        qkv = F.linear(y, self.wqkv.weight)
        nr = (c.n_heads + c.n_kv_heads) * c.head_dim
        rot = qkv[:, :nr].reshape(B, S, -1, c.head_dim).float()
        cos = torch.cat([rope[0], rope[0]], -1)[None, :, None, :]
        sin = torch.cat([rope[1], rope[1]], -1)[None, :, None, :]
        rot = (rot * cos + _rotate_half(rot) * sin).to(qkv.dtype).reshape(B * S, nr)
        qkv = torch.cat([rot, qkv[:, nr:]], dim=1)
        if kv is not None:
            kv.append(qkv)
        attn = F.linear(self._attend(qkv, B, S), self.wo.weight)
        h = h + attn
        y = _rmsnorm_ref(h, self.ffn_norm, c.norm_eps)
        g, u = F.linear(y, self.w13.weight).chunk(2, dim=-1)
        mlp = F.linear(F.silu(g) * u, self.w2.weight)
        return h, mlp

    def decode(self, h, delta, rope, cache, layer: int, hip: bool):
        """One new token per batch row (``h`` [B, dim]) against the cache:
        the block of :meth:`forward_hip` / :meth:`forward_torch` with
        ``M = B``, the new K/V appended at ``cache.lens`` and the attention
        over ``cache.lens + 1`` keys."""
        from ..ops import llm

        c = self.cfg
        k, v = cache.k[layer], cache.v[layer]
        if hip:
            if delta is None:
                y = llm.rmsnorm(h, self.attn_norm, c.norm_eps)
            else:
                h, y = llm.add_rmsnorm(h, delta, self.attn_norm, c.norm_eps)
            qkv = _lin(y, self.wqkv)
            llm.rope_kv_append(qkv, rope[0], rope[1], k, v, cache.lens, c.n_heads, c.n_kv_heads)
            ctx = llm.attention_decode(qkv, k, v, cache.lens_incl, c.n_heads, c.n_kv_heads,
                                       impl="sdpa" if ATTN_IMPL == "sdpa" else None)
            h, y = llm.add_rmsnorm(h, _lin(ctx, self.wo), self.ffn_norm, c.norm_eps)
            return h, _lin(llm.swiglu(_lin(y, self.w13)), self.w2)
        if delta is not None:
            h = h + delta
        y = _rmsnorm_ref(h, self.attn_norm, c.norm_eps)
        qkv = F.linear(y, self.wqkv.weight)
        llm.rope_kv_append(qkv, rope[0], rope[1], k, v, cache.lens, c.n_heads, c.n_kv_heads, impl="torch")
        ctx = llm.attention_decode(qkv, k, v, cache.lens_incl, c.n_heads, c.n_kv_heads, impl="torch")
        h = h + F.linear(ctx, self.wo.weight)
        y = _rmsnorm_ref(h, self.ffn_norm, c.norm_eps)
        g, u = F.linear(y, self.w13.weight).chunk(2, dim=-1)
        return h, F.linear(F.silu(g) * u, self.w2.weight)


class KVCache:
    """The state of one generation: per layer the rotated keys and the values
    of ``batch`` rows, bf16 (``dtype``) ``[batch, n_kv_heads, max_len,
    head_dim]`` so one head's keys are contiguous, and the device-side
    bookkeeping -- ``lens`` int32 ``[batch]`` (keys held per row), ``step``
    int32 ``[1]`` (tokens emitted), ``done`` int32 ``[batch]`` (row has
    emitted ``eos_id``).  Nothing past ``lens[b]`` is ever read."""

    def __init__(self, cfg: LlamaConfig, batch: int, max_len: int, device=None, dtype=torch.bfloat16):
        if batch < 1 or max_len < 1:
            raise ValueError(f"KVCache: batch and max_len must be >= 1, got {batch}, {max_len}")
        self.cfg, self.batch, self.max_len = cfg, int(batch), int(max_len)
        shape = (self.batch, cfg.n_kv_heads, self.max_len, cfg.head_dim)
        self.k = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(cfg.n_layers)]
        self.v = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(cfg.n_layers)]
        self.lens = torch.zeros(self.batch, device=device, dtype=torch.int32)
        self.lens_incl = torch.zeros(self.batch, device=device, dtype=torch.int32)  # lens + 1 during a decode step
        self.step = torch.zeros(1, device=device, dtype=torch.int32)
        self.done = torch.zeros(self.batch, device=device, dtype=torch.int32)

    def reset(self):
        for t in (self.lens, self.lens_incl, self.step, self.done):
            t.zero_()


def _lin(x, mod: nn.Linear, tstash=None):
    """Bias-free linear; with a transposed weight copy attached
    (:meth:`Llama.enable_transposed_dgrad`) the input gradient uses it."""
    from ..ops import gemm

    # each GEMM on the package's kernel or on the library (PTO_GEMM); all on
    # the library, it is F.linear / llm.linear_tw itself
    return gemm.linear(x, mod.weight, getattr(mod, "weight_t", None), getattr(mod, "dw_kcontig", False), tstash)


def _plan(kind: str, x, mod: nn.Linear) -> str:
    """Who runs the GEMM ``kind`` of ``mod`` on ``x``: ``ops.gemm.gemm_plan``
    for bf16 HIP tensors, the library for anything else."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and mod.weight.dtype == torch.bfloat16):
        return "lib"
    from ..ops import gemm

    return gemm.gemm_plan(kind, x.numel() // x.shape[-1], mod.out_features, mod.in_features)


def _rmsnorm_ref(x, w, eps):
    xf = x.float()
    n = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return w * n.to(x.dtype)


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig | str = "llama3-8b", impl: str = "hip", device=None,
                 dtype=torch.bfloat16, checkpoint: str = "none", init_std: float = 0.02,
                 label_smoothing: float = 0.0, z_loss: float = 0.0):
        """``label_smoothing`` / ``z_loss``: options of the training loss
        (:func:`..ops.llm.cross_entropy`).  After a forward with labels
        ``last_z_loss`` is the detached z part of the loss,
        ``z_loss * mean_valid(logsumexp^2)`` (``None`` when ``z_loss == 0``)."""
        super().__init__()
        if isinstance(cfg, str):
            cfg = CONFIGS[cfg]
        if impl not in ("hip", "torch"):
            raise ValueError(f"impl must be hip|torch, got {impl}")
        if checkpoint not in ("none", "full"):
            raise ValueError("checkpoint must be none|full")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        if not z_loss >= 0.0:
            raise ValueError(f"z_loss must be >= 0, got {z_loss}")
        self.cfg, self.impl, self.checkpoint = cfg, impl, checkpoint
        self.label_smoothing, self.z_loss = float(label_smoothing), float(z_loss)
        self.last_z_loss = None
        kw = dict(device=device, dtype=dtype)
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.dim, **kw)
        self.layers = nn.ModuleList(LlamaBlock(cfg, **kw) for _ in range(cfg.n_layers))
        self.norm = nn.Parameter(torch.ones(cfg.dim, **kw))
        self.lm_head = None if cfg.tie_embeddings else nn.Linear(cfg.dim, cfg.vocab_size, bias=False, **kw)
        self._rope = {}
        self.reset_parameters(init_std)

    @torch.no_grad()
    def reset_parameters(self, std: float = 0.02):
        out_std = std / math.sqrt(2 * self.cfg.n_layers)  # scaled residual-branch outputs
        for name, p in self.named_parameters():
            if p.dim() == 1:
                p.fill_(1.0)
            elif name.endswith("wo.weight") or name.endswith("w2.weight"):
                p.normal_(0.0, out_std)
            else:
                p.normal_(0.0, std)

    def rope(self, S: int, device):
        key = (S, str(device))
        if key not in self._rope:
            from ..ops.llm import rope_tables

            self._rope[key] = rope_tables(S, self.cfg.head_dim, self.cfg.rope_theta, device, self.cfg.rope_scaling)
        return self._rope[key]

    def linear_modules(self):
        mods = [m for blk in self.layers for m in (blk.wqkv, blk.wo, blk.w13, blk.w2)]
        return mods + ([self.lm_head] if self.lm_head is not None else [])

    def _mark_kcontig_dw(self):
        """Weight-gradient GEMMs that run faster from transposed activations
        (measured per shape, tools/dw_layout_bench.py): wo and w13."""
        for blk in self.layers:
            blk.wo.dw_kcontig = True
            blk.w13.dw_kcontig = True

    @torch.no_grad()
    def enable_transposed_dgrad(self):
        """Keep ``W^T`` next to every linear weight (bf16, +1x weight memory:
        16 GB for Llama-3-8B) so each dgrad GEMM reads K-contiguous operands.
        The copies must be refreshed after every weight update
        (:meth:`refresh_transposed`)."""
        for m in self.linear_modules():
            if getattr(m, "weight_t", None) is None:
                w = m.weight
                m.weight_t = torch.empty(w.shape[1], w.shape[0], device=w.device, dtype=w.dtype)
        self._mark_kcontig_dw()
        self.refresh_transposed()

    @torch.no_grad()
    def refresh_transposed(self):
        from ..ops import llm

        for m in self.linear_modules():
            wt = getattr(m, "weight_t", None)
            if wt is not None:
                llm.transpose_into(m.weight, wt)

    def _head_weight(self):
        return self.tok_emb.weight if self.lm_head is None else self.lm_head.weight

    def _final_hidden(self, tokens: torch.Tensor, kv=None):
        """Blocks and final norm: the ``[B*S, dim]`` input of the head GEMM
        (``kv``: a list that receives every layer's rotated QKV, for prefill)."""
        B, S = tokens.shape
        rope = self.rope(S, tokens.device)
        h = self.tok_emb(tokens).reshape(B * S, self.cfg.dim)
        delta = None
        for blk in self.layers:
            fn = blk.forward_hip if self.impl == "hip" else blk.forward_torch
            if self.checkpoint == "full" and self.training and torch.is_grad_enabled():
                from torch.utils.checkpoint import checkpoint

                h, delta = checkpoint(fn, h, delta, rope, B, S, use_reentrant=False)
            elif kv is not None:
                h, delta = fn(h, delta, rope, B, S, kv)
            else:
                h, delta = fn(h, delta, rope, B, S)
        if self.impl == "hip":
            from ..ops import llm

            return llm.add_rmsnorm(h, delta, self.norm, self.cfg.norm_eps)[1]
        return _rmsnorm_ref(h + delta, self.norm, self.cfg.norm_eps)

    def _head(self, y):
        if self.impl == "hip" and self.lm_head is not None:
            return _lin(y, self.lm_head)
        return F.linear(y, self._head_weight())

    @torch.no_grad()
    def evaluate(self, tokens: torch.Tensor, labels: torch.Tensor, acc, head_chunk: int | None = 2048):
        """Add the plain NLL and top-1 / top-k counts of ``tokens`` / ``labels``
        ``[B, S]`` to ``acc`` (:class:`..ops.llm.EvalAccumulator`) without a
        host sync.  The head GEMM (the path of :meth:`forward`) and the
        accumulator run on at most ``head_chunk`` rows at a time, so the
        ``[B*S, V]`` logits never exist at once (``None``: one chunk).
        Leaves ``training``, ``last_z_loss`` and every ``.grad`` alone."""
        if head_chunk is not None and head_chunk < 1:
            raise ValueError(f"head_chunk must be >= 1 or None, got {head_chunk}")
        y = self._final_hidden(tokens)
        labels = labels.reshape(-1)
        if labels.numel() != y.shape[0]:
            raise ValueError(f"evaluate: {y.shape[0]} tokens, {labels.numel()} labels")
        step = y.shape[0] if head_chunk is None else int(head_chunk)
        for r0 in range(0, y.shape[0], max(step, 1)):
            acc.update(self._head(y[r0:r0 + step]), labels[r0:r0 + step])
        return acc

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, lens: torch.Tensor | None, cache: KVCache):
        """Run the right-padded prompts ``tokens`` [B, P] through the training
        forward path, copy every layer's rotated K and its V into ``cache``
        and set ``cache.lens`` to ``lens`` (int32 [B] on the device; None: P
        for every row).  Returns the logits ``[B, V]`` at each row's last real
        position.  Causality keeps the padding out of every real position,
        and what the padding leaves in the cache lies past ``lens``."""
        B, P = tokens.shape
        c = self.cfg
        if B != cache.batch or P > cache.max_len:
            raise ValueError(f"prefill: {B} x {P} prompts do not fit a {cache.batch} x {cache.max_len} cache")
        if lens is None:
            lens = torch.full((B,), P, device=tokens.device, dtype=torch.int32)
        kv = []
        y = self._final_hidden(tokens, kv=kv)
        H, Hkv = c.n_heads, c.n_kv_heads
        for i, qkv in enumerate(kv):
            v4 = qkv.view(B, P, H + 2 * Hkv, c.head_dim)
            cache.k[i][:, :, :P].copy_(v4[:, :, H:H + Hkv].transpose(1, 2))
            cache.v[i][:, :, :P].copy_(v4[:, :, H + Hkv:].transpose(1, 2))
        cache.reset()
        cache.lens.copy_(lens)
        last = (lens.long() - 1).clamp(0, P - 1)[:, None, None].expand(B, 1, c.dim)
        return self._head(y.view(B, P, c.dim).gather(1, last)[:, 0].contiguous())

    @torch.no_grad()
    def decode_step(self, cur: torch.Tensor, cache: KVCache):
        """Logits ``[B, V]`` of the next position given one new token ``cur``
        [B] per row: its K/V are appended at ``cache.lens`` and it attends to
        the ``cache.lens + 1`` keys then held.  ``cache.lens`` itself is
        advanced by the sampler (:func:`..ops.llm.sample`), not here.  Every
        op takes its lengths from the device, so the step can be captured in
        a graph and replayed."""
        hip = self.impl == "hip"
        rope = self.rope(cache.max_len, cur.device)
        torch.add(cache.lens, 1, out=cache.lens_incl)
        h = self.tok_emb(cur)
        delta = None
        for i, blk in enumerate(self.layers):
            h, delta = blk.decode(h, delta, rope, cache, i, hip)
        if hip:
            from ..ops import llm

            y = llm.add_rmsnorm(h, delta, self.norm, self.cfg.norm_eps)[1]
        else:
            y = _rmsnorm_ref(h + delta, self.norm, self.cfg.norm_eps)
        return self._head(y)

    @torch.no_grad()
    def generate(self, prompts: torch.Tensor, prompt_lens=None, max_new_tokens: int = 16, temperature: float = 0.0,
                 top_k: int = 0, eos_id: int | None = None, seed: int = 0, graph: bool = False,
                 return_logits: bool = False, cache: KVCache | None = None):
        """Generate ``max_new_tokens`` tokens after each prompt: ``[B,
        max_new_tokens]`` int64 on the device (with ``return_logits`` also the
        ``[B, max_new_tokens, V]`` logits each token was chosen from).

        ``prompts`` [B, P] is right-padded, ``prompt_lens`` the real lengths
        as host integers (None: P for every row).  Prefill fills the KV cache
        (``cache``: one to reuse; default a new one of exactly the length
        needed), then every token costs one :meth:`decode_step` and one
        :func:`..ops.llm.sample`: greedy at ``temperature == 0``, else
        temperature / top-k sampling.  All uniforms are drawn once, before
        the loop, as ``[max_new_tokens, B]`` from a device generator seeded
        with ``seed`` and indexed by the device step counter, so the result
        is a function of (weights, prompts, options, seed).  A row that emits
        ``eos_id`` keeps emitting it.  Nothing in the loop syncs with the
        host.  ``graph=True`` warms one step eagerly, restores the step state,
        captures decode_step + sample + advance once and replays it for every
        token after the first; it returns the tokens of ``graph=False``.

        Leaves ``training``, every ``.grad`` and ``last_z_loss`` alone.
        Raises ValueError when ``max(prompt_lens) + max_new_tokens`` exceeds
        ``cfg.max_seq_len`` or the cache."""
        from ..ops import llm

        B, P = prompts.shape
        n_new = int(max_new_tokens)
        if n_new < 1:
            raise ValueError(f"generate: max_new_tokens must be >= 1, got {max_new_tokens}")
        host_lens = [P] * B if prompt_lens is None else [int(x) for x in prompt_lens]
        if len(host_lens) != B or min(host_lens) < 1 or max(host_lens) > P:
            raise ValueError(f"generate: prompt_lens must be {B} integers in [1, {P}]")
        need = max(host_lens) + n_new
        if need > self.cfg.max_seq_len:
            raise ValueError(f"generate: {max(host_lens)} prompt + {n_new} new tokens exceed max_seq_len "
                             f"{self.cfg.max_seq_len}")
        dev = prompts.device
        if cache is None:
            cache = KVCache(self.cfg, B, max(need, P), dev, self.tok_emb.weight.dtype)
        elif cache.batch != B or need > cache.max_len or P > cache.max_len:
            raise ValueError(f"generate: {B} rows of {need} tokens exceed the {cache.batch} x {cache.max_len} cache")
        lens = torch.tensor(host_lens, dtype=torch.int32).to(dev)
        u = None
        if temperature > 0:
            u = torch.rand(n_new, B, device=dev, dtype=torch.float32,
                           generator=torch.Generator(device=dev).manual_seed(int(seed)))
        out = torch.zeros(B, n_new, device=dev, dtype=torch.int64)
        cur = torch.zeros(B, device=dev, dtype=torch.int64)
        kept = torch.empty(B, n_new, self.cfg.vocab_size, device=dev, dtype=self.tok_emb.weight.dtype) \
            if return_logits else None
        opts = dict(u=u, temperature=temperature, top_k=top_k, cur=cur, out=out, step=cache.step, done=cache.done,
                    eos_id=eos_id, advance=True, impl=None if self.impl == "hip" else "torch")

        logits = self.prefill(prompts, lens, cache)
        if kept is not None:
            kept[:, 0].copy_(logits)
        llm.sample(logits, **opts)  # the first token is not in the cache yet: lens stays

        def one_step():
            z = self.decode_step(cur, cache)
            llm.sample(z, lens=cache.lens, **opts)
            return z

        use_graph = bool(graph) and dev.type == "cuda" and n_new > 1
        if use_graph:
            state = [t.clone() for t in (cur, cache.step, cache.lens, cache.done)]
            one_step()  # library handles, workspaces, the rope table; then put the step state back
            for t, saved in zip((cur, cache.step, cache.lens, cache.done), state):
                t.copy_(saved)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                z = one_step()
        for t in range(1, n_new):
            if use_graph:
                g.replay()
            else:
                z = one_step()
            if kept is not None:
                kept[:, t].copy_(z)
        return (out, kept) if return_logits else out

    def forward(self, tokens: torch.Tensor, labels: torch.Tensor | None = None):
        """``tokens`` [B, S] int64 -> mean CE loss if ``labels`` given, else logits."""
        B, S = tokens.shape
        y = self._final_hidden(tokens)
        logits = self._head(y)
        if self.impl == "hip":
            from ..ops import llm

            if labels is None:
                return logits.view(B, S, -1)
            loss, self.last_z_loss = llm.cross_entropy(logits, labels.reshape(-1), label_smoothing=self.label_smoothing,
                                                       z_loss=self.z_loss, return_z=True)
            return loss
        if labels is None:
            return logits.view(B, S, -1)
        labels = labels.reshape(-1)
        loss = F.cross_entropy(logits.float(), labels, label_smoothing=self.label_smoothing)
        if self.z_loss:
            valid = labels != -100  # F.cross_entropy's ignore_index
            lse2 = torch.logsumexp(logits.float(), dim=-1).square()
            z_part = self.z_loss * (lse2 * valid).sum() / valid.sum().clamp_min(1)
            self.last_z_loss = z_part.detach()
            loss = loss + z_part
        return loss


def synthetic_tokens(batch: int, seq_len: int, vocab: int, device, seed: int = 0):
    """Random token ids + next-token labels (no dataset access: synthetic)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randint(0, vocab, (batch, seq_len + 1), generator=g)
    return t[:, :-1].contiguous().to(device), t[:, 1:].contiguous().to(device)
