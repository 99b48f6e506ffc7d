#!/usr/bin/env python3
"""Cost of KV-cache generation (profiles/decode.md).

``--part attn``: ``ops.llm.attention_decode`` alone at the Llama-3-8B head
shape (H 32, Hkv 8, D 128), B in {1, 8}, a full cache of 1024 / 8192 / 32768
keys.  Sides per shape: the owned split-KV kernel with the default split
count (:func:`decode_splits`), SDPA on the valid prefix sliced out of the
same cache with a host-known length (the comparison baseline: the parent
commit has no decode path), and the op's own torch fallback
(``impl="sdpa"``, device-side lengths through a mask).  Then one sweep of
the owned kernel over ``n_splits``.  Every launch reads the next of several
cache copies whose total size exceeds the 256 MB last-level cache, so K/V
come from HBM.  Time is per call from HIP events around ``--reps``
back-to-back calls, median and min over ``--rounds``; bytes/s counts the K
and V bytes of the valid history once (2 * B * Hkv * len * D * 2 B).

``--part generate``: ``Llama.generate`` tokens/s, ``--new`` tokens after a
``--prompt``-token prompt, B in {1, 8}, eager against ``graph=True``, each
with ``PTO_SKINNY`` 0 and 1 (the decode linears on hipBLASLt or on the
package's skinny GEMM); host clock around a call that ends in a device
synchronise, the prefill (a call with one new token) timed the same way and
subtracted for the decode rate.

``--part linear``: every linear layer shape of ``--models`` at M in {1, 8,
16}: ``ops.gemm.skinny_nt`` against ``F.linear``, and for the gate|up weight
the SwiGLU-fused call against ``F.linear`` + ``llm.swiglu``.  Each call reads
the next of several weight copies (at least 768 MB in rotation); the two
sides alternate round by round in one process; bytes/s counts the weight
bytes once.  Then a sweep of ``n_splits`` for the ``wo`` / ``w2`` shapes.

``--part extend`` (profiles/extend.md): ``ops.llm.attention_extend`` at the
same head shape, T in {1, 4, 8, 16, 64} new tokens per row after a history of
1024 / 8192 / 32768 keys, B in {1, 8}, with the same rotation of cache copies:
the owned MFMA kernel with the default split count and over an ``n_splits``
sweep, SDPA with an explicit mask on the same cache, and T successive
``attention_decode`` calls (which share one cache copy).  Then
``Llama.prefill`` of ``4 * --prompt`` tokens unchunked against ``chunk=128``
and ``chunk=512``.

``--part mx`` (profiles/decode_mx.md): the weight-only MXFP4 / MXFP8 skinny
GEMM (``ops.gemm.skinny_mx_nt``) on the same layer shapes and row counts
against ``skinny_nt`` and ``F.linear`` on the bf16 weight, all sides
alternating round by round in one process, every side rotating over at least
768 MB of ITS OWN weight bytes (bytes/s counts those once); a sweep of
``n_splits`` at M = 1 for every shape and format; the graph-replayed decode
step of ``Llama.generate`` at B in {1, 8} on bf16 weights (``PTO_SKINNY`` 0
and 1) and after ``quantize_weights`` of each format; and, for information,
the logits of the quantised llama3-mini against its unquantised self.

``--part mxrows`` (profiles/gemm_mx_rows.md): the any-row MX GEMM
(``ops.gemm.mx_nt``) on the layer shapes of llama3-1b and llama3-8b at M in
{32, 64, 128, 512, 2048}, both formats (w13 also with the SwiGLU epilogue),
against ``F.linear`` on the dequantised bf16 weight (plus ``llm.swiglu``) and
the package's bf16 GEMM (``ops.gemm.gemm_nt``), sides alternating and weights
rotating as in ``--part mx``; bytes/s counts each side's own weight bytes
once, TFLOP/s ``2 M N K``.  A coarse ``n_splits`` sweep at M = 32 for every
shape.  Then llama3-8b end to end, ``quantize_weights(mxfp4)`` with the bf16
weights kept against ``keep_bf16=False``: ``torch.cuda.memory_allocated()``,
a 2048-token prefill, ``extend`` at B = 8, T = 8 and the graph-replayed decode
step at B = 8.

``--part kvfp8`` (profiles/decode_kv_fp8.md): ``attention_decode`` on a bf16
against a ``float8_e4m3fn`` cache at the (B, history) rows of ``--part attn``,
measured alternately, each side rotating over its own cache copies, bytes/s on
its own cache bytes; the fp8 side also at half and twice the default split
count.  Then the llama3-mini logits on an fp8 against a bf16 cache, and the
graph-replayed llama3-8b MXFP4 step at B = 8 on a 32768-token history with
``torch.cuda.memory_allocated`` per cache dtype.

One JSON line per row.

    python tools/decode_bench.py [--part attn|generate|linear|extend|mx|mxrows|kvfp8|all] [--rounds 15] [--reps 20]
                                 [--models llama3-1b] [--prompt 512] [--new 128] [--repeats 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CEILING = 6.29e12  # bytes/s, measured float4 copy (profiles/grad_clip.md)
H, HKV, D = 32, 8, 128
LLC_BYTES = 768 << 20  # rotate over at least this much K/V: three times the last-level cache


def timed(fn, rounds: int, reps: int):
    """(median, min) microseconds per call: HIP events around ``reps`` calls."""
    import torch

    for _ in range(2 * reps):
        fn()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def attn(args):
    import torch
    import torch.nn.functional as F

    from pytorch_operator_1_amd.ops import llm

    dev = torch.device("cuda")
    for B in (1, 8):
        for hist in (1024, 8192, 32768):
            kv_bytes = 2 * B * HKV * hist * D * 2
            ncopy = max(2, -(-LLC_BYTES // kv_bytes))
            g = torch.Generator(device=dev).manual_seed(0)
            ks = [torch.randn(B, HKV, hist, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(ncopy)]
            vs = [torch.randn(B, HKV, hist, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(ncopy)]
            q = torch.randn(B, H * D, device=dev, dtype=torch.bfloat16, generator=g)
            lens = torch.full((B,), hist, device=dev, dtype=torch.int32)
            q4 = q.view(B, H, 1, D)
            turn = [0]

            def nxt():
                turn[0] = (turn[0] + 1) % ncopy
                return ks[turn[0]], vs[turn[0]]

            def owned(ns=None):
                k, v = nxt()
                return llm.attention_decode(q, k, v, lens, H, HKV, n_splits=ns)

            def sdpa_slice():
                k, v = nxt()
                return F.scaled_dot_product_attention(q4, k[:, :, :hist], v[:, :, :hist], enable_gqa=True)

            def fallback():
                k, v = nxt()
                return llm.attention_decode(q, k, v, lens, H, HKV, impl="sdpa")

            turn[0] = 0
            o = owned().float()
            turn[0] = 0
            ref = sdpa_slice().reshape(B, H * D).float()  # the same cache copy
            err = float((o - ref).norm() / ref.norm())
            default = llm.decode_splits(B, HKV, hist)
            base = {"B": B, "history": hist, "kv_MB": round(kv_bytes / 2**20, 1), "cache_copies": ncopy,
                    "rounds": args.rounds, "reps": args.reps}

            def row(case, med, mn, **kw):
                print(json.dumps({**base, "case": case, **kw, "median_us": round(med, 2), "min_us": round(mn, 2),
                                  "TBps_median": round(kv_bytes / med / 1e6, 3),
                                  "fraction_of_ceiling": round(kv_bytes / (med * 1e-6) / CEILING, 3)}), flush=True)

            row("owned (default splits)", *timed(owned, args.rounds, args.reps), n_splits=default,
                chunk=llm.decode_chunk(hist, default), relerr_vs_sdpa=round(err, 5))
            row("sdpa on the sliced prefix", *timed(sdpa_slice, args.rounds, args.reps))
            try:
                row("torch fallback (impl=sdpa)", *timed(fallback, args.rounds, max(2, args.reps // 4)))
            except RuntimeError as e:  # a baseline that does not run is reported, not hidden
                print(json.dumps({**base, "case": "torch fallback (impl=sdpa)", "error": str(e)[:200]}), flush=True)
            ns = 1
            while ns <= min(256, hist // 64):
                row("owned, n_splits sweep", *timed(lambda: owned(ns), args.rounds, args.reps), n_splits=ns,
                    chunk=llm.decode_chunk(hist, ns))
                ns *= 2
            del ks, vs
            torch.cuda.empty_cache()


def timed_pair(fns, rounds: int, reps: int):
    """``timed`` for several callables measured alternately, round by round:
    a list of (median, min) microseconds per call."""
    import torch

    for fn in fns:
        for _ in range(reps):
            fn()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3 / reps)
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def linear_shapes(cfg):
    """(layer, n_out, k_in) of the decode step's linear layers."""
    qkv = (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
    return [("wqkv", qkv, cfg.dim), ("wo", cfg.dim, cfg.n_heads * cfg.head_dim), ("w13", 2 * cfg.ffn_dim, cfg.dim),
            ("w2", cfg.dim, cfg.ffn_dim), ("head", cfg.vocab_size, cfg.dim)]


def linear(args):
    import torch
    import torch.nn.functional as F

    from pytorch_operator_1_amd.models.llama import CONFIGS
    from pytorch_operator_1_amd.ops import gemm, llm

    dev = torch.device("cuda")
    for name in args.models.split(","):
        for layer, n_out, k_in in linear_shapes(CONFIGS[name]):
            w_bytes = n_out * k_in * 2
            ncopy = max(2, -(-LLC_BYTES // w_bytes))
            g = torch.Generator(device=dev).manual_seed(0)
            ws = [torch.randn(n_out, k_in, device=dev, dtype=torch.bfloat16, generator=g) * k_in ** -0.5
                  for _ in range(ncopy)]
            turn = [0]

            def nxt():
                turn[0] = (turn[0] + 1) % ncopy
                return ws[turn[0]]

            def row(case, med, mn, **kw):
                print(json.dumps({"model": name, "layer": layer, "n_out": n_out, "k_in": k_in, **kw, "case": case,
                                  "weight_MB": round(w_bytes / 2**20, 1), "weight_copies": ncopy,
                                  "rounds": args.rounds, "reps": args.reps, "median_us": round(med, 2),
                                  "min_us": round(mn, 2), "TBps_median": round(w_bytes / med / 1e6, 3),
                                  "fraction_of_ceiling": round(w_bytes / (med * 1e-6) / CEILING, 3)}), flush=True)

            for M in (1, 8, 16):
                x = torch.randn(M, k_in, device=dev, dtype=torch.bfloat16, generator=g)
                ns = gemm.skinny_splits(n_out, k_in)
                err = float((gemm.skinny_nt(x, ws[0]).float() - F.linear(x, ws[0]).float()).norm() /
                            F.linear(x, ws[0]).float().norm())
                sides = [("skinny_nt", lambda: gemm.skinny_nt(x, nxt())), ("F.linear", lambda: F.linear(x, nxt()))]
                if layer == "w13":
                    sides += [("skinny_nt swiglu", lambda: gemm.skinny_nt(x, nxt(), swiglu=True)),
                              ("F.linear + llm.swiglu", lambda: llm.swiglu(F.linear(x, nxt())))]
                for (case, _), (med, mn) in zip(sides, timed_pair([f for _, f in sides], args.rounds, args.reps)):
                    row(case, med, mn, M=M, n_splits=ns if case.startswith("skinny") else None,
                        relerr_vs_lib=round(err, 5))
            if layer in ("wo", "w2"):
                x = torch.randn(1, k_in, device=dev, dtype=torch.bfloat16, generator=g)
                sweep = [1, 2, 4, 8, 16, 32]
                res = timed_pair([lambda n=n: gemm.skinny_nt(x, nxt(), n_splits=n) for n in sweep], args.rounds,
                                 args.reps)
                for n, (med, mn) in zip(sweep, res):
                    row("skinny_nt, n_splits sweep", med, mn, M=1, n_splits=n)
            del ws
            torch.cuda.empty_cache()


def generate(args):
    import torch

    from pytorch_operator_1_amd.models.llama import CONFIGS, Llama

    dev = torch.device("cuda")
    for name in args.models.split(","):
        torch.manual_seed(0)
        model = Llama(CONFIGS[name], impl="hip", device=dev)
        for B in (1, 8):
            prompts = torch.randint(0, model.cfg.vocab_size, (B, args.prompt), device=dev,
                                    generator=torch.Generator(device=dev).manual_seed(1))

            def run_once(n_new, graph):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(prompts, max_new_tokens=n_new, graph=graph)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            def run(n_new, graph, skinny="0"):
                os.environ["PTO_SKINNY"] = skinny  # read at call time by ops.gemm.skinny_plan
                try:
                    return run_once(n_new, graph)
                finally:
                    os.environ.pop("PTO_SKINNY", None)

            outs = {}
            keys = [(graph, skinny) for skinny in ("0", "1") for graph in (False, True)]
            for graph, skinny in keys:  # warm every path: code objects, the library's picks, the rope tables
                run(args.new, graph, skinny)
            t = {"prefill0": [], "prefill1": [], **{k: [] for k in keys}}
            for skinny in ("0", "1"):
                run(1, False, skinny)
            for _ in range(args.repeats):
                for skinny in ("0", "1"):
                    t["prefill" + skinny].append(run(1, False, skinny)[0])
                for graph, skinny in keys:
                    dt, outs[graph, skinny] = run(args.new, graph, skinny)
                    t[graph, skinny].append(dt)
            for graph, skinny in keys:
                pre = sorted(t["prefill" + skinny])[len(t["prefill" + skinny]) // 2]
                ts = sorted(t[graph, skinny])
                med = ts[len(ts) // 2]
                print(json.dumps({"case": "generate graph" if graph else "generate eager", "PTO_SKINNY": int(skinny),
                                  "model": name, "B": B,
                                  "prompt": args.prompt, "new_tokens": args.new, "repeats": args.repeats,
                                  "median_ms": round(med * 1e3, 2), "min_ms": round(ts[0] * 1e3, 2),
                                  "prefill_ms": round(pre * 1e3, 2),
                                  "decode_ms_per_step": round((med - pre) / (args.new - 1) * 1e3, 4),
                                  "decode_tokens_per_s": round(B * (args.new - 1) / (med - pre), 1),
                                  "tokens_per_s_with_prefill": round(B * args.new / med, 1),
                                  "graph_equals_eager": bool(torch.equal(outs[False, skinny], outs[True, skinny])),
                                  "tokens_equal_PTO_SKINNY_0": bool(torch.equal(outs[graph, skinny],
                                                                                outs[graph, "0"]))}), flush=True)
        del model
        torch.cuda.empty_cache()


def extend(args):
    """T new tokens per row against ``history`` cached keys (lens = history, every token live)."""
    import torch
    import torch.nn.functional as F

    from pytorch_operator_1_amd.ops import llm

    dev = torch.device("cuda")
    for B in (1, 8):
        for hist in (1024, 8192, 32768):
            for T in (1, 4, 8, 16, 64):
                max_len = hist + T
                kv_bytes = 2 * B * HKV * max_len * D * 2
                ncopy = max(2, -(-LLC_BYTES // kv_bytes))
                g = torch.Generator(device=dev).manual_seed(0)
                ks = [torch.randn(B, HKV, max_len, D, device=dev, dtype=torch.bfloat16, generator=g)
                      for _ in range(ncopy)]
                vs = [torch.randn(B, HKV, max_len, D, device=dev, dtype=torch.bfloat16, generator=g)
                      for _ in range(ncopy)]
                q = torch.randn(B * T, H * D, device=dev, dtype=torch.bfloat16, generator=g)
                lens = torch.full((B,), hist, device=dev, dtype=torch.int32)
                n_new = torch.full((B,), T, device=dev, dtype=torch.int32)
                steps = [lens + t + 1 for t in range(T)]  # the lengths of T successive decode steps
                qt = [q.view(B, T, H * D)[:, t].contiguous() for t in range(T)]
                q4 = q.view(B, T, H, D).transpose(1, 2)
                mask = (torch.arange(max_len, device=dev)[None, :] <= hist + torch.arange(T, device=dev)[:, None])
                turn = [0]

                def nxt():
                    turn[0] = (turn[0] + 1) % ncopy
                    return ks[turn[0]], vs[turn[0]]

                def owned(ns=None):
                    k, v = nxt()
                    return llm.attention_extend(q, k, v, lens, n_new, T, H, HKV, n_splits=ns)

                def sdpa_mask():
                    k, v = nxt()
                    return F.scaled_dot_product_attention(q4, k, v, attn_mask=mask, enable_gqa=True)

                def decode_steps():
                    k, v = nxt()  # one copy for the T steps: the later ones may find it in the cache
                    return [llm.attention_decode(qt[t], k, v, steps[t], H, HKV) for t in range(T)]

                turn[0] = 0
                o = owned().float()
                turn[0] = 0
                ref = sdpa_mask().transpose(1, 2).reshape(B * T, H * D).float()  # the same cache copy
                err = float((o - ref).norm() / ref.norm())
                tiles = llm.extend_row_tiles(T, H, HKV)
                default = llm.decode_splits(B * tiles, HKV, max_len)
                base = {"B": B, "history": hist, "T": T, "kv_MB": round(kv_bytes / 2**20, 1), "cache_copies": ncopy,
                        "rounds": args.rounds, "reps": args.reps}

                def row(case, med, mn, **kw):
                    print(json.dumps({**base, "case": case, **kw, "median_us": round(med, 2), "min_us": round(mn, 2),
                                      "TBps_median": round(kv_bytes / med / 1e6, 3)}), flush=True)

                row("extend (default splits)", *timed(owned, args.rounds, args.reps), n_splits=default,
                    relerr_vs_sdpa=round(err, 5))
                row("sdpa, explicit mask", *timed(sdpa_mask, args.rounds, args.reps))
                row("T attention_decode calls", *timed(decode_steps, args.rounds, max(2, args.reps // 4)))
                ns = 1
                while ns <= min(256, max_len // 64):
                    row("extend, n_splits sweep", *timed(lambda: owned(ns), args.rounds, args.reps), n_splits=ns)
                    ns *= 4
                del ks, vs
                torch.cuda.empty_cache()
    prefill(args)


def prefill(args):
    """``Llama.prefill`` of a ``--prompt * 4``-token prompt, unchunked against ``chunk=`` (host clock, synchronised)."""
    import torch

    from pytorch_operator_1_amd.models.llama import CONFIGS, KVCache, Llama

    dev = torch.device("cuda")
    for name in args.models.split(","):
        torch.manual_seed(0)
        model = Llama(CONFIGS[name], impl="hip", device=dev)
        P = args.prompt * 4
        for B in (1, 8):
            tok = torch.randint(0, model.cfg.vocab_size, (B, P), device=dev)
            cache = KVCache(model.cfg, B, P, dev)
            for chunk in (None, 128, 512):
                ts = []
                for _ in range(args.repeats + 1):  # the first run warms up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.prefill(tok, None, cache, chunk=chunk)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                ts = sorted(ts[1:])
                print(json.dumps({"case": "prefill", "model": name, "B": B, "prompt": P, "chunk": chunk,
                                  "median_ms": round(ts[len(ts) // 2], 2), "min_ms": round(ts[0], 2),
                                  "repeats": args.repeats}), flush=True)
        del model
        torch.cuda.empty_cache()


def mx(args):
    """Weight-only MXFP4 / MXFP8 decode linears against the bf16 paths."""
    import torch
    import torch.nn.functional as F

    from pytorch_operator_1_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_1_amd.ops import gemm, llm

    dev = torch.device("cuda")
    fmts = ("mxfp4", "mxfp8")
    bits = {"mxfp4": 4.25, "mxfp8": 8.25}
    for name in args.models.split(","):
        for layer, n_out, k_in in linear_shapes(CONFIGS[name]):
            w_bytes = n_out * k_in * 2
            ncopy = max(2, -(-LLC_BYTES // w_bytes))
            g = torch.Generator(device=dev).manual_seed(0)
            ws = [torch.randn(n_out, k_in, device=dev, dtype=torch.bfloat16, generator=g) * k_in ** -0.5
                  for _ in range(ncopy)]
            # each format rotates over at least LLC_BYTES of its own (smaller) bytes
            qbytes = {f: int(n_out * k_in * bits[f] / 8) for f in fmts}
            qs = {f: [gemm.quantize_mx(ws[i % ncopy], f) for i in range(max(2, -(-LLC_BYTES // qbytes[f])))]
                  for f in fmts}
            turn = {"bf16": 0, **{f: 0 for f in fmts}}

            def nxt(kind):
                pool = ws if kind == "bf16" else qs[kind]
                turn[kind] = (turn[kind] + 1) % len(pool)
                return pool[turn[kind]]

            def row(case, med, mn, nbytes, **kw):
                print(json.dumps({"part": "mx", "model": name, "layer": layer, "n_out": n_out, "k_in": k_in, **kw,
                                  "case": case, "weight_MB": round(nbytes / 2**20, 1), "rounds": args.rounds,
                                  "reps": args.reps, "median_us": round(med, 2), "min_us": round(mn, 2),
                                  "TBps_median": round(nbytes / med / 1e6, 3),
                                  "fraction_of_ceiling": round(nbytes / (med * 1e-6) / CEILING, 3)}), flush=True)

            for M in (1, 8, 16):
                x = torch.randn(M, k_in, device=dev, dtype=torch.bfloat16, generator=g)
                sides = [(f"skinny_mx_nt {f}", (lambda f=f: gemm.skinny_mx_nt(x, nxt(f))), qbytes[f],
                          gemm.skinny_mx_splits(n_out, k_in, f)) for f in fmts]
                sides += [("skinny_nt", lambda: gemm.skinny_nt(x, nxt("bf16")), w_bytes,
                           gemm.skinny_splits(n_out, k_in)),
                          ("F.linear", lambda: F.linear(x, nxt("bf16")), w_bytes, None)]
                if layer == "w13":
                    sides += [(f"skinny_mx_nt {f} swiglu", (lambda f=f: gemm.skinny_mx_nt(x, nxt(f), swiglu=True)),
                               qbytes[f], gemm.skinny_mx_splits(n_out, k_in, f)) for f in fmts]
                    sides += [("skinny_nt swiglu", lambda: gemm.skinny_nt(x, nxt("bf16"), swiglu=True), w_bytes,
                               gemm.skinny_splits(n_out, k_in)),
                              ("F.linear + llm.swiglu", lambda: llm.swiglu(F.linear(x, nxt("bf16"))), w_bytes, None)]
                res = timed_pair([s[1] for s in sides], args.rounds, args.reps)
                for (case, _, nbytes, ns), (med, mn) in zip(sides, res):
                    row(case, med, mn, nbytes, M=M, n_splits=ns)
            x = torch.randn(1, k_in, device=dev, dtype=torch.bfloat16, generator=g)
            sweep = [1, 2, 4, 8, 16, 32]
            for f in fmts:
                res = timed_pair([lambda n=n: gemm.skinny_mx_nt(x, nxt(f), n_splits=n) for n in sweep], args.rounds,
                                 args.reps)
                for n, (med, mn) in zip(sweep, res):
                    row(f"skinny_mx_nt {f}, n_splits sweep", med, mn, qbytes[f], M=1, n_splits=n,
                        default=gemm.skinny_mx_splits(n_out, k_in, f))
            del ws, qs
            torch.cuda.empty_cache()

    # the graph-replayed decode step: bf16 weights on the library / on the skinny kernel, then quantised
    for name in args.models.split(","):
        torch.manual_seed(0)
        model = Llama(CONFIGS[name], impl="hip", device=dev)
        for B in (1, 8):
            prompts = torch.randint(0, model.cfg.vocab_size, (B, args.prompt), device=dev,
                                    generator=torch.Generator(device=dev).manual_seed(1))

            def run(n_new, skinny):
                os.environ["PTO_SKINNY"] = skinny
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.generate(prompts, max_new_tokens=n_new, graph=n_new > 1)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0
                finally:
                    os.environ.pop("PTO_SKINNY", None)

            def step_ms(skinny):
                run(args.new, skinny)  # warm: code objects, the library's picks, the capture path
                run(1, skinny)
                pre = sorted(run(1, skinny) for _ in range(args.repeats))[args.repeats // 2]
                tot = sorted(run(args.new, skinny) for _ in range(args.repeats))
                return (tot[len(tot) // 2] - pre) / (args.new - 1) * 1e3, (tot[0] - pre) / (args.new - 1) * 1e3

            cases = [("bf16, PTO_SKINNY=0", "0", None), ("bf16, PTO_SKINNY=1", "1", None),
                     ("quantize_weights(mxfp4)", "0", "mxfp4"), ("quantize_weights(mxfp8)", "0", "mxfp8")]
            for case, skinny, fmt in cases:
                model.drop_quantized()
                if fmt is not None:
                    model.quantize_weights(fmt)
                med, mn = step_ms(skinny)
                print(json.dumps({"part": "mx", "case": "graph-replayed decode step", "weights": case, "model": name,
                                  "B": B, "prompt": args.prompt, "new_tokens": args.new, "repeats": args.repeats,
                                  "decode_ms_per_step": round(med, 4), "decode_ms_per_step_min": round(mn, 4)}),
                      flush=True)
            model.drop_quantized()
        del model
        torch.cuda.empty_cache()

    # for information: logits of the quantised llama3-mini against its unquantised self
    tok = torch.randint(0, 1024, (4, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    for f in fmts:
        torch.manual_seed(0)
        model = Llama(CONFIGS["llama3-mini"], impl="hip", device=dev)
        with torch.no_grad():
            ref = model(tok).double()
            model.quantize_weights(f)
            got = model(tok).double()
        print(json.dumps({"part": "mx", "case": "llama3-mini logits, quantised vs unquantised", "fmt": f,
                          "relerr": round(float((got - ref).norm() / ref.norm()), 5)}), flush=True)


def mxrows(args):
    """The any-row MX GEMM against the bf16 paths; a model on its packed weights alone."""
    import torch
    import torch.nn.functional as F

    from pytorch_operator_1_amd.models.llama import CONFIGS, KVCache, Llama
    from pytorch_operator_1_amd.ops import gemm, llm

    dev = torch.device("cuda")
    fmts = ("mxfp4", "mxfp8")
    bits = {"mxfp4": 4.25, "mxfp8": 8.25}
    for name in ("llama3-1b", "llama3-8b"):
        for layer, n_out, k_in in linear_shapes(CONFIGS[name]):
            w_bytes = n_out * k_in * 2
            qbytes = {f: int(n_out * k_in * bits[f] / 8) for f in fmts}
            g = torch.Generator(device=dev).manual_seed(0)
            w0 = torch.randn(n_out, k_in, device=dev, dtype=torch.bfloat16, generator=g) * k_in ** -0.5
            pools = {}
            for f in fmts:  # each side rotates over at least LLC_BYTES of its own bytes; the values repeat
                q = gemm.quantize_mx(w0, f)
                pools[f] = [q] + [gemm.MXWeight(q.data.clone(), q.scales.clone(), f, q.shape)
                                  for _ in range(max(2, -(-LLC_BYTES // qbytes[f])) - 1)]
            wd = gemm.dequantize_mx(pools["mxfp4"][0])
            pools["bf16"] = [wd] + [wd.clone() for _ in range(max(2, -(-LLC_BYTES // w_bytes)) - 1)]
            del w0
            turn = {k: 0 for k in pools}

            def nxt(kind):
                turn[kind] = (turn[kind] + 1) % len(pools[kind])
                return pools[kind][turn[kind]]

            def row(case, med, mn, nbytes, M, **kw):
                print(json.dumps({"part": "mxrows", "model": name, "layer": layer, "n_out": n_out, "k_in": k_in, "M": M,
                                  **kw, "case": case, "weight_MB": round(nbytes / 2**20, 1), "rounds": args.rounds,
                                  "reps": args.reps, "median_us": round(med, 2), "min_us": round(mn, 2),
                                  "TBps_median": round(nbytes / med / 1e6, 3),
                                  "fraction_of_ceiling": round(nbytes / (med * 1e-6) / CEILING, 3),
                                  "TFLOPs_median": round(2 * M * n_out * k_in / med / 1e6, 1)}), flush=True)

            for M in (32, 64, 128, 512, 2048):
                x = torch.randn(M, k_in, device=dev, dtype=torch.bfloat16, generator=g)
                sides = [(f"mx_nt {f}", (lambda f=f: gemm.mx_nt(x, nxt(f))), qbytes[f], gemm.mx_splits(M, n_out, k_in, f))
                         for f in fmts]
                sides += [("F.linear", lambda: F.linear(x, nxt("bf16")), w_bytes, None),
                          ("gemm_nt", lambda: gemm.gemm_nt(x, nxt("bf16")), w_bytes, None)]
                if layer == "w13":
                    sides += [(f"mx_nt {f} swiglu", (lambda f=f: gemm.mx_nt(x, nxt(f), swiglu=True)), qbytes[f],
                               gemm.mx_splits(M, n_out, k_in, f)) for f in fmts]
                    sides += [("F.linear + llm.swiglu", lambda: llm.swiglu(F.linear(x, nxt("bf16"))), w_bytes, None)]
                res = timed_pair([s[1] for s in sides], args.rounds, args.reps)
                for (case, _, nbytes, ns), (med, mn) in zip(sides, res):
                    row(case, med, mn, nbytes, M, n_splits=ns)
            x = torch.randn(32, k_in, device=dev, dtype=torch.bfloat16, generator=g)
            sweep = [n for n in (1, 2, 4, 8, 16) if n <= max(1, k_in // 256)]
            res = timed_pair([lambda n=n: gemm.mx_nt(x, nxt("mxfp4"), n_splits=n) for n in sweep], args.rounds,
                             args.reps)
            for n, (med, mn) in zip(sweep, res):
                row("mx_nt mxfp4, n_splits sweep", med, mn, qbytes["mxfp4"], 32, n_splits=n,
                    default=gemm.mx_splits(32, n_out, k_in, "mxfp4"))
            del pools, wd
            torch.cuda.empty_cache()

    # llama3-8b end to end: the bf16 weights kept next to the packed ones, then released
    name, B = "llama3-8b", 8
    torch.manual_seed(0)
    model = Llama(CONFIGS[name], impl="hip", device=dev)
    cfg = model.cfg
    gen = torch.Generator(device=dev).manual_seed(1)
    long_prompt = torch.randint(0, cfg.vocab_size, (1, 2048), device=dev, generator=gen)
    chunk = torch.randint(0, cfg.vocab_size, (B, 8), device=dev, generator=gen)
    prompts = torch.randint(0, cfg.vocab_size, (B, args.prompt), device=dev, generator=gen)

    def clock(fn):
        ts = []
        for _ in range(args.repeats + 1):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = sorted(ts[1:])
        return round(ts[len(ts) // 2], 3), round(ts[0], 3)

    for keep in (True, False):
        before = torch.cuda.memory_allocated()
        model.quantize_weights("mxfp4", keep_bf16=keep)
        torch.cuda.synchronize()
        base = {"part": "mxrows", "model": name, "fmt": "mxfp4", "keep_bf16": keep, "repeats": args.repeats}
        print(json.dumps({**base, "case": "memory_allocated", "GB_before": round(before / 1e9, 2),
                          "GB_after": round(torch.cuda.memory_allocated() / 1e9, 2)}), flush=True)
        cache = KVCache(cfg, 1, 2048, dev)
        med, mn = clock(lambda: model.prefill(long_prompt, None, cache))
        print(json.dumps({**base, "case": "prefill", "B": 1, "prompt": 2048, "median_ms": med, "min_ms": mn}),
              flush=True)
        cache = KVCache(cfg, B, 1024, dev)

        def ext():
            cache.reset()
            cache.lens.fill_(512)
            model.extend(chunk, cache, logits="last")

        med, mn = clock(ext)
        print(json.dumps({**base, "case": "extend", "B": B, "T": 8, "history": 512, "median_ms": med, "min_ms": mn}),
              flush=True)
        del cache

        def run(n_new):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(prompts, max_new_tokens=n_new, graph=n_new > 1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        run(args.new)
        run(1)
        pre = sorted(run(1) for _ in range(args.repeats))[args.repeats // 2]
        tot = sorted(run(args.new) for _ in range(args.repeats))
        print(json.dumps({**base, "case": "graph-replayed decode step", "B": B, "prompt": args.prompt,
                          "new_tokens": args.new,
                          "decode_ms_per_step": round((tot[len(tot) // 2] - pre) / (args.new - 1) * 1e3, 4),
                          "decode_ms_per_step_min": round((tot[0] - pre) / (args.new - 1) * 1e3, 4)}), flush=True)


def kvfp8(args):
    import torch

    from pytorch_operator_1_amd.models.llama import CONFIGS, KVCache, Llama
    from pytorch_operator_1_amd.ops import llm

    dev = torch.device("cuda")
    fp8 = torch.float8_e4m3fn
    sc = torch.tensor([[0.5], [0.25], [2.0], [4.0]], device=dev).expand(4, HKV).contiguous()
    for B in (1, 8):
        for hist in (1024, 8192, 32768):
            nbytes = {"bf16": 2 * B * HKV * hist * D * 2, "fp8": 2 * B * HKV * hist * D}
            ncopy = max(2, -(-LLC_BYTES // nbytes["fp8"]))  # both sides rotate over at least the LLC bound
            g = torch.Generator(device=dev).manual_seed(0)
            pool = {"bf16": [], "fp8": []}
            for _ in range(ncopy):
                kv = [torch.randn(B, HKV, hist, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(2)]
                pool["bf16"].append(kv)
                pool["fp8"].append([llm._quantize_kv(t, sc[2 + i, 0]) for i, t in enumerate(kv)])
            q = torch.randn(B, H * D, device=dev, dtype=torch.bfloat16, generator=g)
            lens = torch.full((B,), hist, device=dev, dtype=torch.int32)
            turn = {"bf16": 0, "fp8": 0}

            def run(side, ns=None):
                turn[side] = (turn[side] + 1) % ncopy
                k, v = pool[side][turn[side]]
                return llm.attention_decode(q, k, v, lens, H, HKV, n_splits=ns, kv_scale=sc if side == "fp8" else None)

            turn.update(bf16=0, fp8=0)
            a, b = run("bf16").float(), run("fp8").float()
            default = llm.decode_splits(B, HKV, hist)
            sweep = sorted({max(1, default // 2), default, min(2 * default, max(1, hist // 128))})
            fns = [("bf16", default), *(("fp8", ns) for ns in sweep)]
            res = timed_pair([lambda s=s, ns=ns: run(s, ns) for s, ns in fns], args.rounds, args.reps)
            for (side, ns), (med, mn) in zip(fns, res):
                print(json.dumps({"part": "kvfp8", "case": f"attention_decode {side}", "B": B, "history": hist,
                                  "cache_copies": ncopy, "kv_MB": round(nbytes[side] / 2**20, 1), "n_splits": ns,
                                  "default_splits": default, "rounds": args.rounds, "reps": args.reps,
                                  "median_us": round(med, 2), "min_us": round(mn, 2),
                                  "TBps_median": round(nbytes[side] / med / 1e6, 3),
                                  "fraction_of_ceiling": round(nbytes[side] / (med * 1e-6) / CEILING, 3),
                                  "relerr_fp8_vs_bf16_cache": round(float((b - a).norm() / a.norm()), 5)}), flush=True)
            del pool
            torch.cuda.empty_cache()

    # llama3-mini: what the 8-bit cache does to the logits at scale 1 (a measurement, asserted nowhere).  Token 0 comes
    # from the prefill alone, so both runs feed the same token to step 1: its logits differ by the cache alone.
    torch.manual_seed(0)
    mini = Llama(CONFIGS["llama3-mini"], impl="hip", device=dev)
    prompts = torch.randint(0, mini.cfg.vocab_size, (3, 128), device=dev,
                            generator=torch.Generator(device=dev).manual_seed(1))
    zs = [mini.generate(prompts, [5, 128, 37], max_new_tokens=2, return_logits=True,
                        cache=KVCache(mini.cfg, 3, 130, dev, dt))[1][:, 1].float() for dt in (torch.bfloat16, fp8)]
    print(json.dumps({"part": "kvfp8", "case": "llama3-mini step-1 logits, fp8 cache vs bf16 cache (scale 1)",
                      "max_abs": round(float((zs[1] - zs[0]).abs().max()), 4),
                      "max_abs_logit": round(float(zs[0].abs().max()), 3),
                      "relerr": round(float((zs[1] - zs[0]).norm() / zs[0].norm()), 5)}), flush=True)
    del mini

    # llama3-8b, MXFP4 weights, B = 8 on a 32768-token history: the graph-replayed step per cache dtype.  The
    # history is random bytes (a step's time does not depend on the values), lens is put back before every round.
    name, B, hist = "llama3-8b", 8, 32768
    torch.manual_seed(0)
    model = Llama(CONFIGS[name], impl="hip", device=dev)
    model.quantize_weights("mxfp4", keep_bf16=False)
    cur = torch.zeros(B, device=dev, dtype=torch.int64)
    for dt in (torch.bfloat16, fp8):
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        cache = KVCache(model.cfg, B, hist, dev, dt)
        for t in cache.k + cache.v:
            t.normal_() if dt == torch.bfloat16 else t.view(torch.uint8).random_(0, 0x78)
        held = torch.cuda.memory_allocated()

        def one():
            llm.sample(model.decode_step(cur, cache), cur=cur, step=cache.step, done=cache.done, lens=cache.lens,
                       advance=True)

        cache.lens.fill_(hist - args.reps)
        one()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            one()
        ts = []
        for _ in range(args.rounds + 1):  # the first round warms up
            cache.lens.fill_(hist - args.reps)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                graph.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / args.reps)
        ts = sorted(ts[1:])
        print(json.dumps({"part": "kvfp8", "case": "graph-replayed decode step", "model": name, "weights": "mxfp4",
                          "B": B, "history": hist, "cache": str(dt).split(".")[-1], "rounds": args.rounds, "reps": args.reps,
                          "median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4),
                          "cache_GB": round((held - before) / 1e9, 2),
                          "memory_allocated_GB": round(held / 1e9, 2)}), flush=True)
        del graph, cache


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["attn", "generate", "linear", "extend", "mx", "mxrows", "kvfp8", "all"],
                    default="all")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--models", default="llama3-1b")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 1 or args.reps < 1 or args.repeats < 1 or args.new < 2:
        ap.error("--rounds, --reps and --repeats must be >= 1, --new >= 2")
    import torch

    if not torch.cuda.is_available():
        sys.exit("decode_bench: needs a HIP device (no CPU fallback: a CPU timing says nothing here)")
    if args.part in ("attn", "all"):
        attn(args)
    if args.part in ("linear", "all"):
        linear(args)
    if args.part in ("generate", "all"):
        generate(args)
    if args.part in ("extend", "all"):
        extend(args)
    if args.part in ("mx", "all"):
        mx(args)
    if args.part in ("mxrows", "all"):
        mxrows(args)
    if args.part in ("kvfp8", "all"):
        kvfp8(args)


if __name__ == "__main__":
    main()
