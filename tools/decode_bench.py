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
``--prompt``-token prompt, B in {1, 8}, eager against ``graph=True``; host
clock around a call that ends in a device synchronise, the prefill (a call
with one new token) timed the same way and subtracted for the decode rate.

One JSON line per row.

    python tools/decode_bench.py [--part attn|generate|all] [--rounds 15] [--reps 20]
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

            def run(n_new, graph):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(prompts, max_new_tokens=n_new, graph=graph)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            outs = {}
            for graph in (False, True):  # warm every path: code objects, the library's picks, the rope tables
                run(args.new, graph)
            run(1, False)
            t = {"prefill": [], False: [], True: []}
            for _ in range(args.repeats):
                t["prefill"].append(run(1, False)[0])
                for graph in (False, True):
                    dt, outs[graph] = run(args.new, graph)
                    t[graph].append(dt)
            pre = sorted(t["prefill"])[len(t["prefill"]) // 2]
            for graph in (False, True):
                ts = sorted(t[graph])
                med = ts[len(ts) // 2]
                print(json.dumps({"case": "generate graph" if graph else "generate eager", "model": name, "B": B,
                                  "prompt": args.prompt, "new_tokens": args.new, "repeats": args.repeats,
                                  "median_ms": round(med * 1e3, 2), "min_ms": round(ts[0] * 1e3, 2),
                                  "prefill_ms": round(pre * 1e3, 2),
                                  "decode_ms_per_step": round((med - pre) / (args.new - 1) * 1e3, 4),
                                  "decode_tokens_per_s": round(B * (args.new - 1) / (med - pre), 1),
                                  "tokens_per_s_with_prefill": round(B * args.new / med, 1),
                                  "graph_equals_eager": bool(torch.equal(outs[False], outs[True]))}), flush=True)
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["attn", "generate", "all"], default="all")
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
    if args.part in ("generate", "all"):
        generate(args)


if __name__ == "__main__":
    main()
