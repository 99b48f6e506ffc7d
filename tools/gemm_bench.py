#!/usr/bin/env python3
"""The linear layers of Llama-3-8B at 16,384 tokens: the package's bf16 MFMA
GEMM (ops/gemm.py) against what the training step runs today -- the library
GEMM (hipBLASLt through torch) PLUS the transposes it needs:

* fwd    ``F.linear(x, w)``                              vs ``gemm_nt(x, w)``
* dgrad  ``F.linear(dy, wt)`` + this weight's share of ``refresh_transposed``
         (one ``transpose_into(w, wt)`` per step)        vs ``gemm_nn(dy, w)``
         (``lib_plain``: ``dy.mm(w)``, today's PTO_WT=0 path, for reference)
* wgrad  wo, w13 (``dw_kcontig``): ``transpose_into(x)`` [+ ``transpose_into(dy)``
         for wo; w13 gets dY^T from the SwiGLU backward, not charged here] +
         ``dyt.mm(xt.t())``; the others ``dy.t().mm(x)``  vs ``gemm_tn(dy, x)``

The two sides are timed interleaved (one launch of each per repeat), median
of HIP-event times; the whole table is taken ``--runs`` times.  One JSON line
per (family, kind, run).

    python tools/gemm_bench.py [--tokens 16384] [--reps 10] [--runs 2] [--out profiles/raw/gemm_bf16.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# family: (k_in, n_out, weight gradient from transposed activations today)
FAMILIES = {"wqkv": (4096, 6144, False), "wo": (4096, 4096, True), "w13": (4096, 28672, True),
            "w2": (14336, 4096, False), "lm_head": (4096, 128256, False)}
KINDS = ("fwd", "dgrad", "wgrad")


def timed_pair(fa, fb, reps):
    """Median microseconds of ``fa`` and of ``fb``, one launch of each per
    repeat, alternating."""
    import torch

    for _ in range(2):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    ta.sort()
    tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2]


def relerr(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm())


def main():
    import torch
    import torch.nn.functional as F

    from pytorch_operator_1_amd.ops import gemm, llm

    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--families", default="", help="only these, comma-separated")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    T = a.tokens
    want = [f for f in a.families.split(",") if f] or list(FAMILIES)
    sink = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for run in range(a.runs):
        for fam in want:
            k_in, n_out, kcontig = FAMILIES[fam]
            torch.manual_seed(1)
            x =torch.randn(T, k_in, device=dev).bfloat16()
            w = (torch.randn(n_out, k_in, device=dev) * 0.02).bfloat16()
            flops = 2.0 * T * k_in * n_out
            for kind in KINDS:
                if kind == "fwd":
                    y = torch.empty(T, n_out, device=dev, dtype=torch.bfloat16)
                    lib = lambda: F.linear(x, w)  # noqa: E731
                    own = lambda: gemm.gemm_nt(x, w, out=y)  # noqa: E731
                    extra = {}
                elif kind == "dgrad":
                    dy = torch.randn(T, n_out, device=dev).bfloat16()
                    wt = torch.empty(k_in, n_out, device=dev, dtype=torch.bfloat16)
                    llm.transpose_into(w, wt)
                    dx = torch.empty(T, k_in, device=dev, dtype=torch.bfloat16)

                    def lib():
                        llm.transpose_into(w, wt)  # this weight's share of refresh_transposed
                        return F.linear(dy, wt)

                    own = lambda: gemm.gemm_nn(dy, w, out=dx)  # noqa: E731
                    t_plain, t_gemm = timed_pair(lambda: dy.mm(w), lambda: F.linear(dy, wt), a.reps)
                    extra = {"lib_plain_us": round(t_plain, 1), "lib_gemm_only_us": round(t_gemm, 1)}
                else:
                    dy = torch.randn(T, n_out, device=dev).bfloat16()
                    dw = torch.empty(n_out, k_in, device=dev, dtype=torch.bfloat16)
                    if kcontig:
                        xt = torch.empty(k_in, T, device=dev, dtype=torch.bfloat16)
                        dyt = torch.empty(n_out, T, device=dev, dtype=torch.bfloat16)
                        llm.transpose_into(dy, dyt)

                        def lib():
                            llm.transpose_into(x, xt)
                            if fam != "w13":  # w13's dY^T is written by the SwiGLU backward
                                llm.transpose_into(dy, dyt)
                            return dyt.mm(xt.t())
                    else:
                        lib = lambda: dy.t().mm(x)  # noqa: E731
                    own = lambda: gemm.gemm_tn(dy, x, out=dw)  # noqa: E731
                    t_plain, _ = timed_pair(lambda: dy.t().mm(x), lambda: None, a.reps)
                    extra = {"lib_plain_us": round(t_plain, 1)}
                err = relerr(own(), lib())
                t_own, t_lib = timed_pair(own, lib, a.reps)
                emit({"family": fam, "kind": kind, "run": run, "tokens": T, "k_in": k_in, "n_out": n_out,
                      "own_us": round(t_own, 1), "lib_us": round(t_lib, 1), "own_tflops": round(flops / t_own / 1e6, 1),
                      "lib_tflops": round(flops / t_lib / 1e6, 1), "own_wins": t_own < t_lib,
                      "relerr_vs_lib": err, **extra})
                del lib, own
                if kind != "fwd":
                    del dy
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
