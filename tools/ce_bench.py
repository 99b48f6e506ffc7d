#!/usr/bin/env python3
"""Cost of label smoothing and z-loss inside the vocab-wide cross entropy
(csrc/kernels/llm_kernels.hip), at the Llama-3-8B step's shape: bf16 logits
``[16384, 128256]`` (4.2 GB).

Sides, forward and backward each:

``plain (this)``      pto_ce_fwd / pto_ce_bwd of this tree's library
``ex (this)``         pto_ce_fwd_ex / pto_ce_bwd_ex, label_smoothing 0.1, z_loss 1e-4
``plain (baseline)``  with ``--baseline-lib`` (a library built from another
                      commit): that library's pto_ce_fwd / pto_ce_bwd

All sides are timed interleaved in one process (one launch of each per round,
the order rotated, HIP events); median and min over ``--rounds``.  The forward
reads the logits once (2 B/element), the backward reads them and writes the
gradient in place (4 B/element); bytes/time is given against the 6.29 TB/s
streaming ceiling (float4 copy) of the MI355X.  The backward overwrites its
input, so every timed launch is preceded, outside the events, by a copy of
the logits into the working buffer.  The plain sides' outputs are compared
bit for bit.  One JSON line per row.

    python tools/ce_bench.py [--rounds 20] [--rows 16384] [--vocab 128256] [--baseline-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CEILING = 6.29e12  # bytes/s, measured float4 copy (profiles/grad_clip.md)
SMOOTHING, Z_COEF = 0.1, 1e-4


def interleaved(fns: dict, rounds: int, before=None):
    """{name: (median, min)} microseconds, one launch of each per round, the
    order rotated from round to round; ``before`` runs ahead of every launch,
    outside the timed events."""
    import torch

    for _ in range(3):
        for fn in fns.values():
            if before:
                before()
            fn()
    times = {k: [] for k in fns}
    order = list(fns.items())
    for r in range(rounds):
        for k, fn in order[r % len(order):] + order[:r % len(order)]:  # no side always follows the same one
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    if args.rounds < 1:
        ap.error("--rounds must be >= 1")

    import torch

    from pytorch_operator_1_amd.ops import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    M, V = args.rows, args.vocab
    plain = {"this": L}
    if args.baseline_lib:
        B = ctypes.CDLL(args.baseline_lib)
        for name in ("pto_ce_fwd", "pto_ce_bwd"):
            getattr(B, name).argtypes = _lib._SIGS[name]
        plain["baseline"] = B

    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.empty(M, V, device=dev, dtype=torch.bfloat16)
    for rows in src.split(1024):  # 3 * randn in bf16 without an fp32 tensor of the full shape
        rows.copy_(3 * torch.randn(rows.shape, device=dev, generator=g))
    labels = torch.randint(0, V, (M,), device=dev, generator=g)
    labels[5] = -100
    work = torch.empty_like(src)
    lse = torch.empty(M, device=dev, dtype=torch.float32)
    rows_out = torch.empty(M, device=dev, dtype=torch.float32)
    scale = torch.full((1,), 1.0 / (M - 1), device=dev, dtype=torch.float32)

    def fwd(fn, *ex):
        return lambda: _lib.check(fn(src.data_ptr(), labels.data_ptr(), lse.data_ptr(), rows_out.data_ptr(), M, V,
                                     -100, *ex, _lib.stream_ptr()), "ce_fwd")

    def bwd(fn, *ex):
        return lambda: _lib.check(fn(work.data_ptr(), labels.data_ptr(), lse.data_ptr(), scale.data_ptr(), M, V,
                                     -100, *ex, _lib.stream_ptr()), "ce_bwd")

    fwds = {f"fwd plain ({k})": fwd(lib.pto_ce_fwd) for k, lib in plain.items()}
    fwds["fwd ex (this)"] = fwd(L.pto_ce_fwd_ex, SMOOTHING, Z_COEF)
    bwds = {f"bwd plain ({k})": bwd(lib.pto_ce_bwd) for k, lib in plain.items()}
    bwds["bwd ex (this)"] = bwd(L.pto_ce_bwd_ex, SMOOTHING, Z_COEF)

    # results must not change: the plain sides bit for bit
    same = None
    if args.baseline_lib:
        outs = []
        for k in plain:
            lse.fill_(float("nan"))
            fwds[f"fwd plain ({k})"]()
            work.copy_(src)
            bwds[f"bwd plain ({k})"]()
            outs.append((lse.clone(), rows_out.clone(), work.clone()))
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        del outs
    fwds["fwd plain (this)"]()  # the backward sides read this lse

    for fns, nbytes, before in ((fwds, 2 * M * V, None), (bwds, 4 * M * V, lambda: work.copy_(src))):
        for name, (med, mn) in interleaved(fns, args.rounds, before).items():
            rec = {"case": name, "rows": M, "vocab": V, "bytes": nbytes, "rounds": args.rounds,
                   "median_us": round(med, 1), "min_us": round(mn, 1), "TBps_median": round(nbytes / med / 1e6, 3),
                   "fraction_of_ceiling": round(nbytes / (med * 1e-6) / CEILING, 3)}
            if same is not None and "plain" in name:
                rec["plain_outputs_bit_equal"] = same
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
