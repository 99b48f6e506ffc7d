#!/usr/bin/env python3
"""Cost of the held-out evaluation of the Llama trainer (profiles/lm_eval.md).

``--part kernels``: ``pto_ce_eval`` + ``pto_eval_accum`` (per-row NLL and
label rank, then the fp64 record) against ``pto_ce_fwd`` on the same bf16
logits ``[4096, 128256]`` (1.05 GB).  Both read every logit once (2
B/element), so the expectation is parity.  ``pto_ce_fwd`` is timed as two
sides, so the difference between them is the run-to-run spread the eval
pair is judged against.  All sides interleaved in one process, the order
rotated, HIP events; median and min over ``--rounds``.

``--part trainer``: wall time (host clock around a call that ends in the
record's device-to-host read) and peak device memory above what the trainer
holds at rest of one ``LlamaTrainer.evaluate(batches=1)``, ``head_chunk``
2048 against ``None`` (the whole ``[B*S, V]`` logits at once), alternated.

One JSON line per row.

    python tools/lm_eval_bench.py [--part kernels|trainer|all] [--rounds 30] [--rows 4096] [--vocab 128256]
                                  [--model llama3-1b] [--seq-len 4096] [--batch-size 2] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ce_bench import CEILING, interleaved  # noqa: E402  (tools/ce_bench.py)


def kernels(args):
    import torch

    from pytorch_operator_1_amd.ops import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    M, V = args.rows, args.vocab
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.empty(M, V, device=dev, dtype=torch.bfloat16)
    for rows in src.split(1024):  # 3 * randn in bf16 without an fp32 tensor of the full shape
        rows.copy_(3 * torch.randn(rows.shape, device=dev, generator=g))
    labels = torch.randint(0, V, (M,), device=dev, generator=g)
    labels[5] = -100
    lse = torch.empty(M, device=dev, dtype=torch.float32)
    loss = torch.empty(M, device=dev, dtype=torch.float32)
    row_loss = torch.empty(M, device=dev, dtype=torch.float32)
    row_rank = torch.empty(M, device=dev, dtype=torch.int32)
    acc = torch.zeros(5, device=dev, dtype=torch.float64)

    def fwd():
        _lib.check(L.pto_ce_fwd(src.data_ptr(), labels.data_ptr(), lse.data_ptr(), loss.data_ptr(), M, V, -100,
                                _lib.stream_ptr()), "ce_fwd")

    def ev():
        _lib.check(L.pto_ce_eval(src.data_ptr(), labels.data_ptr(), row_loss.data_ptr(), row_rank.data_ptr(), M, V,
                                 -100, _lib.stream_ptr()), "ce_eval")

    def pair():
        ev()
        _lib.check(L.pto_eval_accum(row_loss.data_ptr(), row_rank.data_ptr(), M, 5, acc.data_ptr(),
                                    _lib.stream_ptr()), "eval_accum")

    # the two kernels must agree on the row losses they both compute
    fwd()
    pair()
    same = float((row_loss - loss).abs().max())
    nbytes = 2 * M * V
    sides = {"ce_fwd (a)": fwd, "ce_eval + eval_accum": pair, "ce_fwd (b)": fwd, "ce_eval alone": ev}
    for name, (med, mn) in interleaved(sides, args.rounds).items():
        print(json.dumps({"case": name, "rows": M, "vocab": V, "bytes": nbytes, "rounds": args.rounds,
                          "median_us": round(med, 1), "min_us": round(mn, 1),
                          "TBps_median": round(nbytes / med / 1e6, 3),
                          "fraction_of_ceiling": round(nbytes / (med * 1e-6) / CEILING, 3),
                          "max_abs_row_loss_diff_vs_ce_fwd": same}), flush=True)


def trainer(args):
    import torch

    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    dev = torch.device("cuda")
    tr = LlamaTrainer(dev, model=args.model, batch_size=args.batch_size, seq_len=args.seq_len)
    chunks = (2048, None)
    for hc in chunks:  # warm every shape: code objects, the library's algorithm picks, the held-out batch
        tr.evaluate(batches=1, head_chunk=hc)
    torch.cuda.synchronize()
    rest = torch.cuda.memory_allocated()
    times = {hc: [] for hc in chunks}
    peak = {hc: 0 for hc in chunks}
    res = {}
    for _ in range(args.repeats):
        for hc in chunks:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            res[hc] = tr.evaluate(batches=1, head_chunk=hc)  # result() reads the record: the work is finished
            times[hc].append(time.perf_counter() - t0)
            peak[hc] = max(peak[hc], torch.cuda.max_memory_allocated() - rest)
    for hc in chunks:
        t = sorted(times[hc])
        print(json.dumps({"case": f"evaluate(batches=1, head_chunk={hc})", "model": args.model,
                          "tokens": res[hc]["tokens"], "repeats": args.repeats,
                          "median_ms": round(t[len(t) // 2] * 1e3, 2), "min_ms": round(t[0] * 1e3, 2),
                          "max_ms": round(t[-1] * 1e3, 2), "peak_MB_above_rest": round(peak[hc] / 2**20, 1),
                          "rest_MB": round(rest / 2**20, 1), "loss": res[hc]["loss"], "top1": res[hc]["top1"],
                          "topk": res[hc]["topk"]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["kernels", "trainer", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--model", default="llama3-1b")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.rounds < 1 or args.repeats < 1:
        ap.error("--rounds and --repeats must be >= 1")
    import torch

    if not torch.cuda.is_available():
        sys.exit("lm_eval_bench: needs a HIP device (no CPU fallback: a CPU timing says nothing here)")
    if args.part in ("kernels", "all"):
        kernels(args)
    if args.part in ("trainer", "all"):
        trainer(args)


if __name__ == "__main__":
    main()
