#!/usr/bin/env python3
"""Cost and gain of micro-batch gradient accumulation (ops/optim.py
``grad_accum_multi``, csrc/kernels/optim_kernels.hip ``k_grad_accum_multi``,
``GradBucketer(accum_steps=N)``).

``kernel``  pto_grad_accum_multi over the parameter shapes of a model
            (``--model``, ``--layers`` of it besides embedding and head), one
            launch for the whole list, per mode and gradient dtype: time and
            bytes/time, with the bytes of the kernel's table (bf16 / fp32 per
            element: INIT 2+4 / 4+4, ADD 2+4+4 / 4+4+4, FOLD 2+4+2 / 4+4+4).
            The modes of one dtype are timed interleaved.
``step``    LlamaTrainer at ``--grad-accum-steps`` N = each of ``--n``: ms per
            optimizer step, tokens/s, ``torch.cuda.max_memory_allocated`` and
            the StepTimer phases (a second, shorter run: the phase events
            cost a little).  One trainer at a time; the N are visited
            ``--rounds`` times in rotation so that no N always runs first.

One JSON line per row.

    python tools/grad_accum_bench.py kernel [--model llama3-8b] [--layers 4] [--rounds 20]
    python tools/grad_accum_bench.py step   [--model llama3-8b] [--batch-size 4] [--seq-len 4096]
                                            [--n 1,2,4,8] [--steps 4] [--warmup 2] [--rounds 2]
"""
from __future__ import annotations

import argparse
import dataclasses
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_clip_bench import CEILING, interleaved  # noqa: E402

# bytes per element: (bf16, fp32)
BYTES = {"init": (2 + 4, 4 + 4), "add": (2 + 4 + 4, 4 + 4 + 4), "fold": (2 + 4 + 2, 4 + 4 + 4)}


def model_shapes(model: str, layers: int | None):
    import torch

    if model == "resnet50":
        from pytorch_operator_1_amd.models.resnet import resnet50

        with torch.device("meta"):
            return [tuple(p.shape) for p in resnet50().parameters()]
    from pytorch_operator_1_amd.models.llama import CONFIGS, Llama

    cfg = CONFIGS[model]
    if layers is not None:
        cfg = dataclasses.replace(cfg, n_layers=layers)
    return [tuple(p.shape) for p in Llama(cfg, impl="torch", device=torch.device("meta")).parameters()]


def cmd_kernel(args):
    import torch

    from pytorch_operator_1_amd.ops.optim import grad_accum_multi

    dev = torch.device("cuda")
    shapes = model_shapes(args.model, args.layers)
    numel = sum(torch.Size(s).numel() for s in shapes)
    for dtype in (torch.bfloat16, torch.float32):
        grads = [torch.randn(s, device=dev).to(dtype) for s in shapes]
        accs = [torch.zeros(s, device=dev) for s in shapes]
        outs = [torch.empty_like(g) for g in grads]
        none = [None] * len(grads)
        recs = {"init": list(zip(grads, accs, none)), "add": list(zip(grads, accs, none)),
                "fold": list(zip(grads, accs, outs))}
        fns = {m: (lambda m=m: grad_accum_multi(recs[m], m)) for m in recs}
        for mode, (med, mn) in interleaved(fns, args.rounds).items():
            nbytes = numel * BYTES[mode][dtype == torch.float32]
            print(json.dumps({"case": f"{args.model} x{args.layers} layers" if args.layers else args.model,
                              "dtype": str(dtype).split(".")[1], "mode": mode, "tensors": len(shapes),
                              "elements": numel, "bytes": nbytes, "median_us": round(med, 1), "min_us": round(mn, 1),
                              "TBps_median": round(nbytes / med / 1e6, 3),
                              "fraction_of_ceiling": round(nbytes / (med * 1e-6) / CEILING, 3)}), flush=True)
        del grads, accs, outs, recs, fns
        torch.cuda.empty_cache()


def _timed(tr, steps: int) -> float:
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def cmd_step(args):
    import torch

    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    dev = torch.device("cuda")
    ns = [int(x) for x in args.n.split(",")]
    for r in range(args.rounds):
        for n in ns[r % len(ns):] + ns[:r % len(ns)]:
            torch.cuda.reset_peak_memory_stats()
            tr = LlamaTrainer(dev, model=args.model, batch_size=args.batch_size, seq_len=args.seq_len,
                              checkpoint=args.activation_checkpoint, max_grad_norm=args.max_grad_norm,
                              grad_accum_steps=n)
            tr.run(args.warmup)
            sec = _timed(tr, args.steps)
            peak = torch.cuda.max_memory_allocated()
            tr.timer.enabled = True
            tr.run(max(1, args.steps // 2))
            phases = tr.timer.summary()  # mean per ENTRY: forward/backward/allreduce_wait are entered N times a step
            print(json.dumps({"model": args.model, "round": r, "grad_accum_steps": n,
                              "tokens_per_micro_batch": args.batch_size * args.seq_len,
                              "tokens_per_step": tr.samples_per_step(), "ms_per_step": round(sec * 1e3, 2),
                              "tokens_per_s": round(tr.samples_per_step() / sec, 1),
                              "peak_allocated_GB": round(peak / 1e9, 2),
                              "accum_GB": round(tr.bucketer.accum_bytes() / 1e9, 2), "loss": tr.last_loss(),
                              "phase_ms_per_entry": phases}), flush=True)
            tr.bucketer.remove()
            del tr
            gc.collect()
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernel", "step"])
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-tiny", "llama3-1b", "llama3-8b", "resnet50"])
    ap.add_argument("--layers", type=int, default=4,
                    help="kernel: layers of the Llama besides embedding and head (0: all of them)")
    ap.add_argument("--rounds", type=int, default=None, help="default: 20 (kernel), 2 (step)")
    ap.add_argument("--batch-size", type=int, default=4, help="step: rows per micro-batch")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--n", default="1,2,4,8", help="step: the grad_accum_steps to visit")
    ap.add_argument("--steps", type=int, default=4, help="step: timed optimizer steps per visit")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--activation-checkpoint", choices=["none", "full"], default="none")
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    args = ap.parse_args()
    if args.layers == 0 or args.model == "resnet50":
        args.layers = None
    if args.rounds is None:
        args.rounds = 20 if args.mode == "kernel" else 2
    {"kernel": cmd_kernel, "step": cmd_step}[args.mode](args)


if __name__ == "__main__":
    main()
