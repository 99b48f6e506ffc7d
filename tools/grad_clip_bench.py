#!/usr/bin/env python3
"""Cost of device-side global-norm gradient clipping (ops/optim.py,
csrc/kernels/optim_kernels.hip), on synthetic tensors of the models' shapes.

``norm``   stage 1 + stage 2 (pto_grad_sqnorm_multi + pto_grad_norm_finalize)
           over the gradient set of Llama-3-8B (bf16, 16 GB) and of ResNet-50
           (fp32, 102 MB): time and bytes/time against the 6.29 TB/s streaming
           ceiling (float4 copy) of the MI355X.
``optim``  the optimizer launch: pto_adamw_multi (null coefficient pointer)
           against pto_adamw_multi_clip reading a coefficient of 1.0, on
           ``--layers`` Llama-3-8B layers plus embedding and head; the same
           for pto_sgd_multi on ResNet-50.  With ``--baseline-lib`` (a
           library built from another commit) that library's pto_adamw_multi /
           pto_sgd_multi is a third side in the same process.

All sides of a comparison are timed interleaved (one launch of each per
round, HIP events); median and min over ``--rounds``.  One JSON line per row.

    python tools/grad_clip_bench.py norm  [--rounds 20]
    python tools/grad_clip_bench.py optim [--rounds 20] [--layers 2] [--baseline-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CEILING = 6.29e12  # bytes/s, measured float4 copy


def llama_numels(layers=None):
    import torch

    from pytorch_operator_1_amd.models.llama import CONFIGS, Llama

    cfg = CONFIGS["llama3-8b"]
    if layers is not None:
        import dataclasses

        cfg = dataclasses.replace(cfg, n_layers=layers)
    return [p.numel() for p in Llama(cfg, impl="torch", device=torch.device("meta")).parameters()]


def resnet_numels():
    import torch

    from pytorch_operator_1_amd.models.resnet import resnet50

    with torch.device("meta"):
        return [p.numel() for p in resnet50().parameters()]


def interleaved(fns: dict, rounds: int):
    """{name: (median, min)} microseconds, one launch of each per round,
    the order rotated from round to round."""
    import torch

    for _ in range(3):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    order = list(fns.items())
    for r in range(rounds):
        for k, fn in order[r % len(order):] + order[:r % len(order)]:  # no side always follows the same one
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def _table(struct, recs, dev):
    import torch

    raw = (struct * len(recs))(*recs)
    host = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(raw), ctypes.sizeof(raw))), dtype=torch.uint8)
    return host.to(dev)


def norm_case(L, numels, dtype, dev):
    """Closure running stage 1 + stage 2 over fresh random gradients, and the bytes it reads."""
    import torch

    from pytorch_operator_1_amd.ops import _lib
    from pytorch_operator_1_amd.ops.optim import _AdamTensor

    grads = [torch.randn(n, device=dev, dtype=dtype) for n in numels]
    table = _table(_AdamTensor, [_AdamTensor(0, g.data_ptr(), 0, 0, 0, g.numel()) for g in grads], dev)
    cs = [0]
    for n in numels:
        cs.append(cs[-1] + L.pto_grad_sqnorm_chunks(n))
    nb = L.pto_grad_sqnorm_blocks(cs[-1])
    cs_dev = torch.tensor(cs, dtype=torch.int32, device=dev)
    partials = torch.empty(nb, dtype=torch.float32, device=dev)
    rec = torch.zeros(2, dtype=torch.float32, device=dev)
    bf16 = int(dtype == torch.bfloat16)

    def run():
        s = _lib.stream_ptr()
        _lib.check(L.pto_grad_sqnorm_multi(table.data_ptr(), ctypes.sizeof(_AdamTensor), cs_dev.data_ptr(),
                                           len(numels), bf16, partials.data_ptr(), nb, s), "sqnorm")
        _lib.check(L.pto_grad_norm_finalize(partials.data_ptr(), nb, 1.0, 1.0, rec.data_ptr(), s), "finalize")

    run.keep = (grads, table, cs_dev, partials, rec)
    run.rec = rec
    run.ref = lambda: float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    return run, sum(numels) * grads[0].element_size(), nb


def cmd_norm(args):
    import torch

    from pytorch_operator_1_amd.ops import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    cases = {"llama3-8b bf16": (llama_numels(), torch.bfloat16), "resnet50 fp32": (resnet_numels(), torch.float32)}
    runs, meta = {}, {}
    for name, (numels, dtype) in cases.items():
        runs[name], nbytes, nb = norm_case(L, numels, dtype, dev)
        meta[name] = (nbytes, nb, len(numels))
    res = interleaved(runs, args.rounds)
    for name, (med, mn) in res.items():
        nbytes, nb, nt = meta[name]
        got, ref = float(runs[name].rec[0]), runs[name].ref()
        print(json.dumps({"case": name, "tensors": nt, "bytes": nbytes, "partials": nb, "median_us": round(med, 1),
                          "min_us": round(mn, 1), "TBps_median": round(nbytes / med / 1e6, 3),
                          "fraction_of_ceiling": round(nbytes / (med * 1e-6) / CEILING, 3),
                          "norm_relerr_vs_fp64": abs(got - ref) / ref}), flush=True)


def cmd_optim(args):
    import torch

    from pytorch_operator_1_amd.ops import _lib
    from pytorch_operator_1_amd.ops.optim import _AdamTensor, _SgdTensor

    L, dev = _lib.lib(), torch.device("cuda")
    libs = {"this": L}
    if args.baseline_lib:
        B = ctypes.CDLL(args.baseline_lib)
        for name in ("pto_adamw_multi", "pto_sgd_multi"):
            getattr(B, name).argtypes = _lib._SIGS[name]
        libs["baseline"] = B
    one = torch.ones(1, dtype=torch.float32, device=dev)

    # AdamW, mixed precision
    numels = llama_numels(args.layers)
    recs, starts, nb, keep = [], [], 0, []
    for n in numels:
        p = torch.randn(n, device=dev).mul_(0.02).bfloat16()
        g = torch.randn(n, device=dev).bfloat16()
        w, m, v = p.float(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        keep.append((p, g, w, m, v))
        recs.append(_AdamTensor(p.data_ptr(), g.data_ptr(), w.data_ptr(), m.data_ptr(), v.data_ptr(), n))
        starts.append(nb)
        nb += L.pto_adamw_block_count(n)
    table, st = _table(_AdamTensor, recs, dev), torch.tensor(starts, dtype=torch.int32, device=dev)
    hyper = (None, 3e-4, 0.9, 0.95, 1e-8, 0.1, 10, 1.0)

    def adam(lib):
        return lambda: _lib.check(lib.pto_adamw_multi(table.data_ptr(), st.data_ptr(), len(recs), nb, 1, *hyper, 0,
                                                      _lib.stream_ptr()), "adamw")

    fns = {f"adamw_multi ({k})": adam(lib) for k, lib in libs.items()}
    fns["adamw_multi_clip (coef ptr)"] = lambda: _lib.check(
        L.pto_adamw_multi_clip(table.data_ptr(), st.data_ptr(), len(recs), nb, 1, *hyper, one.data_ptr(), 0,
                               _lib.stream_ptr()), "adamw_clip")
    nbytes = sum(numels) * 28  # read g, master, m, v; write p, master, m, v
    for name, (med, mn) in interleaved(fns, args.rounds).items():
        print(json.dumps({"case": name, "params": sum(numels), "median_us": round(med, 1), "min_us": round(mn, 1),
                          "TBps_median": round(nbytes / med / 1e6, 3)}), flush=True)
    del keep, table, st
    torch.cuda.empty_cache()

    # SGD momentum, fp32
    numels = resnet_numels()
    recs, starts, nb, keep = [], [], 0, []
    for n in numels:
        p, g, m = torch.randn(n, device=dev), torch.randn(n, device=dev), torch.zeros(n, device=dev)
        keep.append((p, g, m))
        recs.append(_SgdTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), n))
        starts.append(nb)
        nb += L.pto_sgd_block_count(n)
    table, st = _table(_SgdTensor, recs, dev), torch.tensor(starts, dtype=torch.int32, device=dev)

    def sgd(lib):
        return lambda: _lib.check(lib.pto_sgd_multi(table.data_ptr(), st.data_ptr(), len(recs), nb, None, 1e-3, 0.9,
                                                    1e-4, 1.0, 0, 0, None, 1, _lib.stream_ptr()), "sgd")

    fns = {f"sgd_multi ({k})": sgd(lib) for k, lib in libs.items()}
    fns["sgd_multi_clip (coef ptr)"] = lambda: _lib.check(
        L.pto_sgd_multi_clip(table.data_ptr(), st.data_ptr(), len(recs), nb, None, 1e-3, 0.9, 1e-4, 1.0,
                             one.data_ptr(), 0, 0, None, 1, _lib.stream_ptr()), "sgd_clip")
    for name, (med, mn) in interleaved(fns, args.rounds).items():
        print(json.dumps({"case": name, "params": sum(numels), "median_us": round(med, 1), "min_us": round(mn, 1)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["norm", "optim"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--layers", type=int, default=2, help="optim: Llama-3-8B layers besides embedding and head")
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    {"norm": cmd_norm, "optim": cmd_optim}[args.mode](args)


if __name__ == "__main__":
    main()
