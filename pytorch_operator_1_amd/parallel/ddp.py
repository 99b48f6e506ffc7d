"""Bucketed gradient all-reduce overlapped with backward, for the large
DDP configs (ResNet-50, Llama-3-8B).

Reference parity: the reference workload wraps its model in
``nn.parallel.DistributedDataParallel`` (``examples/mnist/mnist.py:130-134``)
and relies on its bucketing.  This is the MI355X-first replacement:

* Gradients live in ONE flat buffer per dtype, laid out in reverse
  registration order (the order backward produces them), and every
  ``param.grad`` is a view into it: autograd accumulates straight into the
  bucket, there is no copy-in/copy-out as in stock DDP buckets.
* A ``post_accumulate_grad`` hook counts ready params per bucket; a full
  bucket is all-reduced (SUM) at once on a dedicated comm stream after an
  event on the compute stream, so RCCL runs over xGMI while backward keeps
  computing the earlier layers.
* The 1/world average is NOT a separate pass: the fused optimizers take
  ``grad_scale`` and fold it into their single read of the gradient
  (:meth:`grad_scale`), and zero the buffer in the same pass.
* Bucket size: at most 256 MB (xGMI is point-to-point, 7 links x ~150
  GB/s per GPU; a ring all-reduce on 8 GPUs moves 2*(7/8)*size per GPU, so
  large buckets amortise the per-collective latency of ~30-50 us and still
  leave >60 buckets to overlap with Llama-8B's 16 GB of bf16 gradients),
  and at most a quarter of the model (>= 4 buckets, so a small model such
  as ResNet-50 -- 51 MB of bf16 gradients -- overlaps too), never below
  4 MB.
* Comm hook: when the whole gradient buffer is small
  (<= ``PTO_XGMI_MAX_MB``, 512 MB), it is registered with the xGMI peer
  all-reduce kernel (:mod:`.xgmi`, fp32 or bf16), verified against the
  group's all-reduce, and buckets are timed both ways at startup; a
  bucket goes to the kernel if it was faster there (the decision is
  recorded in :attr:`GradBucketer.comm_info`).  The timing is bounded: one
  bucket per power-of-two size class is timed, at most
  ``PTO_XGMI_TUNE_CLASSES`` (4) classes, and every other bucket takes the
  decision of the nearest timed class (:func:`plan_bucket_timing`), so the
  startup cost does not grow with the bucket count; the seconds spent are
  recorded (``comm_info["xgmi_tune_s"]``).
"""
from __future__ import annotations

import os
import time

import torch
import torch.distributed as dist


def plan_bucket_timing(sizes: list[int], max_classes: int = 4) -> list[int]:
    """Which bucket's timing decides each bucket: ``plan[i] = j`` means
    bucket ``i`` takes the xGMI-vs-RCCL decision measured on bucket ``j``
    (``plan[j] == j`` for the timed ones).  Buckets are grouped by
    power-of-two size class; the first bucket of each class is timed, for at
    most ``max_classes`` classes chosen largest first (the large buckets
    carry the bytes); a bucket of an untimed class follows the timed class
    nearest in size.  Deterministic in ``sizes``, so every rank makes the
    same plan (the timing itself is a collective)."""
    cls = [max(1, int(n)).bit_length() for n in sizes]
    first: dict[int, int] = {}
    for i, c in enumerate(cls):
        first.setdefault(c, i)
    timed = sorted(first, reverse=True)[:max(1, max_classes)]
    plan = []
    for c in cls:
        best = min(timed, key=lambda t: (abs(t - c), -t))
        plan.append(first[best])
    return plan


class GradBucketer:
    """Modes (``mode=None`` picks ``copy`` for world > 1, ``none`` for 1):

    * ``view`` — every ``param.grad`` is a persistent view of the flat
      buffer; autograd ACCUMULATES into it (read+read+write), so the
      optimizer must zero it (``zero_grad=True`` in the fused step).
    * ``copy`` — autograd hands each gradient over as a fresh tensor
      (``grad is None`` before backward, so AccumulateGrad steals it with no
      add); the hook copies it into its bucket slot (read+write) and points
      ``param.grad`` at the slot; buckets all-reduce from the slots.
    * ``none`` — single process: no buckets, gradients stay the tensors
      autograd produced (zero extra passes).
    After the optimizer step call :meth:`release` (``copy``/``none``).

    ``accum_steps=N > 1`` (``copy``/``none``): one optimizer step over N
    micro-batches.  :meth:`finish` is called after every backward; the first
    N-1 calls sum the fresh gradients into fp32 accumulators (one per
    parameter, the parameter's layout) with
    :func:`..ops.optim.grad_accum_multi`, issue no collective, wait on
    nothing and leave every ``param.grad`` ``None``.  The N-th
    (:attr:`at_boundary`) folds accumulators plus fresh gradients, rounded
    once to the gradient dtype, into what it would otherwise have copied (the
    bucket slots, or autograd's tensors in place), and the all-reduce runs as
    with N = 1.  The first micro-batch overwrites the accumulators, so they
    are never zeroed and are dead between optimizer steps.
    """

    def __init__(self, module: torch.nn.Module, bucket_mb: float | None = None, process_group=None,
                 overlap: bool = True, mode: str | None = None, comm: str | None = None, force_ddp: bool = False,
                 accum_steps: int = 1):
        """``comm``: "auto" (default, ``PTO_COMM``): per-bucket xGMI kernel
        vs RCCL by measurement; "xgmi": every bucket on the kernel; "rccl":
        never the kernel.  ``force_ddp``: the multi-rank machinery (flat
        buckets, copy mode, comm stream, per-bucket collectives over the
        process group, xGMI hook) even in a group of one rank -- the DDP
        code path's cost measured on one GPU."""
        self.module = module
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.ddp = self.world > 1 or force_ddp
        if force_ddp and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("GradBucketer(force_ddp=True) needs a process group (a 1-rank group is fine)")
        self.overlap = overlap and self.ddp
        self.mode = mode or os.environ.get("PTO_GRAD_MODE") or ("copy" if self.ddp else "none")
        if self.mode not in ("view", "copy", "none"):
            raise ValueError(f"GradBucketer: unknown mode {self.mode}")
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError(f"GradBucketer: accum_steps must be >= 1, got {accum_steps}")
        if self.accum_steps > 1 and self.mode == "view":
            raise ValueError("GradBucketer: accum_steps > 1 is not supported in mode 'view' (autograd already adds "
                             "into the flat buffer there, in the gradient's dtype); use mode 'copy'")
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError("GradBucketer: module has no trainable parameters")
        if bucket_mb is None and "PTO_BUCKET_MB" in os.environ:
            bucket_mb = float(os.environ["PTO_BUCKET_MB"])
        if bucket_mb is None:
            total_bytes = sum(p.numel() * p.element_size() for p in params)
            cap = int(min(256 * 2**20, max(4 * 2**20, total_bytes / 4)))
        else:
            cap = int(bucket_mb * 1024 * 1024)
        self.params = params
        dev = params[0].device
        self._views: dict = {}
        # one flat buffer per dtype, reverse registration order
        self.flat: dict[torch.dtype, torch.Tensor] = {}
        self.buckets: list[dict] = []
        by_dtype: dict[torch.dtype, list] = {}
        for p in reversed(params):
            by_dtype.setdefault(p.dtype, []).append(p)
        for dt, ps in by_dtype.items():
            align = max(1, 256 // torch.empty((), dtype=dt).element_size())  # 256-byte aligned views
            offs, total = [], 0
            for p in ps:
                offs.append(total)
                total += (p.numel() + align - 1) // align * align
            if self.mode == "none":
                continue
            buf = torch.zeros(total, dtype=dt, device=dev)
            self.flat[dt] = buf
            cur, start = [], 0
            for j, (p, o) in enumerate(zip(ps, offs)):
                # same strides as the param (channels_last convs stay NHWC)
                self._views[p] = buf[o:o + p.numel()].as_strided(p.shape, p.stride())
                p.grad = self._views[p] if self.mode == "view" else None
                cur.append(p)
                end = offs[j + 1] if j + 1 < len(ps) else total  # include alignment padding
                if (end - start) * buf.element_size() >= cap or j + 1 == len(ps):
                    self.buckets.append(dict(params=cur, dtype=dt, lo=start, hi=end))
                    cur, start = [], end
        # fp32 running sums of the micro-batch gradients (accum_steps > 1 only)
        self._acc = {p: torch.empty_like(p, dtype=torch.float32) for p in params} if self.accum_steps > 1 else {}
        self._micro = 0  # finish() calls modulo accum_steps
        self._bucket_of = {}
        for i, b in enumerate(self.buckets):
            for p in b["params"]:
                self._bucket_of[p] = i
        self._pending = [0] * len(self.buckets)
        self._works: list = []
        self.comm_stream = torch.cuda.Stream(dev) if (self.overlap and dev.type == "cuda") else None
        self._handles = []
        if self.mode == "copy" or (self.overlap and self.mode == "view"):
            for p in params:
                self._handles.append(p.register_post_accumulate_grad_hook(self._on_grad))
        self._xgmi: dict = {}
        self.comm_info: dict = {"buckets": len(self.buckets), "bucket_bytes": cap, "transport": "rccl"}
        comm = comm or os.environ.get("PTO_COMM", "auto")
        if comm not in ("auto", "xgmi", "rccl"):
            raise ValueError(f"GradBucketer: comm must be auto, xgmi or rccl, not {comm!r}")
        if self.ddp and comm != "rccl" and dev.type == "cuda":
            self._setup_xgmi(comm)
        self.reset()

    def _setup_xgmi(self, comm: str):
        """Register each flat buffer with the xGMI kernel (if small enough),
        verify it, and route the buckets it runs faster."""
        from .xgmi import XgmiAllReduce

        limit = float(os.environ.get("PTO_XGMI_MAX_MB", "512")) * 2**20
        if self.grad_bytes() > limit or any(dt not in (torch.float32, torch.bfloat16) for dt in self.flat):
            self.comm_info["xgmi"] = "not used (gradients above PTO_XGMI_MAX_MB or not fp32/bf16)"
            return
        decisions = []
        for dt, buf in self.flat.items():
            try:
                ar = XgmiAllReduce(buf, group=self.pg, timeout_ms=int(os.environ.get("PTO_XGMI_TIMEOUT_MS", "10000")))
            except (RuntimeError, ValueError) as e:  # every rank raises together
                self.comm_info["xgmi"] = f"setup failed: {e}"[:300]
                return
            mine = [(i, b) for i, b in enumerate(self.buckets) if b["dtype"] == dt]
            ranges = [(b["lo"], b["hi"] - b["lo"]) for _, b in mine]
            res = ar.verify_with_fallback(ranges)
            if not res["correct"]:
                ar.close()
                self.comm_info["xgmi"] = {k: v for k, v in res.items() if k != "verify_log"}
                return
            used = False
            plan = plan_bucket_timing([n for _, n in ranges], int(os.environ.get("PTO_XGMI_TUNE_CLASSES", "4")))
            timings: dict[int, tuple] = {}
            t0 = time.perf_counter()
            for k, ((i, b), rng) in enumerate(zip(mine, ranges)):
                j = plan[k]
                if j not in timings:
                    timings[j] = ar.time_vs_collective([ranges[j]], iters=10, stream=self.comm_stream)
                tx, tr, ok = timings[j]
                take = ok and (comm == "xgmi" or tx < tr)
                b["transport"] = "xgmi" if take else "rccl"
                b["chan"] = i % 2
                used |= take
                decisions.append({"bucket": i, "mb": round((b["hi"] - b["lo"]) * buf.element_size() / 2**20, 2),
                                  "xgmi_us": round(tx, 1), "rccl_us": round(tr, 1), "use": b["transport"],
                                  "timed_on": mine[j][0]})
            self.comm_info["xgmi_tune_s"] = round(self.comm_info.get("xgmi_tune_s", 0.0) + time.perf_counter() - t0, 3)
            self.comm_info["xgmi_timed_buckets"] = self.comm_info.get("xgmi_timed_buckets", 0) + len(timings)
            if used:
                self._xgmi[dt] = ar
            else:
                ar.close()
        self.comm_info.update(transport="xgmi+rccl" if self._xgmi else "rccl", xgmi_buckets=decisions)

    # ------------------------------------------------------------------
    def reset(self):
        self._pending = [len(b["params"]) for b in self.buckets]
        self._copies = [[] for _ in self.buckets]
        self._works = []

    def _bucket_view(self, b):
        return self.flat[b["dtype"]][b["lo"]:b["hi"]]

    def _launch(self, i):
        b = self.buckets[i]
        t = self._bucket_view(b)
        if b.get("transport") == "xgmi":  # the peer-memory kernel on the comm stream (no work handle)
            ar = self._xgmi[b["dtype"]]
            if self.comm_stream is not None:
                self.comm_stream.wait_event(torch.cuda.current_stream(t.device).record_event())
            ar.allreduce_(b["lo"], b["hi"] - b["lo"], chan=b["chan"], stream=self.comm_stream)
            return
        if self.comm_stream is not None:
            ev = torch.cuda.current_stream(t.device).record_event()
            self.comm_stream.wait_event(ev)
            with torch.cuda.stream(self.comm_stream):
                self._works.append(dist.all_reduce(t, group=self.pg, async_op=True))
        else:
            self._works.append(dist.all_reduce(t, group=self.pg, async_op=True))

    def _on_grad(self, p):
        i = self._bucket_of[p]
        if self.mode == "copy":
            v = self._views[p]
            if self.accum_steps > 1:
                # summed (at the boundary: folded into its slot) with the rest of its
                # bucket; until that launch the list keeps the fresh gradient alive
                self._copies[i].append((p, p.grad))
                p.grad = v if self.at_boundary else None
            elif p.grad is not v:  # copied with the rest of its bucket, one multi-tensor launch
                self._copies[i].append((v, p.grad))
                p.grad = v
        self._pending[i] -= 1
        if self._pending[i] == 0:
            self._flush(i)
            if self.overlap and self.at_boundary:
                self._launch(i)

    def _flush(self, i):
        """Copy bucket ``i``'s gradients into their slots: ONE multi-tensor
        launch per bucket instead of one copy kernel per parameter (161 on
        ResNet-50: ~0.8 ms/step of launch-bound copies).  With
        ``accum_steps > 1`` that launch is the accumulation: INIT / ADD into
        the fp32 sums, at the boundary FOLD into the slots (the same bytes
        written as by the copy)."""
        cp = self._copies[i]
        if cp and self.accum_steps > 1:
            self._accumulate([(g, self._acc[p], self._views[p] if self.at_boundary else None) for p, g in cp])
            self._copies[i] = []
        elif cp:
            torch._foreach_copy_([v for v, _ in cp], [g for _, g in cp])
            self._copies[i] = []

    @property
    def at_boundary(self) -> bool:
        """True while the micro-batch in flight is the last of its optimizer
        step: its :meth:`finish` all-reduces and the optimizer follows
        (always, with ``accum_steps == 1``)."""
        return self._micro == self.accum_steps - 1

    def _accumulate(self, records):
        from ..ops.optim import grad_accum_multi

        grad_accum_multi(records, "fold" if self.at_boundary else ("init" if self._micro == 0 else "add"))

    def _finish_micro(self):
        """``accum_steps > 1``: what :meth:`finish` does with this
        micro-batch's gradients before any collective."""
        boundary = self.at_boundary
        if self.mode == "copy":
            for i, b in enumerate(self.buckets):
                if self._pending[i] > 0:  # some of its params got no gradient: null records
                    have = {id(p) for p, _ in self._copies[i]}
                    for p in b["params"]:
                        if id(p) not in have:
                            self._copies[i].append((p, None))
                            if boundary:
                                p.grad = self._views[p]
                    self._flush(i)
            return
        # "none": one launch per gradient dtype over all parameters; the boundary folds in place
        records = []
        for p in self.params:
            g = p.grad
            if boundary and g is None:
                p.grad = torch.empty_like(p)
            records.append((g, self._acc[p], p.grad if boundary else None))
            if not boundary:
                p.grad = None
        self._accumulate(records)

    def finish(self):
        """Call after ``loss.backward()``: launches any bucket whose params
        produced no gradient, waits for all collectives, joins the streams.
        With ``accum_steps > 1`` only every ``accum_steps``-th call does so;
        the others sum the gradients and return."""
        if self.accum_steps > 1:
            self._finish_micro()
            if not self.at_boundary:
                self._micro += 1
                self.reset()
                return
            self._micro = 0
        elif self.mode == "copy":
            for p, v in self._views.items():  # params that got no gradient this step
                if p.grad is not v:
                    if p.grad is None:
                        v.zero_()
                    else:
                        v.copy_(p.grad)
                    p.grad = v
            for i in range(len(self.buckets)):
                self._flush(i)
        if self.ddp:
            if not self.overlap:
                for i in range(len(self.buckets)):
                    self._launch(i)
            else:
                for i, n in enumerate(self._pending):
                    if n > 0:
                        self._pending[i] = 0
                        self._launch(i)
            for w in self._works:
                w.wait()
            if self.comm_stream is not None:
                torch.cuda.current_stream(self.comm_stream.device).wait_stream(self.comm_stream)
            for ar in self._xgmi.values():
                ar.poll()  # a stalled/dead peer raises XgmiTimeout (one step late, never blocking)
        self.reset()

    @property
    def optimizer_zeroes_grads(self) -> bool:
        """``view`` mode needs the fused optimizer to zero the grads in its pass."""
        return self.mode == "view"

    def release(self):
        """After the optimizer step: drop the gradients (``copy``/``none``) so
        the next backward hands fresh tensors over instead of accumulating."""
        if self.mode != "view":
            for p in self.params:
                p.grad = None

    @property
    def grad_scale(self) -> float:
        """Factor the optimizer folds into its gradient read (SUM -> mean
        over the ranks and their micro-batches)."""
        return 1.0 / (self.world * self.accum_steps)

    def zero_(self):
        for buf in self.flat.values():
            buf.zero_()

    def remove(self):
        for h in self._handles:
            h.remove()
        self._handles = []
        for ar in self._xgmi.values():
            ar.close()
        self._xgmi = {}

    def grad_bytes(self) -> int:
        return sum(b.numel() * b.element_size() for b in self.flat.values())

    def accum_bytes(self) -> int:
        """Bytes of the fp32 micro-batch accumulators (0 with ``accum_steps == 1``)."""
        return sum(a.numel() * a.element_size() for a in self._acc.values())
