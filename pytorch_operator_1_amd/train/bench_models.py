"""Large-model DDP training steps for BASELINE configs 3 and 4.

* :class:`ResNetTrainer` — ResNet-50, ImageNet-shaped 224x224 synthetic
  batches, channels_last + bf16 autocast, fp32 master params, SGD
  momentum 0.9 / wd 1e-4 as one HIP launch (``FusedSGD``).
* :class:`LlamaTrainer` — Llama-3-8B (or a smaller preset), bf16 params,
  mixed-precision AdamW (fp32 master/m/v) as one HIP launch
  (``FusedAdamW``), HIP kernels between the hipBLASLt GEMMs.

Both use :class:`..parallel.ddp.GradBucketer`: grads accumulate straight
into flat buckets that are all-reduced over RCCL/xGMI on a comm stream
while backward continues; the 1/world average and grad zeroing are folded
into the optimizer's single pass.  Each ``step()`` is a complete optimizer
step (forward, backward, all-reduce, update) — nothing is skipped.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from ..ops.conv1x1 import GradStash
from ..ops.optim import FusedAdamW, FusedSGD
from ..parallel.ddp import GradBucketer
from ..utils.profiling import StepTimer


class _TorchOpt:
    """Stock ``torch.optim`` behind the fused optimizers' ``step(grad_scale,
    zero_grad, max_grad_norm)`` call (CPU runs: the HIP optimizers need a
    GPU).  Clipping is ``torch.nn.utils.clip_grad_norm_`` on the scaled
    gradients; ``grad_norm`` / ``clip_coef`` as on the fused optimizers."""

    def __init__(self, opt):
        self.opt = opt
        self.state = opt.state
        self.param_groups = opt.param_groups
        self.grad_norm = None
        self.clip_coef = None

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, zero_grad: bool = False, max_grad_norm: float | None = None):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None and grad_scale != 1.0:
                    p.grad.mul_(grad_scale)
        if max_grad_norm is not None:
            params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
            total = torch.nn.utils.clip_grad_norm_(params, max_grad_norm, error_if_nonfinite=False)
            self.grad_norm = total.detach().float().reshape(1)
            self.clip_coef = torch.clamp(max_grad_norm / (self.grad_norm + 1e-6), max=1.0)
        self.opt.step()
        if zero_grad:
            self.opt.zero_grad(set_to_none=False)


def _scalar(t):
    """Host value of a 1-element tensor (a device sync), None before the first step."""
    return None if t is None else float(t)


def _accum_steps(n) -> int:
    if int(n) != n or n < 1:
        raise ValueError(f"grad_accum_steps must be an integer >= 1, got {n}")
    return int(n)


def _accum_text(n: int, bucketer) -> str:
    if n == 1:
        return "off"
    return (f"{n} micro-batches per optimizer step, fp32 sums on the device "
            f"({bucketer.accum_bytes() / 2**20:.0f} MB of accumulators)")


def _clip_text(max_grad_norm):
    if max_grad_norm is None:
        return "off"
    if max_grad_norm == float("inf"):
        return "norm reported, not clipped"
    return f"global grad norm clipped to {max_grad_norm:g} on the device"


def _loss_text(label_smoothing: float, z_loss: float = 0.0) -> str:
    if not (label_smoothing or z_loss):
        return "CE"
    return f"CE label_smoothing={label_smoothing:g} z_loss={z_loss:g}"


class CheckpointMixin:
    """Named tensors of the full training state (parameters, buffers,
    optimizer state) for :class:`..train.checkpoint.ShardedCheckpointer`,
    and the inverse.  DDP replicas hold identical copies, so the sharded
    checkpointer writes each tensor once (its owner rank).

    Checkpoints are taken between optimizer steps.  There the bucketer's
    fp32 micro-batch accumulators (``grad_accum_steps > 1``) are dead: the
    first micro-batch of the next step overwrites them.  So they are not
    checkpointed, and a run resumes the same with any ``grad_accum_steps``."""

    def _param_names(self):
        return {p: n for n, p in self.model.named_parameters()}

    def checkpoint_tensors(self) -> dict:
        t = {f"model.{n}": p.data for n, p in self.model.named_parameters()}
        t.update({f"buffer.{n}": b for n, b in self.model.named_buffers()})
        names = self._param_names()
        for p, st in self.opt.state.items():
            for k, v in st.items():
                if torch.is_tensor(v):
                    t[f"opt.{names[p]}.{k}"] = v
        return t

    def checkpoint_meta(self) -> dict:
        return {"steps_done": self.steps_done, "opt_step": getattr(self.opt, "_step", None)}

    def create_state(self, name: str, shape, dtype):
        """Destination for optimizer state that does not exist yet (resume
        before the first step): same layout as the parameter."""
        if not name.startswith("opt."):
            raise KeyError(name)
        pname, key = name[4:].rsplit(".", 1)
        p = dict(self.model.named_parameters())[pname]
        if list(p.shape) == list(shape):
            v = torch.zeros_like(p, dtype=dtype)
        else:
            v = torch.zeros(shape, dtype=dtype, device=p.device if key != "step" else "cpu")
        self.opt.state[p][key] = v
        return v

    def after_load(self, meta: dict):
        self.steps_done = int(meta.get("steps_done", 0))
        if meta.get("opt_step") is not None and hasattr(self.opt, "_step"):
            self.opt._step = int(meta["opt_step"])
        if hasattr(self.opt, "_tables"):
            self.opt._tables = None  # launch tables point at the old state tensors
        if getattr(self, "_graph", None) is not None:  # a captured step holds the old addresses too
            self._graph = None
            self._eager_done = 0
        refresh = getattr(self.model, "refresh_transposed", None)
        if refresh is not None and getattr(self, "transposed_dgrad", False):
            refresh()


class ResNetTrainer(CheckpointMixin):
    """``graph`` (``PTO_STEP_GRAPH=1``): replay the whole step (forward,
    loss, backward, FusedSGD) as ONE captured HIP graph after
    ``EAGER_STEPS`` eager steps (MIOpen's solver search, library handles and
    the optimizer state are created eagerly); single-process runs only
    (``GradBucketer`` mode ``none``).  Off by default: at batch 256 the GPU
    is never starved by the ~1,400 eager launches per step (26.74 vs 26.73
    ms/step measured, profiles/resnet50_r5.md), so the graph buys nothing
    here -- it is for smaller per-GPU batches, where launch latency shows.

    ``grad_accum_steps=N``: one optimizer step over N micro-batches of
    ``batch_size`` (see :class:`LlamaTrainer`); not with the captured step."""

    EAGER_STEPS = 2

    def __init__(self, device, batch_size: int = 256, image_size: int = 224, lr: float = 0.1,
                 momentum: float = 0.9, weight_decay: float = 1e-4, seed: int = 0, bucket_mb: float | None = None,
                 force_ddp: bool = False, graph: bool | None = None, max_grad_norm: float | None = None,
                 grad_accum_steps: int = 1, label_smoothing: float = 0.0):
        from ..models.resnet import resnet50, synthetic_images

        self.grad_accum_steps = _accum_steps(grad_accum_steps)
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        self.label_smoothing = float(label_smoothing)  # the ImageNet recipe: 0.1; fixed once a step is captured
        if graph is None:
            graph = os.environ.get("PTO_STEP_GRAPH", "0") == "1"
        if graph and self.grad_accum_steps > 1:
            raise ValueError("ResNetTrainer: the captured step (graph=True / PTO_STEP_GRAPH=1) is one micro-batch "
                             "per optimizer step; use grad_accum_steps=1 or graph=False")
        torch.manual_seed(seed)
        # MIOpen find: benchmark the conv solvers once per shape (warmup) and
        # keep the fastest instead of the heuristic pick
        torch.backends.cudnn.benchmark = True
        self.device = device
        self.batch_size = batch_size
        self.max_grad_norm = max_grad_norm  # global-norm clip (inf: report only); fixed once a step is captured
        self.model = resnet50().to(device=device, memory_format=torch.channels_last)
        self.model.train()
        self.bucketer = GradBucketer(self.model, bucket_mb=bucket_mb, force_ddp=force_ddp,
                                     accum_steps=self.grad_accum_steps)
        if device.type == "cuda":
            self.opt = FusedSGD(self.model.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
        else:
            self.opt = _TorchOpt(torch.optim.SGD(self.model.parameters(), lr=lr, momentum=momentum,
                                                 weight_decay=weight_decay))
        # images arrive in the compute dtype on the GPU (what a GPU-side
        # decode/normalise stage hands over); the model casts nothing per step
        self.x, self.y = synthetic_images(batch_size * self.grad_accum_steps, device, image_size, seed=seed,
                                          dtype=torch.bfloat16 if device.type == "cuda" else torch.float32)
        # the fixed micro-batches of one optimizer step: the rows of ONE batch of batch_size * N
        self._micro = list(zip(self.x.split(batch_size), self.y.split(batch_size)))
        self._loss = None
        self.steps_done = 0
        self.timer = StepTimer(device, enabled=False)
        self.use_graph = bool(graph) and device.type == "cuda" and self.bucketer.mode == "none"
        self._graph = None
        self._eager_done = 0

    def step(self):
        if not self.use_graph or self._eager_done < self.EAGER_STEPS:
            self._eager_step()
            self._eager_done += 1
            return
        if self._graph is None:
            self._capture()
        self.opt.sync_lr()
        self._graph.replay()
        self.steps_done += 1

    def _capture(self):
        """Record one whole step into a HIP graph (nothing executes while
        capturing: :meth:`step` replays it right after)."""
        torch.cuda.synchronize(self.device)
        self.bucketer.release()  # grads None: the captured backward allocates them in the graph's pool
        self.opt.prepare_capture(max_grad_norm=self.max_grad_norm)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                out = self.model(self.x)
            loss = F.cross_entropy(out.float(), self.y, label_smoothing=self.label_smoothing)
            loss.backward()
            GradStash.assert_drained()
            self.bucketer.finish()
            self.opt.step(grad_scale=self.bucketer.grad_scale, zero_grad=self.bucketer.optimizer_zeroes_grads,
                          max_grad_norm=self.max_grad_norm)
        self.opt.finish_capture()  # the launch table of the graph's gradients
        self._loss = loss.detach()
        self._graph = g

    def _eager_step(self):
        t = self.timer
        total = None
        for x, y in self._micro:
            with t.phase("forward"), torch.autocast(device_type=self.device.type, dtype=torch.bfloat16):
                out = self.model(x)
            with t.phase("forward"):
                loss = F.cross_entropy(out.float(), y, label_smoothing=self.label_smoothing)
            with t.phase("backward"):
                loss.backward()
                GradStash.assert_drained()  # host counter: no sibling conv1x1 gradient left parked
            with t.phase("allreduce_wait"):  # not the last micro-batch: the fp32 accumulation, no collective
                self.bucketer.finish()
            total = loss.detach() if total is None else total + loss.detach()
        if self.grad_accum_steps > 1:
            loss = total / self.grad_accum_steps
        with t.phase("optimizer"):
            self.opt.step(grad_scale=self.bucketer.grad_scale, zero_grad=self.bucketer.optimizer_zeroes_grads,
                          max_grad_norm=self.max_grad_norm)
            self.bucketer.release()
        self._loss = loss.detach()
        self.steps_done += 1

    def run(self, n: int):
        for _ in range(n):
            self.step()

    def last_loss(self):
        return None if self._loss is None else float(self._loss)

    def last_grad_norm(self):
        return _scalar(self.opt.grad_norm) if self.max_grad_norm is not None else None

    def last_clip_coef(self):
        return _scalar(self.opt.clip_coef) if self.max_grad_norm is not None else None

    def samples_per_step(self) -> int:
        return self.batch_size * self.grad_accum_steps

    def describe(self) -> dict:
        return {"model": "resnet50 (v1.5, 25.6M params)", "input_shape": [3, 224, 224],
                "optimizer": "SGD momentum=0.9 wd=1e-4 (FusedSGD HIP)", "amp": "bf16 autocast, fp32 master",
                "step": (f"whole step replayed as one HIP graph (after {self.EAGER_STEPS} eager steps)"
                         if self.use_graph else "eager"),
                "grad_clip": _clip_text(self.max_grad_norm),
                "grad_accum": _accum_text(self.grad_accum_steps, self.bucketer),
                "loss": _loss_text(self.label_smoothing)}


class LlamaTrainer(CheckpointMixin):
    def __init__(self, device, model: str = "llama3-8b", batch_size: int = 2, seq_len: int = 4096,
                 lr: float = 3e-4, weight_decay: float = 0.1, seed: int = 0, checkpoint: str = "none",
                 impl: str | None = None, bucket_mb: float | None = None, force_ddp: bool = False,
                 max_grad_norm: float | None = None, grad_accum_steps: int = 1, label_smoothing: float = 0.0,
                 z_loss: float = 0.0):
        """``label_smoothing`` / ``z_loss``: options of the training loss
        (:class:`..models.llama.Llama`); :meth:`last_z_loss` is the z part of
        the last step's loss.

        ``grad_accum_steps=N``: :meth:`step` stays ONE optimizer step and
        runs N micro-batches of ``batch_size`` rows (forward, backward,
        ``bucketer.finish()``), summing their gradients in fp32 on the device
        (:class:`..parallel.ddp.GradBucketer`); optimizer, weight
        re-transposes and all-reduce are paid once per N.  The synthetic data
        is ONE batch of ``batch_size * N`` rows cut into N fixed micro-batches.
        Every micro-batch loss is a mean over its own tokens and the step
        weighs them 1/N each, which is the mean over all tokens only when the
        micro-batches hold equally many valid tokens (true of the synthetic
        data; a loader with padding would have to weigh by token count)."""
        from ..models.llama import CONFIGS, Llama, synthetic_tokens

        self.grad_accum_steps = _accum_steps(grad_accum_steps)
        torch.manual_seed(seed)
        impl = impl or ("hip" if device.type == "cuda" else "torch")
        self.cfg = CONFIGS[model]
        self.name = model
        self.device = device
        self.batch_size, self.seq_len = batch_size, seq_len
        self.max_grad_norm = max_grad_norm  # global-norm clip (the Llama recipe: 1.0; inf: report only)
        self.model = Llama(self.cfg, impl=impl, device=device, checkpoint=checkpoint, label_smoothing=label_smoothing,
                           z_loss=z_loss)
        self.model.train()
        # W^T copies for K-contiguous dgrad GEMMs (PTO_WT=0: plain F.linear backward;
        # with PTO_GEMM=1 the package's NN GEMM then reads W as stored, ops/gemm.py)
        self.transposed_dgrad = impl == "hip" and os.environ.get("PTO_WT", "1") == "1"
        if self.transposed_dgrad:
            self.model.enable_transposed_dgrad()
        self.bucketer = GradBucketer(self.model, bucket_mb=bucket_mb, force_ddp=force_ddp,
                                     accum_steps=self.grad_accum_steps)
        if device.type == "cuda":
            self.opt = FusedAdamW(self.model.parameters(), lr=lr, betas=(0.9, 0.95), eps=1e-8,
                                  weight_decay=weight_decay)
        else:  # CPU: stock AdamW on the bf16 params (tests of the checkpoint/resume path)
            self.opt = _TorchOpt(torch.optim.AdamW(self.model.parameters(), lr=lr, betas=(0.9, 0.95), eps=1e-8,
                                                   weight_decay=weight_decay))
        self.tokens, self.labels = synthetic_tokens(batch_size * self.grad_accum_steps, seq_len, self.cfg.vocab_size,
                                                    device, seed=seed)
        self._micro = list(zip(self.tokens.split(batch_size), self.labels.split(batch_size)))
        self._loss = None
        self._z = None
        self._seed = seed
        self._heldout = []  # evaluate(split="heldout")'s batches, made on first use
        self._eval = None
        self.steps_done = 0
        self.timer = StepTimer(device, enabled=False)

    def step(self):
        t = self.timer
        total = ztotal = None
        for tokens, labels in self._micro:
            with t.phase("forward"):
                loss = self.model(tokens, labels)
            with t.phase("backward"):
                loss.backward()
            with t.phase("allreduce_wait"):  # not the last micro-batch: the fp32 accumulation, no collective
                self.bucketer.finish()
            total = loss.detach() if total is None else total + loss.detach()
            z = self.model.last_z_loss  # None when z_loss is off
            ztotal = z if ztotal is None or z is None else ztotal + z
        if self.grad_accum_steps > 1:
            loss = total / self.grad_accum_steps  # on the device, no sync
            ztotal = None if ztotal is None else ztotal / self.grad_accum_steps
        with t.phase("optimizer"):
            self.opt.step(grad_scale=self.bucketer.grad_scale, zero_grad=self.bucketer.optimizer_zeroes_grads,
                          max_grad_norm=self.max_grad_norm)
            self.bucketer.release()
            if self.transposed_dgrad:
                self.model.refresh_transposed()
        self._loss = loss.detach()
        self._z = ztotal
        self.steps_done += 1

    def run(self, n: int):
        for _ in range(n):
            self.step()

    def last_loss(self):
        return None if self._loss is None else float(self._loss)

    def last_z_loss(self):
        """The z part of the last step's loss (mean over its micro-batches); None when ``z_loss`` is off."""
        return _scalar(self._z)

    def _heldout_batches(self, n: int):
        """The first ``n`` held-out batches of ``batch_size x seq_len``, made
        on first use and kept.  Batch i of rank r is seeded from (seed, r, i)
        through a hash, so it differs from the training batch (seeded with
        ``seed`` itself) and from every other rank's and index's."""
        import hashlib

        import torch.distributed as dist

        from ..models.llama import synthetic_tokens

        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        while len(self._heldout) < n:
            key = f"heldout/{self._seed}/{rank}/{len(self._heldout)}".encode()
            s = int.from_bytes(hashlib.sha256(key).digest()[:8], "little") >> 1
            self._heldout.append(synthetic_tokens(self.batch_size, self.seq_len, self.cfg.vocab_size, self.device,
                                                  seed=s))
        return self._heldout[:n]

    def evaluate(self, batches: int = 1, split: str = "heldout", topk: int = 5, head_chunk: int | None = 2048) -> dict:
        """Plain NLL, perplexity and top-1 / top-``topk`` accuracy of the
        current weights, accumulated on the device
        (:class:`..ops.llm.EvalAccumulator`): ``split="heldout"`` over
        ``batches`` fixed synthetic batches the model never trains on,
        ``split="train"`` over the training micro-batches.  Under DDP the
        record is all-reduced, so every rank returns the same dict (kept for
        :meth:`last_eval`).  Reads the model and writes nothing training
        reads: weights, optimizer state, ``W^T`` copies, ``steps_done`` and
        the RNG streams are as before."""
        from ..ops.llm import EvalAccumulator

        if split == "heldout":
            if int(batches) != batches or batches < 1:
                raise ValueError(f"evaluate: batches must be an integer >= 1, got {batches}")
            data = self._heldout_batches(int(batches))
        elif split == "train":
            data = self._micro
        else:
            raise ValueError(f"evaluate: split must be heldout|train, got {split!r}")
        acc = EvalAccumulator(self.device, topk=topk)
        for tokens, labels in data:
            self.model.evaluate(tokens, labels, acc, head_chunk=head_chunk)
        acc.all_reduce()
        self._eval = acc.result()
        return self._eval

    def last_eval(self):
        """The dict of the last :meth:`evaluate`; None before the first."""
        return self._eval

    def sample(self, prompt_len: int = 16, new_tokens: int = 32, temperature: float = 0.0, top_k: int = 0,
               seed: int = 0):
        """Generate ``new_tokens`` tokens (:meth:`..models.llama.Llama.generate`)
        after the first ``prompt_len`` tokens of held-out batch 0, row 0:
        ``(prompt, tokens)`` as Python lists (the one host sync).  Like
        :meth:`evaluate` it writes nothing training reads."""
        if not 1 <= int(prompt_len) <= self.seq_len:
            raise ValueError(f"sample: prompt_len must be in [1, {self.seq_len}], got {prompt_len}")
        prompt = self._heldout_batches(1)[0][0][:1, :int(prompt_len)].contiguous()
        out = self.model.generate(prompt, max_new_tokens=int(new_tokens), temperature=temperature, top_k=top_k,
                                  seed=seed)
        return prompt[0].tolist(), out[0].tolist()

    def last_grad_norm(self):
        return _scalar(self.opt.grad_norm) if self.max_grad_norm is not None else None

    def last_clip_coef(self):
        return _scalar(self.opt.clip_coef) if self.max_grad_norm is not None else None

    def samples_per_step(self) -> int:
        return self.batch_size * self.grad_accum_steps * self.seq_len  # tokens

    def flops_per_step(self) -> float:
        return self.cfg.train_flops_per_token(self.seq_len) * self.samples_per_step()

    def describe(self) -> dict:
        return {"model": f"{self.name} ({self.cfg.num_params() / 1e9:.2f}B params)",
                "optimizer": "AdamW betas=(0.9,0.95) wd=0.1 (FusedAdamW HIP, fp32 master/m/v)",
                "amp": "bf16 params/activations, fp32 optimizer state",
                "checkpoint": self.model.checkpoint,
                "dgrad": "W^T copies (K-contiguous dX GEMMs)" if self.transposed_dgrad else "F.linear",
                "grad_clip": _clip_text(self.max_grad_norm),
                "grad_accum": _accum_text(self.grad_accum_steps, self.bucketer),
                "loss": _loss_text(self.model.label_smoothing, self.model.z_loss)}
