"""Large-model DDP trainer CLI (BASELINE configs 3-5 as PyTorchJob
workloads): Llama-3 (``llama3-tiny`` / ``-1b`` / ``-8b``) or ResNet-50,
synthetic data, with periodic sharded checkpoints and automatic resume.

The reference's only workload is the MNIST example, which saves a final
``state_dict`` and cannot resume (``examples/mnist/mnist.py:146-147``); its
operator restarts failed replicas (``pkg/controller.v1/pytorch/pod.go:91-109``)
but a restarted replica starts from step 0.  Here:

* every ``--checkpoint-interval`` steps the full training state (params,
  BN buffers, fp32 master weights, optimizer moments, step counters) is
  written by :class:`~.checkpoint.ShardedCheckpointer`: each tensor once, by
  its owner rank, snapshotted to host memory and written on a background
  thread, the manifest committed last;
* on start the newest committed step is restored (own shard read, owners
  broadcast) and training continues from it ("Resumed from <dir> at step N");
* ``--grad-accum-steps N`` makes every step N micro-batches of
  ``--batch-size`` with one optimizer update (fp32 gradient sums on the
  device); checkpoints fall between optimizer steps and need nothing extra;
* ``--label-smoothing F`` / ``--z-loss F`` set the options of the training
  loss (the Llama cross entropy computes both inside its HIP kernels;
  ``--z-loss`` is Llama only) and ``--z-loss`` logs the z part of the loss;
* ``--eval-interval N`` (Llama only) evaluates the model every N optimizer
  steps and after the last one on ``--eval-batches K`` held-out synthetic
  batches it never trains on: plain NLL (no smoothing, no z-loss),
  perplexity, top-1 and top-``--eval-topk`` accuracy, accumulated on the
  device with one all-reduce and one sync per evaluation, the head GEMM in
  chunks of ``--eval-head-chunk R`` rows so the full logits never exist.
  It prints an ``eval step`` line, emits an ``eval`` metrics event, and its
  time stays out of the samples/s of the training log;
* ``--sample-interval N`` (Llama only) lets rank 0 generate
  ``--sample-tokens T`` tokens after the first ``--sample-prompt-len P``
  tokens of a held-out row every N optimizer steps and after the last one,
  with the KV-cache decode path (greedy, or ``--temperature F`` /
  ``--top-k K`` sampling from ``--sample-seed S``).  It prints a
  ``sample step`` line, emits a ``sample`` metrics event, and its time
  stays out of the samples/s as well;
* a collective failure exits 138 (retryable for ``restartPolicy: ExitCode``)
  exactly like the MNIST trainer, so kill/rejoin works for these models too.

Example (one replica per GPU, through the operator or torchrun)::

    python -m pytorch_operator_1_amd.train.lm --model llama3-8b --steps 1000 \\
        --checkpoint-dir /ckpt/job --checkpoint-interval 100 --backend rccl
"""
from __future__ import annotations

import argparse
import os
import signal
import sys
import time

import torch

from ..utils import dist as pdist
from . import checkpoint as ckpt
from .mnist import Metrics, run_with_retryable_exit


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Llama-3 / ResNet-50 DDP trainer (MI355X)")
    p.add_argument("--model", default="llama3-tiny",
                   choices=["llama3-tiny", "llama3-mini", "llama3-1b", "llama3-8b", "resnet50"])
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--batch-size", type=int, default=None, help="per rank (default 2 llama, 64 resnet50)")
    p.add_argument("--seq-len", type=int, default=512)
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log-interval", type=int, default=10)
    p.add_argument("--backend", default=None, help="rccl|nccl|gloo (default: rccl on GPU, gloo on CPU)")
    p.add_argument("--no-cuda", action="store_true")
    p.add_argument("--activation-checkpoint", choices=["none", "full"], default="none")
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--checkpoint-interval", type=int, default=0)
    p.add_argument("--sync-checkpoint", action="store_true", help="write shards on the training thread")
    p.add_argument("--fail-at-step", type=int, default=int(os.environ.get("PTO_FAIL_AT_STEP", "0")),
                   help="fault injection: SIGKILL self before this step (first incarnation only)")
    p.add_argument("--fail-rank", type=int, default=int(os.environ.get("PTO_FAIL_RANK", "0")))
    p.add_argument("--max-grad-norm", type=float, default=None,
                   help="clip the global gradient norm to this value on the device and log it "
                        "(inf: log the norm without clipping; default: off)")
    p.add_argument("--grad-accum-steps", type=int, default=1,
                   help="micro-batches of --batch-size per optimizer step, their gradients summed in fp32 on "
                        "the device (default 1: off); --steps counts optimizer steps")
    p.add_argument("--label-smoothing", type=float, default=0.0,
                   help="label smoothing of the cross entropy, in [0, 1) (default 0: off)")
    p.add_argument("--z-loss", type=float, default=0.0,
                   help="coefficient of the z-loss, z_loss * logsumexp(logits)^2 per token, added to the Llama "
                        "loss and logged (default 0: off; about 1e-4 in bf16 LM recipes)")
    p.add_argument("--eval-interval", type=int, default=0,
                   help="evaluate the Llama model on held-out synthetic batches every N optimizer steps and after "
                        "the last one: plain NLL, perplexity, top-1 / top-k accuracy, accumulated on the device "
                        "(default 0: off)")
    p.add_argument("--eval-batches", type=int, default=1, help="held-out batches of --batch-size per evaluation")
    p.add_argument("--eval-topk", type=int, default=5, help="k of the top-k accuracy")
    p.add_argument("--eval-head-chunk", type=int, default=2048,
                   help="rows of logits alive at once during evaluation (the head GEMM runs per chunk)")
    p.add_argument("--sample-interval", type=int, default=0,
                   help="generate from a held-out prompt with the Llama model every N optimizer steps and after "
                        "the last one (default 0: off)")
    p.add_argument("--sample-tokens", type=int, default=32, help="tokens to generate per sample")
    p.add_argument("--sample-prompt-len", type=int, default=16, help="prompt tokens taken from the held-out row")
    p.add_argument("--temperature", type=float, default=0.0, help="sampling temperature (default 0: greedy)")
    p.add_argument("--top-k", type=int, default=0, help="sample among the k most likely tokens (default 0: all)")
    p.add_argument("--sample-seed", type=int, default=0, help="seed of the sampler's uniforms")
    args = p.parse_args(argv)
    if args.sample_interval < 0:
        p.error("--sample-interval must be >= 0")
    if args.sample_tokens < 1 or args.sample_prompt_len < 1:
        p.error("--sample-tokens and --sample-prompt-len must be >= 1")
    if not args.temperature >= 0.0 or args.top_k < 0:
        p.error("--temperature and --top-k must be >= 0")
    if args.model == "resnet50" and (args.sample_interval or args.sample_tokens != 32 or args.sample_prompt_len != 16
                                     or args.temperature != 0.0 or args.top_k != 0 or args.sample_seed != 0):
        p.error("--sample-interval / --sample-tokens / --sample-prompt-len / --temperature / --top-k / "
                "--sample-seed are for the Llama models")
    if args.model != "resnet50" and args.sample_interval and args.sample_prompt_len > args.seq_len:
        p.error("--sample-prompt-len must not exceed --seq-len")
    if args.eval_interval < 0:
        p.error("--eval-interval must be >= 0")
    if args.eval_batches < 1 or args.eval_topk < 1 or args.eval_head_chunk < 1:
        p.error("--eval-batches, --eval-topk and --eval-head-chunk must be >= 1")
    if args.model == "resnet50" and (args.eval_interval or args.eval_batches != 1 or args.eval_topk != 5
                                     or args.eval_head_chunk != 2048):
        p.error("--eval-interval / --eval-batches / --eval-topk / --eval-head-chunk are for the Llama models")
    if not 0.0 <= args.label_smoothing < 1.0:
        p.error("--label-smoothing must be in [0, 1)")
    if not args.z_loss >= 0.0:
        p.error("--z-loss must be >= 0")
    if args.z_loss > 0 and args.model == "resnet50":
        p.error("--z-loss is for the Llama models")
    if args.grad_accum_steps < 1:
        p.error("--grad-accum-steps must be >= 1")
    if args.max_grad_norm is not None and not args.max_grad_norm >= 0:
        p.error("--max-grad-norm must be >= 0")
    return args


def build(args, device):
    from .bench_models import LlamaTrainer, ResNetTrainer

    if args.model == "resnet50":
        kw = {} if args.lr is None else {"lr": args.lr}
        return ResNetTrainer(device, batch_size=args.batch_size or 64, image_size=args.image_size, seed=args.seed,
                             max_grad_norm=args.max_grad_norm, grad_accum_steps=args.grad_accum_steps,
                             label_smoothing=args.label_smoothing, **kw)
    kw = {} if args.lr is None else {"lr": args.lr}
    return LlamaTrainer(device, model=args.model, batch_size=args.batch_size or 2, seq_len=args.seq_len,
                        seed=args.seed, checkpoint=args.activation_checkpoint, max_grad_norm=args.max_grad_norm,
                        grad_accum_steps=args.grad_accum_steps, label_smoothing=args.label_smoothing,
                        z_loss=args.z_loss, **kw)


def _evaluate(args, trainer, device, metrics, done: int, rank: int) -> float:
    """One held-out evaluation after optimizer step ``done``: print and emit
    it, return the seconds it took (the training steps before it are
    finished first, so none of their time is counted as evaluation)."""
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t0 = time.time()
    ev = trainer.evaluate(batches=args.eval_batches, topk=args.eval_topk, head_chunk=args.eval_head_chunk)
    print(f"eval step {done}\tloss={ev['loss']:.6f}\tppl={ev['ppl']:.4f}\ttop1={ev['top1']:.6f}\t"
          f"top{ev['k']}={ev['topk']:.6f}\ttokens={ev['tokens']}", flush=True)
    metrics.emit(event="eval", step=done, loss=ev["loss"], ppl=ev["ppl"], top1=ev["top1"], topk=ev["topk"],
                 k=ev["k"], tokens=ev["tokens"], rank=rank)
    return time.time() - t0


def _sample(args, trainer, device, metrics, done: int, rank: int) -> float:
    """One generation after optimizer step ``done``, on rank 0 alone (it
    needs no collective): print and emit it, return the seconds it took."""
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t0 = time.time()
    if rank == 0:
        prompt, tokens = trainer.sample(prompt_len=args.sample_prompt_len, new_tokens=args.sample_tokens,
                                        temperature=args.temperature, top_k=args.top_k, seed=args.sample_seed)
        print(f"sample step {done}\tprompt={prompt}\ttokens={tokens}", flush=True)
        metrics.emit(event="sample", step=done, prompt=prompt, tokens=tokens, temperature=args.temperature,
                     top_k=args.top_k, seed=args.sample_seed, rank=rank)
    return time.time() - t0


def _main(argv=None):
    args = parse_args(argv)
    use_gpu = not args.no_cuda and torch.cuda.is_available() and os.environ.get("PTO_NO_GPU") != "1"
    env, device = pdist.init_distributed(args.backend, use_gpu=use_gpu)
    rank, world = env.rank, env.world_size
    metrics = Metrics()
    trainer = build(args, device)
    saver = None
    start = 0
    if args.checkpoint_dir:
        saver = ckpt.ShardedCheckpointer(args.checkpoint_dir, rank, world, async_write=not args.sync_checkpoint)
        man = saver.load_into(trainer.checkpoint_tensors(), create=trainer.create_state)
        if man is not None:
            trainer.after_load(man["meta"])
            start = int(man["step"])
            print(f"Resumed from {saver.resumed_from} at step {start}", flush=True)
    fail = args.fail_at_step if (args.fail_at_step and rank == args.fail_rank and start == 0) else 0
    t_last, steps_since = time.time(), 0
    for step in range(start, args.steps):
        if fail and step == fail:
            # deterministic injection: the kill lands after the checkpoint in
            # flight is durable (a real crash may lose it; resume then falls
            # back to the previous committed step)
            if saver:
                saver.commit()
            print(f"[fault-injection] rank {rank} SIGKILL at step {step}", flush=True)
            os.kill(os.getpid(), signal.SIGKILL)
        trainer.step()
        steps_since += 1
        done = step + 1
        if done == start + 1:
            if device.type == "cuda":
                torch.cuda.synchronize(device)
            metrics.emit(event="first_step", t=time.time(), rank=rank)
        if done % args.log_interval == 0 or done == args.steps:
            loss = trainer.last_loss()
            now = time.time()
            sps = steps_since * trainer.samples_per_step() * world / max(now - t_last, 1e-9)
            clip, extra = "", {}
            if args.max_grad_norm is not None:  # read here only: last_loss() has already synced
                extra = {"grad_norm": trainer.last_grad_norm(), "clip_coef": trainer.last_clip_coef()}
                clip = f"\tgrad_norm={extra['grad_norm']:.4f}"
            if args.z_loss > 0:  # likewise after the sync
                extra["z_loss"] = trainer.last_z_loss()
                clip += f"\tz_loss={extra['z_loss']:.6f}"
            print(f"step {done}/{args.steps}\tloss={loss:.6f}{clip}\t{sps:.1f} samples/s", flush=True)
            metrics.emit(event="train", step=done, loss=loss, samples_per_sec=round(sps, 1),
                         step_seconds=(now - t_last) / steps_since, rank=rank, **extra)
            t_last, steps_since = now, 0
        if args.eval_interval and (done % args.eval_interval == 0 or done == args.steps):
            t_last += _evaluate(args, trainer, device, metrics, done, rank)  # outside the throughput window
        if args.sample_interval and (done % args.sample_interval == 0 or done == args.steps):
            t_last += _sample(args, trainer, device, metrics, done, rank)
        if saver and args.checkpoint_interval and done % args.checkpoint_interval == 0 and done < args.steps:
            saver.save(done, trainer.checkpoint_tensors(), trainer.checkpoint_meta())
    if saver:
        saver.save(args.steps, trainer.checkpoint_tensors(), trainer.checkpoint_meta())
        saver.close()
    print(f"final_loss={trainer.last_loss():.8f}", flush=True)
    pdist.cleanup()
    return 0


def main(argv=None):
    return run_with_retryable_exit(_main, argv)


if __name__ == "__main__":
    sys.exit(main())
