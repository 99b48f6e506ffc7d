"""Gradient accumulation over micro-batches, the parts that run without a
GPU: the torch path of ``grad_accum_multi``, ``GradBucketer(accum_steps=N)``
over gloo, the trainers' bookkeeping, the CLI flag and checkpoint/resume."""
import json
import multiprocessing as mp
import os
import socket

import pytest
import torch

from mp_util import collect

SHAPES = [(1,), (5,), (37, 61), (2 * 2048 + 13,)]


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_torch_path_all_modes_bitwise(dtype):
    from pytorch_operator_1_amd.ops.optim import grad_accum_multi

    gen = torch.Generator().manual_seed(1)

    def grads(missing=None):
        gs = [torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
        gs.append(torch.randn(4, 8, 3, 3, generator=gen).to(dtype).contiguous(memory_format=torch.channels_last))
        if missing is not None:
            gs[missing] = None
        return gs

    accs = [torch.full_like(g, 1e30, dtype=torch.float32) for g in grads()]  # garbage: INIT overwrites it
    want = [a.clone() for a in accs]
    for mode, missing in [("init", 1), ("add", 2), ("add", 4), ("fold", 3), ("fold", 0)]:
        gs = grads(missing)
        outs = [torch.full_like(a, -7.0, dtype=dtype) if mode == "fold" else None for a in accs]
        grad_accum_multi(list(zip(gs, accs, outs)), mode)
        for i, g in enumerate(gs):
            if mode == "init":
                want[i] = torch.zeros_like(want[i]) if g is None else g.float()
            elif mode == "add" and g is not None:
                want[i] = want[i] + g.float()
            assert torch.equal(bits(accs[i]), bits(want[i])), (mode, i)
            if mode == "fold":
                out = (want[i] if g is None else want[i] + g.float()).to(dtype)
                assert outs[i].dtype == dtype and torch.equal(bits(outs[i]), bits(out)), (mode, i)
    # in place: the gradient tensor itself receives the folded sum
    g = torch.ones(5, dtype=dtype)
    acc = torch.full((5,), 256.0)
    grad_accum_multi([(g, acc, g)], "fold")
    assert torch.equal(g, torch.full((5,), 257.0).to(dtype)) and torch.equal(acc, torch.full((5,), 256.0))
    with pytest.raises(ValueError):
        grad_accum_multi([(g, acc, None)], "fold")
    with pytest.raises(ValueError):
        grad_accum_multi([(g[:2], acc, None)], "add")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in SHAPES])


def _consts(rank, k):
    """Small integers: every sum below is exact in fp32."""
    gen = torch.Generator().manual_seed(100 + 10 * rank + k)
    return [torch.randint(-8, 9, s, generator=gen).float() for s in SHAPES]


def _bucket_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from pytorch_operator_1_amd.parallel.ddp import GradBucketer

    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    dist.all_reduce = counted
    m = Toy()
    bk = GradBucketer(m, bucket_mb=0.001, accum_steps=2)
    problems = []
    if bk.mode != "copy" or len(bk.buckets) < 3:
        problems.append(f"mode {bk.mode}, {len(bk.buckets)} buckets")
    sum((p * c).sum() for p, c in zip(m.ps, _consts(rank, 0))).backward()
    bk.finish()
    if calls or any(p.grad is not None for p in m.ps) or bk.at_boundary is not True:
        problems.append(f"after micro-batch 0: {len(calls)} collectives, at_boundary {bk.at_boundary}")
    sum((p * c).sum() for p, c in zip(m.ps, _consts(rank, 1))).backward()
    bk.finish()
    if len(calls) != len(bk.buckets):
        problems.append(f"{len(calls)} collectives for {len(bk.buckets)} buckets")
    for i, p in enumerate(m.ps):
        want = sum(_consts(r, 0)[i] + _consts(r, 1)[i] for r in range(world))
        if p.grad is None or not torch.equal(p.grad, want):
            problems.append(f"param {i}: wrong sum")
    q.put((rank, problems, bk.grad_scale))
    dist.destroy_process_group()


def test_bucketer_copy_mode_two_rank_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_bucket_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = collect(q, ps, 2, timeout=240)
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(r for r, _, _ in res) == [0, 1]
    for _, problems, scale in res:
        assert problems == []
        assert scale == 0.25


def test_view_mode_refuses_accumulation():
    from pytorch_operator_1_amd.parallel.ddp import GradBucketer

    with pytest.raises(ValueError, match="copy"):
        GradBucketer(Toy(), mode="view", accum_steps=2)
    bk = GradBucketer(Toy())
    assert bk.accum_steps == 1 and bk.accum_bytes() == 0 and bk.at_boundary and bk.grad_scale == 1.0


def _trainer(**kw):
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    return LlamaTrainer(torch.device("cpu"), model="llama3-tiny", batch_size=2, seq_len=32, **kw)


def test_llama_trainer_two_micro_batches():
    import math

    tr = _trainer(grad_accum_steps=2, max_grad_norm=float("inf"))
    one = _trainer()
    assert tr.tokens.shape == (4, 32) and [t.shape[0] for t, _ in tr._micro] == [2, 2]
    from pytorch_operator_1_amd.models.llama import synthetic_tokens

    # the rows of ONE batch of 4 from the same seed
    assert torch.equal(tr.tokens, synthetic_tokens(4, 32, tr.cfg.vocab_size, "cpu", seed=0)[0])
    assert torch.equal(torch.cat([t for t, _ in tr._micro]), tr.tokens)
    assert tr.samples_per_step() == 2 * one.samples_per_step() == 2 * 2 * 32
    tr.run(2)
    assert tr.steps_done == 2
    assert math.isfinite(tr.last_loss()) and math.isfinite(tr.last_grad_norm())
    assert tr.describe()["grad_accum"].startswith("2 micro-batches") and one.describe()["grad_accum"] == "off"
    assert tr.bucketer.accum_bytes() == 4 * sum(p.numel() for p in tr.model.parameters())
    assert tr.bucketer.grad_scale == 0.5
    with pytest.raises(ValueError):
        _trainer(grad_accum_steps=0)


def test_resnet_captured_step_refuses_accumulation():
    from pytorch_operator_1_amd.train.bench_models import ResNetTrainer

    with pytest.raises(ValueError, match="grad_accum_steps"):
        ResNetTrainer(torch.device("cpu"), batch_size=2, image_size=32, graph=True, grad_accum_steps=2)


def test_cli_flag():
    from pytorch_operator_1_amd.train import lm

    assert lm.parse_args([]).grad_accum_steps == 1
    assert lm.parse_args(["--grad-accum-steps", "4"]).grad_accum_steps == 4
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit):
            lm.parse_args(["--grad-accum-steps", bad])


def test_checkpoint_round_trip(tmp_path):
    """Save after step 1, resume into a new trainer, take step 2: the loss
    of an uninterrupted run, bitwise; the accumulators are not in the manifest."""
    from pytorch_operator_1_amd.train.checkpoint import ShardedCheckpointer

    def names(d, n):
        tr = _trainer(grad_accum_steps=n)
        tr.step()
        ck = ShardedCheckpointer(str(d), 0, 1, async_write=False)
        ck.save(1, tr.checkpoint_tensors(), tr.checkpoint_meta())
        ck.close()
        man = json.load(open(os.path.join(str(d), "step-000000001", "manifest.json")))
        return tr, set(man["tensors"])

    tr, with_accum = names(tmp_path / "n2", 2)
    _, without = names(tmp_path / "n1", 1)
    assert with_accum == without
    tr.step()
    resumed = _trainer(grad_accum_steps=2)
    man = ShardedCheckpointer(str(tmp_path / "n2"), 0, 1).load_into(resumed.checkpoint_tensors(),
                                                                     create=resumed.create_state)
    resumed.after_load(man["meta"])
    assert resumed.steps_done == 1
    resumed.step()
    assert resumed.steps_done == 2 and resumed.last_loss() == tr.last_loss()
