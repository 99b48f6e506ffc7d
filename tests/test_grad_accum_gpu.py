"""Gradient accumulation over micro-batches with fp32 sums on the device:
``k_grad_accum_multi`` (csrc/kernels/optim_kernels.hip) behind
``ops.optim.grad_accum_multi``, ``GradBucketer(accum_steps=N)`` and the
trainers' ``grad_accum_steps``.

The kernel's arithmetic is fully specified (one fp32 add, one round to
nearest even), so it is compared BITWISE with the same torch expression
evaluated on the same device.

Measured on an MI355X (test_trainer_accumulation_matches_one_batch, relative
errors against the fp32 ``impl="torch"`` model on the same rows; the bound for
``e_b`` is ``2 * e_a + 2^-9``): loss e_a 5.7e-6, e_b 5.7e-6; grad_norm
e_a 1.07e-3, e_b 1.07e-3 (profiles/grad_accum.md).
"""
import multiprocessing as mp
import socket

import pytest
import torch

from mp_util import collect

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
SHAPES = [(1,), (5,), (37, 61), (2 * 2048 + 13,)]  # the last: three blocks, ragged tail


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def _unaligned(n, dtype, gen):
    """A dense n-element view that starts one element past a 16-byte boundary."""
    v = torch.randn(n + 1, device=DEV, generator=gen).to(dtype)[1:]
    assert v.data_ptr() % 16 == v.element_size()
    return v


def _grads(dtype, gen):
    """One gradient per test tensor: SHAPES, an unaligned view (scalar path)
    and, in fp32, a channels-last 4-D tensor."""
    gs = [torch.randn(s, device=DEV, generator=gen).to(dtype) for s in SHAPES]
    gs.append(_unaligned(1001, dtype, gen))
    if dtype == torch.float32:
        gs.append(torch.randn(4, 8, 3, 3, device=DEV, generator=gen).contiguous(memory_format=torch.channels_last))
    return gs


def ref_step(mode, g, acc, dtype):
    """(acc, out) after one launch, by the torch expression of the kernel's table."""
    if mode == "init":
        return (torch.zeros_like(acc) if g is None else torch.empty_like(acc).copy_(g)), None
    if mode == "add":
        return (acc.clone() if g is None else acc + g.float()), None
    return acc.clone(), (acc if g is None else acc + g.float()).to(dtype)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_modes_bitwise(dtype, in_place):
    from pytorch_operator_1_amd.ops.optim import grad_accum_multi

    gen = torch.Generator(device=DEV).manual_seed(5)
    first = _grads(dtype, gen)
    # garbage in the accumulators: INIT must overwrite it, not add to it
    accs = [torch.full_like(g, 1e30, dtype=torch.float32) for g in first]
    assert accs[-1].stride() == first[-1].stride()
    want = [a.clone() for a in accs]
    for mode in ["init", "add", "add", "fold"]:
        gs = first if mode == "init" else _grads(dtype, gen)
        g0 = [g.clone() for g in gs]
        outs = [None] * len(gs)
        if mode == "fold":
            outs = gs if in_place else [torch.full_like(g, -7.0) for g in gs]
        grad_accum_multi(list(zip(gs, accs, outs)), mode)
        for i, g in enumerate(g0):
            want[i], out = ref_step(mode, g, want[i], dtype)
            assert same_bits(accs[i], want[i]), (mode, i)
            if mode == "fold":
                assert same_bits(outs[i], out), (mode, i)
                assert in_place or same_bits(gs[i], g)  # a separate output leaves the gradient alone
            else:
                assert same_bits(gs[i], g), (mode, i)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_null_gradient_records(dtype):
    """One tensor of the table (a different one per mode) has no gradient:
    zeros / unchanged / cast(acc); the others are unaffected by it."""
    from pytorch_operator_1_amd.ops.optim import grad_accum_multi

    gen = torch.Generator(device=DEV).manual_seed(6)
    n = len(_grads(dtype, gen))
    accs = [torch.full_like(g, 3.0, dtype=torch.float32) for g in _grads(dtype, gen)]
    want = [a.clone() for a in accs]
    for mode, missing in [("init", 3), ("add", 2), ("add", n - 1), ("fold", 3), ("fold", 0)]:
        gs = _grads(dtype, gen)
        gs[missing] = None
        outs = [torch.full_like(a, -7.0, dtype=dtype) if mode == "fold" else None for a in accs]
        grad_accum_multi(list(zip(gs, accs, outs)), mode)
        for i, g in enumerate(gs):
            want[i], out = ref_step(mode, g, want[i], dtype)
            assert same_bits(accs[i], want[i]), (mode, i)
            if mode == "fold":
                assert same_bits(outs[i], out), (mode, i)
    # an all-null table (no gradient dtype to go by) still initialises
    grad_accum_multi([(None, a, None) for a in accs], "init")
    assert all(a.abs().max().item() == 0.0 for a in accs)


def test_fp32_accumulation_is_real():
    """256 + 1 + 1 + 1 + 1 in bf16 gradients: 260 through the fp32
    accumulator, 256 as a bf16 running sum (257 rounds back to 256)."""
    from pytorch_operator_1_amd.ops.optim import grad_accum_multi

    n = 2048 + 5
    acc = torch.empty(n, device=DEV)
    one = torch.ones(n, device=DEV, dtype=torch.bfloat16)
    grad_accum_multi([(torch.full_like(one, 256.0), acc, None)], "init")
    for _ in range(3):
        grad_accum_multi([(one, acc, None)], "add")
    out = torch.empty_like(one)
    grad_accum_multi([(one, acc, out)], "fold")
    assert out.dtype == torch.bfloat16 and torch.equal(out, torch.full_like(one, 260.0))
    running = torch.full_like(one, 256.0)
    for _ in range(4):
        running += one
    assert torch.equal(running, torch.full_like(one, 256.0))


def test_layout_and_mode_are_checked():
    from pytorch_operator_1_amd.ops.optim import grad_accum_multi

    acc = torch.zeros(4, 6, device=DEV)
    g = torch.zeros(4, 6, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        grad_accum_multi([(g.t(), acc.t(), None)], "add")  # not dense
    with pytest.raises(ValueError):
        grad_accum_multi([(g[:2], acc, None)], "add")  # shapes differ
    with pytest.raises(ValueError):
        grad_accum_multi([(g, acc.bfloat16(), None)], "add")  # accumulator not fp32
    with pytest.raises(ValueError):
        grad_accum_multi([(g, acc, None)], "fold")  # fold needs an output
    with pytest.raises(ValueError):
        grad_accum_multi([(g, acc, None)], "sum")


# ---- GradBucketer -----------------------------------------------------------

class Toy(torch.nn.Module):
    def __init__(self, dtype, extra=False):
        super().__init__()
        shapes = SHAPES + ([(7,)] if extra else [])
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s, device=DEV, dtype=dtype)) for s in shapes])


def _cycle_consts(seed, n_micro, dtype):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [[torch.randn(s, device=DEV, generator=gen).to(dtype) for s in SHAPES] for _ in range(n_micro)]


def _fp32_sum(cs, dtype):
    total = cs[0].float()
    for c in cs[1:]:
        total = total + c.float()
    return total.to(dtype)


def _copy_mode_worker(port, q):
    import os

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    import torch.distributed as dist

    from pytorch_operator_1_amd.parallel.ddp import GradBucketer

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)
    calls = []
    real = dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    dist.all_reduce = counted
    dt = torch.bfloat16
    m = Toy(dt)
    bk = GradBucketer(m, bucket_mb=0.001, force_ddp=True, comm="rccl", accum_steps=3)
    problems = []

    def check(cond, what):
        if not cond:
            problems.append(what)

    check(bk.mode == "copy" and len(bk.buckets) >= 3, f"mode {bk.mode}, {len(bk.buckets)} buckets")
    check(bk.grad_scale == 1 / 3, f"grad_scale {bk.grad_scale}")
    check(bk.accum_bytes() == 4 * sum(p.numel() for p in m.ps), f"accum_bytes {bk.accum_bytes()}")
    flat = bk.flat[dt]
    for cycle in range(2):  # the second cycle's INIT must discard the first cycle's sums
        consts = _cycle_consts(20 + cycle, 3, dt)
        calls.clear()
        for k in range(3):
            check(bk.at_boundary == (k == 2), f"at_boundary wrong at micro-batch {k}")
            sum((p * c).sum() for p, c in zip(m.ps, consts[k])).backward()
            bk.finish()
            if k < 2:
                check(all(p.grad is None for p in m.ps), f"cycle {cycle} micro-batch {k}: a grad is set")
                check(not calls, f"cycle {cycle} micro-batch {k}: {len(calls)} collectives before the boundary")
        check(len(calls) == len(bk.buckets), f"cycle {cycle}: {len(calls)} collectives for {len(bk.buckets)} buckets")
        for i, p in enumerate(m.ps):
            want = _fp32_sum([consts[k][i] for k in range(3)], dt)
            inside = (p.grad is not None and p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr())
            check(inside, f"cycle {cycle} param {i}: grad is not a view of the flat buffer")
            check(inside and same_bits(p.grad, want), f"cycle {cycle} param {i}: wrong sum")
        bk.release()
    torch.cuda.synchronize()
    q.put(problems)
    dist.destroy_process_group()


def test_bucketer_copy_mode_accumulates_then_reduces():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_copy_mode_worker, args=(port, q))
    p.start()
    problems = collect(q, [p], 1)[0]
    p.join(60)
    assert p.exitcode == 0
    assert problems == []


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_bucketer_none_mode_accumulates_in_place(dtype):
    from pytorch_operator_1_amd.parallel.ddp import GradBucketer

    m = Toy(dtype, extra=True)  # the extra parameter is never in the loss
    bk = GradBucketer(m, accum_steps=3)
    assert bk.mode == "none" and bk.grad_scale == 1 / 3
    assert bk.accum_bytes() == 4 * sum(p.numel() for p in m.ps)
    ps = list(m.ps)
    for cycle in range(2):
        consts = _cycle_consts(30 + cycle, 3, dtype)
        for k in range(3):
            assert bk.at_boundary == (k == 2)
            sum((p * c).sum() for p, c in zip(ps, consts[k])).backward()
            bk.finish()
            if k < 2:
                assert all(p.grad is None for p in ps)
        for i, p in enumerate(ps[:-1]):
            assert same_bits(p.grad, _fp32_sum([consts[k][i] for k in range(3)], dtype)), (cycle, i)
        assert ps[-1].grad.dtype == dtype and ps[-1].grad.abs().max().item() == 0.0
        bk.release()


def test_view_mode_and_captured_step_refuse_accumulation():
    from pytorch_operator_1_amd.parallel.ddp import GradBucketer
    from pytorch_operator_1_amd.train.bench_models import ResNetTrainer

    with pytest.raises(ValueError, match="copy"):
        GradBucketer(Toy(torch.bfloat16), mode="view", accum_steps=2)
    with pytest.raises(ValueError):
        GradBucketer(Toy(torch.bfloat16), accum_steps=0)
    # refused by the argument check, before the model is built
    with pytest.raises(ValueError, match="grad_accum_steps"):
        ResNetTrainer(torch.device(DEV), batch_size=2, image_size=32, graph=True, grad_accum_steps=2)


# ---- trainers ---------------------------------------------------------------

def _first_step(tr):
    tr.step()
    return tr.last_loss(), tr.last_grad_norm()


@pytest.fixture(scope="module")
def llama_first_steps():
    """The first optimizer step of llama3-tiny on the same 4 rows: (a) one
    batch of 4, (b) 4 micro-batches of 1, (c) one batch of 4 again, and the
    fp32 ``impl="torch"`` model with (a)'s initial weights as the reference."""
    from pytorch_operator_1_amd.models.llama import Llama
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    dev = torch.device(DEV)
    kw = dict(model="llama3-tiny", seq_len=128, max_grad_norm=INF, seed=3)
    a = LlamaTrainer(dev, batch_size=4, **kw)
    ref = Llama(a.cfg, impl="torch", device=dev, dtype=torch.float32)
    ref.load_state_dict(a.model.state_dict())
    loss = ref(a.tokens, a.labels)
    loss.backward()
    ref_loss = loss.item()
    ref_norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ref.parameters())).item()
    b = LlamaTrainer(dev, batch_size=1, grad_accum_steps=4, **kw)
    c = LlamaTrainer(dev, batch_size=4, **kw)
    same_init = all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    return dict(a=a, b=b, c=c, same_init=same_init, ref=(ref_loss, ref_norm),
                ra=_first_step(a), rb=_first_step(b), rc=_first_step(c))


def test_trainer_bookkeeping(llama_first_steps):
    r = llama_first_steps
    a, b = r["a"], r["b"]
    assert r["ra"] == r["rc"]  # a repeat is bitwise: the comparison below means something
    assert r["same_init"]
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.labels, b.labels)
    assert [t.shape[0] for t, _ in b._micro] == [1, 1, 1, 1]
    assert torch.equal(torch.cat([t for t, _ in b._micro]), a.tokens)
    assert a.samples_per_step() == b.samples_per_step() == 4 * 128
    assert b.steps_done == 1 and b.opt._step == 1
    assert b.describe()["grad_accum"].startswith("4 micro-batches") and a.describe()["grad_accum"] == "off"
    assert b.bucketer.accum_bytes() == 4 * sum(p.numel() for p in b.model.parameters())
    assert all(p.grad is None for p in b.model.parameters())  # released after the step


def test_trainer_accumulation_matches_one_batch(llama_first_steps):
    """(b) against (a) cannot be bitwise: the weight-gradient GEMMs sum over
    other token counts before rounding to bf16.  With e_a the relative error
    of (a) against the fp32 model, (b)'s may be at most 2 * e_a + 2^-9 (twice:
    rounding at other points of an equally precise computation; 2^-9: half a
    bf16 ulp, should e_a happen to be tiny)."""
    r = llama_first_steps
    for what, ref, va, vb in zip(("loss", "grad_norm"), r["ref"], r["ra"], r["rb"]):
        e_a, e_b = abs(va - ref) / abs(ref), abs(vb - ref) / abs(ref)
        print(f"{what}: ref {ref!r} a {va!r} b {vb!r} e_a {e_a:.3e} e_b {e_b:.3e} bound {2 * e_a + 2.0 ** -9:.3e}")
        assert e_b <= 2 * e_a + 2.0 ** -9, what


def test_one_step_is_the_path_without_the_keyword():
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    dev = torch.device(DEV)
    losses = []
    for kw in ({}, {"grad_accum_steps": 1}):
        tr = LlamaTrainer(dev, model="llama3-tiny", batch_size=2, seq_len=128, seed=5, **kw)
        seq = []
        for _ in range(3):
            tr.step()
            seq.append(tr.last_loss())
        losses.append(seq)
        assert tr.bucketer.accum_bytes() == 0 and tr.bucketer.grad_scale == 1.0
    assert losses[0] == losses[1]
