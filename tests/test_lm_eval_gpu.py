"""Held-out evaluation on the device (``pto_ce_eval`` / ``pto_eval_accum``
behind ``EvalAccumulator``): per-row NLL and label rank against the torch
formulas on the same bf16 values (exact counts, ties at the label
included), the fp64 record, chunked accumulation, labels outside the
vocabulary, and the path up through ``Llama.evaluate``,
``LlamaTrainer.evaluate`` and the ``--eval-*`` flags of train/lm.py.
Inputs and planted rows: tests/lm_eval_util.py."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from lm_eval_util import K, M, PLANTED_RANKS, close, ignore_index, planted_case, ref_rows, rows_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 8: the smallest legal row, one thread has data; 1000: fewer 16-byte chunks than
# threads; 2056: 257 chunks, one thread takes a second iteration; 128256: Llama-3
VOCABS = [8, 1000, 2056, 128256]

_dev = {}


def _case(V):
    """The planted case on the device with its reference rows, made once and never written."""
    if V not in _dev:
        z, y = planted_case(V)
        z, y = z.to(DEV), y.to(DEV)
        _dev[V] = (z, y) + ref_rows(z, y, ignore_index(V))
    return _dev[V]


def _acc(V, **kw):
    from pytorch_operator_1_amd.ops.llm import EvalAccumulator

    return EvalAccumulator(DEV, topk=K, ignore_index=ignore_index(V), **kw)


@pytest.mark.parametrize("V", VOCABS)
def test_rows_and_record(V):
    z, y, want_loss, want_rank, valid = _case(V)
    acc = _acc(V)
    row_loss, row_rank = acc.update(z, y, return_rows=True)
    assert row_loss.dtype == torch.float32 and row_rank.dtype == torch.int32
    ties = int(((z == z.gather(1, y.clamp_min(0)[:, None])).sum(1) > 1)[valid].sum())
    err = ((row_loss - want_loss).abs() / want_loss.clamp_min(1.0)).max().item()
    print(f"V={V}: rows with a tie at the label {ties}/{int(valid.sum())}, rank mismatches "
          f"{int((row_rank.long() != want_rank).sum())}, max row loss err/scale {err:.3e}")
    assert torch.equal(row_rank.long(), want_rank)
    assert row_rank[5].item() == -1 and row_loss[5].item() == 0.0
    for r, want in PLANTED_RANKS.items():
        assert row_rank[r].item() == want, (r, row_rank[r].item())
    assert torch.equal(row_rank[valid] == 0, z[valid].float().argmax(1) == y[valid])
    assert rows_close(row_loss, want_loss)
    res = acc.result()
    n = int(valid.sum())
    want_ce = F.cross_entropy(z.float(), y, ignore_index=ignore_index(V)).item()
    print(f"  record: {res}, F.cross_entropy {want_ce:.6f}")
    assert res["tokens"] == n == M - 1 and res["k"] == K
    assert res["top1"] == int((want_rank == 0).sum()) / n
    assert res["topk"] == int(((want_rank >= 0) & (want_rank < K)).sum()) / n
    assert res["top1"] >= 2 / n and res["topk"] >= res["top1"] + 1 / n  # the planted rows count
    assert close(res["loss"], want_ce)
    assert res["ppl"] == math.exp(res["loss"])


@pytest.mark.parametrize("V", VOCABS)
def test_accumulation_is_exact_and_repeatable(V):
    z, y = _case(V)[:2]
    one = _acc(V)
    one.update(z, y)
    parts = _acc(V)
    for a, b in ((0, 40), (40, 80), (80, 96)):
        parts.update(z[a:b], y[a:b])
    o, p = one.acc.tolist(), parts.acc.tolist()
    print(f"V={V}: one call {o}, 40+40+16 {p}")
    assert o[1:] == p[1:] and o[1] == M - 1 and o[4] == 0
    assert abs(o[0] - p[0]) <= 1e-12 * abs(o[0])  # identical row losses, another fp64 order
    again = _acc(V)
    again.update(z, y)
    assert torch.equal(again.acc, one.acc)  # bitwise
    again.update(z, y)
    assert again.result()["tokens"] == 2 * (M - 1)
    again.reset()
    assert torch.equal(again.acc, torch.zeros(5, device=DEV, dtype=torch.float64))
    empty = again.result()
    assert empty["tokens"] == 0 and math.isnan(empty["loss"]) and math.isnan(empty["ppl"])
    assert empty["top1"] == 0 and empty["topk"] == 0


@pytest.mark.parametrize("V", VOCABS)
def test_labels_outside_the_vocabulary_are_counted_not_read(V):
    """Nothing is provoked: the kernel writes -2 for such a row and never forms z[y]."""
    z, y = _case(V)[:2]
    base_loss, base_rank = _acc(V).update(z, y, return_rows=True)
    bad = y.clone()
    bad[10], bad[11] = V, -7
    acc = _acc(V)
    row_loss, row_rank = acc.update(z, bad, return_rows=True)
    assert row_rank[10].item() == -2 and row_rank[11].item() == -2
    assert row_loss[10].item() == 0.0 and row_loss[11].item() == 0.0
    keep = torch.ones(M, dtype=torch.bool, device=DEV)
    keep[10] = keep[11] = False
    assert torch.equal(row_rank[keep], base_rank[keep]) and torch.equal(row_loss[keep], base_loss[keep])
    assert acc.acc.tolist()[4] == 2.0 and acc.acc.tolist()[1] == M - 3
    with pytest.raises(ValueError, match="2"):
        acc.result()


def test_argument_errors():
    from pytorch_operator_1_amd.ops.llm import EvalAccumulator

    z, y = _case(1000)[:2]
    acc = EvalAccumulator(DEV)
    with pytest.raises(TypeError):
        acc.update(z.float(), y)
    with pytest.raises(RuntimeError):
        acc.update(torch.zeros(4, 1004, device=DEV, dtype=torch.bfloat16),
                   torch.zeros(4, device=DEV, dtype=torch.int64))  # V % 8 != 0: refused by the launcher
    with pytest.raises(ValueError):
        acc.update(z, y[:-1])
    rows = acc.update(z[:0], y[:0], return_rows=True)  # M = 0: nothing is launched
    assert rows[0].numel() == 0 and rows[1].numel() == 0
    assert torch.equal(acc.acc, torch.zeros(5, device=DEV, dtype=torch.float64))
    assert acc.result()["tokens"] == 0


@pytest.mark.parametrize("V", VOCABS)
def test_hip_matches_the_cpu_path(V):
    from pytorch_operator_1_amd.ops.llm import EvalAccumulator

    z, y = _case(V)[:2]
    hip = _acc(V)
    h_loss, h_rank = hip.update(z.view(4, 24, V), y.view(4, 24), return_rows=True)
    cpu = EvalAccumulator("cpu", topk=K, ignore_index=ignore_index(V))
    c_loss, c_rank = cpu.update(z.cpu(), y.cpu(), return_rows=True)
    assert torch.equal(h_rank.cpu(), c_rank)
    assert rows_close(h_loss.cpu(), c_loss)
    a, b = hip.result(), cpu.result()
    assert (a["tokens"], a["top1"], a["topk"], a["k"]) == (b["tokens"], b["top1"], b["topk"], b["k"])
    assert close(a["loss"], b["loss"])


def test_llama_evaluate_matches_formulas_on_its_logits():
    from pytorch_operator_1_amd.models.llama import Llama, synthetic_tokens
    from pytorch_operator_1_amd.ops.llm import EvalAccumulator

    torch.manual_seed(5)
    model = Llama("llama3-tiny", impl="hip", device=DEV, label_smoothing=0.1, z_loss=1e-2)
    model.train()
    tok, lab = synthetic_tokens(2, 128, model.cfg.vocab_size, DEV, seed=1)
    lab = lab.clone()
    lab[0, 3] = -100
    with torch.no_grad():
        z = model(tok).reshape(-1, model.cfg.vocab_size)
    want_loss, want_rank, valid = ref_rows(z, lab.reshape(-1), -100)
    n = int(valid.sum())
    acc = EvalAccumulator(DEV, topk=K)
    model.evaluate(tok, lab, acc, head_chunk=None)
    res = acc.result()
    want_ce = F.cross_entropy(z.float(), lab.reshape(-1)).item()
    print(f"one chunk: {res}, formulas on model(tokens): loss {want_ce:.6f}")
    assert res["tokens"] == n == 255
    assert res["top1"] == int((want_rank == 0).sum()) / n
    assert res["topk"] == int(((want_rank >= 0) & (want_rank < K)).sum()) / n
    assert close(res["loss"], want_ce)  # plain NLL: neither the model's smoothing nor its z-loss
    acc = EvalAccumulator(DEV, topk=K)
    model.evaluate(tok, lab, acc, head_chunk=96)  # 256 rows -> 96 + 96 + 64
    chunked = acc.result()
    print(f"head_chunk=96: {chunked}")
    assert chunked["tokens"] == n and close(chunked["loss"], res["loss"])
    assert model.training and model.last_z_loss is None
    assert all(p.grad is None for p in model.parameters())


def test_trainer_evaluate_leaves_training_state_alone():
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    tr = LlamaTrainer(torch.device(DEV), model="llama3-tiny", batch_size=2, seq_len=128, lr=3e-3)
    tr.run(16)
    state = {k: v.clone() for k, v in tr.checkpoint_tensors().items()}
    wts = [m.weight_t.clone() for m in tr.model.linear_modules()]
    steps, cpu_rng, dev_rng = tr.steps_done, torch.get_rng_state(), torch.cuda.get_rng_state()
    had_grad = [p.grad is not None for p in tr.model.parameters()]
    train = tr.evaluate(split="train")
    held = tr.evaluate(batches=2)
    print(f"train split {train}\nheld out {held}")
    assert tr.last_eval() is held
    assert train["tokens"] == 2 * 128 and held["tokens"] == 2 * 2 * 128 and held["k"] == 5
    now = tr.checkpoint_tensors()
    assert set(now) == set(state) and all(torch.equal(now[k], state[k]) for k in state)
    assert len(wts) > 0 and all(torch.equal(m.weight_t, w) for m, w in zip(tr.model.linear_modules(), wts))
    assert tr.steps_done == steps == 16
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), dev_rng)
    assert tr.model.training
    assert [p.grad is not None for p in tr.model.parameters()] == had_grad  # no parameter gained a .grad
    with torch.no_grad():
        want = sum(tr.model(t, l).item() for t, l in tr._micro) / len(tr._micro)
    assert close(train["loss"], want)
    assert held["loss"] > train["loss"]  # the training batch is memorised, fresh tokens are not
    tr.step()
    assert tr.steps_done == 17 and math.isfinite(tr.last_loss())


def test_lm_cli_evaluates_on_gpu(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = root
    cmd = [sys.executable, "-m", "pytorch_operator_1_amd.train.lm", "--model", "llama3-tiny", "--seq-len", "128",
           "--steps", "4", "--log-interval", "2", "--eval-interval", "2", "--eval-batches", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("eval step")]
    print("\n".join(lines))
    assert len(lines) == 2, r.stdout
    for line, step in zip(lines, (2, 4)):
        m = re.fullmatch(r"eval step (\d+)\tloss=(\S+)\tppl=(\S+)\ttop1=(\S+)\ttop5=(\S+)\ttokens=(\d+)", line)
        assert m and int(m.group(1)) == step and int(m.group(6)) == 512, line
        assert math.isfinite(float(m.group(2)))
