"""Global-norm gradient clipping on the CPU path: ``_TorchOpt`` semantics,
the ``--max-grad-norm`` flag of train/lm.py and its log / metrics output."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--no-cuda", "--model", "llama3-tiny", "--steps", "4", "--log-interval", "2", "--seq-len", "64"]


def _run(extra, tmp_path, name):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    metrics = tmp_path / f"{name}.jsonl"
    env.update(PYTHONPATH=ROOT, OMP_NUM_THREADS="2", PTO_METRICS_FILE=str(metrics))
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_1_amd.train.lm"] + ARGS + extra,
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    events = [json.loads(l) for l in metrics.read_text().splitlines()]
    return r.stdout, [e for e in events if e["event"] == "train"]


def _final(out):
    return re.search(r"final_loss=([0-9.]+)", out).group(1)


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _run([], tmp_path_factory.mktemp("plain"), "plain")


def test_torchopt_clip_matches_fp64():
    from pytorch_operator_1_amd.train.bench_models import _TorchOpt

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    params = list(model.parameters())
    p0 = [p.detach().double().clone() for p in params]
    grads = [torch.randn_like(p) * 3.0 for p in params]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    lr, scale, max_norm = 0.1, 0.5, 1.0
    opt = _TorchOpt(torch.optim.SGD(params, lr=lr))
    opt.step(grad_scale=scale, zero_grad=True, max_grad_norm=max_norm)
    g64 = [g.double() * scale for g in grads]
    norm = torch.sqrt(sum((g ** 2).sum() for g in g64))
    coef = min(1.0, max_norm / (norm.item() + 1e-6))
    assert coef < 1.0  # clipping is active in this case
    assert opt.grad_norm.shape == (1,) and opt.grad_norm.dtype == torch.float32
    assert abs(opt.grad_norm.item() - norm.item()) < 1e-6 * norm.item()
    assert abs(opt.clip_coef.item() - coef) < 1e-6 * coef
    for p, q, g in zip(params, p0, g64):
        assert torch.allclose(p.detach().double(), q - lr * coef * g, rtol=0, atol=1e-6)
        assert p.grad.abs().max().item() == 0.0
    # a bound above the norm leaves the gradients alone: coef == 1 exactly
    for p, g in zip(params, grads):
        p.grad = g.clone()
    opt.step(grad_scale=1.0, max_grad_norm=float("inf"))
    assert opt.clip_coef.item() == 1.0
    for p, g in zip(params, grads):
        assert torch.equal(p.grad, g)


def test_torchopt_default_has_no_norm():
    from pytorch_operator_1_amd.train.bench_models import _TorchOpt

    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.full((3,), 100.0)
    opt = _TorchOpt(torch.optim.SGD([p], lr=1.0))
    opt.step()
    assert opt.grad_norm is None and opt.clip_coef is None
    assert torch.equal(p.detach(), torch.full((3,), -99.0))


def test_lm_flag_logs_grad_norm(tmp_path):
    out, train = _run(["--max-grad-norm", "0.5"], tmp_path, "clip")
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 2 and all("grad_norm=" in l for l in lines), out
    assert len(train) == 2
    for e in train:
        assert e["grad_norm"] > 0 and 0 < e["clip_coef"] <= 1
        assert abs(e["clip_coef"] - min(1.0, 0.5 / (e["grad_norm"] + 1e-6))) < 1e-5


def test_lm_without_flag_is_unchanged(plain_run, tmp_path):
    out, train = plain_run
    assert "grad_norm" not in out
    assert len(train) == 2 and all("grad_norm" not in e and "clip_coef" not in e for e in train)
    # report-only (coef == 1 exactly) walks the same trajectory as the default path
    out_inf, train_inf = _run(["--max-grad-norm", "inf"], tmp_path, "inf")
    assert _final(out_inf) == _final(out)
    assert all(e["clip_coef"] == 1.0 and e["grad_norm"] > 0 for e in train_inf)


def test_trainer_none_is_default_path():
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    dev = torch.device("cpu")
    a = LlamaTrainer(dev, model="llama3-tiny", batch_size=2, seq_len=64)
    b = LlamaTrainer(dev, model="llama3-tiny", batch_size=2, seq_len=64, max_grad_norm=None)
    c = LlamaTrainer(dev, model="llama3-tiny", batch_size=2, seq_len=64, max_grad_norm=1e-3)
    for t in (a, b, c):
        t.run(2)
    assert a.last_grad_norm() is None and b.last_grad_norm() is None
    assert a.last_loss() == b.last_loss()
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)
    assert c.last_grad_norm() > 0 and c.last_clip_coef() < 1
    assert a.describe()["grad_clip"] == "off" and "0.001" in c.describe()["grad_clip"]


def test_parse_args_rejects_negative():
    from pytorch_operator_1_amd.train import lm

    assert lm.parse_args([]).max_grad_norm is None
    assert lm.parse_args(["--max-grad-norm", "inf"]).max_grad_norm == float("inf")
    with pytest.raises(SystemExit):
        lm.parse_args(["--max-grad-norm", "-1"])
