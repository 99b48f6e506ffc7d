"""Label smoothing and z-loss of the LM loss on the CPU path: the value the
torch model computes, the unchanged default path, the ``--label-smoothing`` /
``--z-loss`` flags of train/lm.py and their log / metrics output."""
import json
import math
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


def test_model_loss_matches_fp64_formulas():
    from pytorch_operator_1_amd.models.llama import Llama, synthetic_tokens

    eps, zc = 0.1, 1e-2
    torch.manual_seed(0)
    model = Llama("llama3-tiny", impl="torch", device="cpu", label_smoothing=eps, z_loss=zc)
    tok, lab = synthetic_tokens(2, 64, model.cfg.vocab_size, "cpu", seed=1)
    lab = lab.clone()
    lab[0, 3] = -100
    with torch.no_grad():
        loss = model(tok, lab)
        z = model(tok).reshape(-1, model.cfg.vocab_size).double()
    y = lab.reshape(-1)
    valid = y != -100
    lse = torch.logsumexp(z, dim=-1)
    zy = z.gather(1, y.clamp_min(0)[:, None])[:, 0]
    rows = (1 - eps) * (lse - zy) + eps * (lse - z.mean(-1)) + zc * lse ** 2
    want = (rows * valid).sum() / valid.sum()
    want_z = zc * (lse ** 2 * valid).sum() / valid.sum()
    assert abs(loss.item() - want.item()) < 1e-5 * want.item()
    assert not model.last_z_loss.requires_grad
    assert abs(model.last_z_loss.item() - want_z.item()) < 1e-5 * want_z.item()
    # z_loss off: no z part is kept
    plain = Llama("llama3-tiny", impl="torch", device="cpu", label_smoothing=eps)
    plain(tok, lab)
    assert plain.last_z_loss is None


def test_model_rejects_out_of_range():
    from pytorch_operator_1_amd.models.llama import Llama

    for kw in ({"label_smoothing": 1.0}, {"label_smoothing": -0.1}, {"z_loss": -1.0}):
        with pytest.raises(ValueError):
            Llama("llama3-tiny", impl="torch", device="cpu", **kw)


def test_trainer_zero_is_default_path():
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    dev = torch.device("cpu")
    a = LlamaTrainer(dev, model="llama3-tiny", batch_size=2, seq_len=64)
    b = LlamaTrainer(dev, model="llama3-tiny", batch_size=2, seq_len=64, label_smoothing=0.0, z_loss=0.0)
    for t in (a, b):
        t.run(2)
    assert a.last_loss() == b.last_loss()
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)
    for t in (a, b):
        assert t.last_z_loss() is None and t.describe()["loss"] == "CE"


def test_trainer_z_loss_mean_over_micro_batches():
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    tr = LlamaTrainer(torch.device("cpu"), model="llama3-tiny", batch_size=1, seq_len=64, label_smoothing=0.1,
                      z_loss=1e-4, grad_accum_steps=2)
    assert tr.last_z_loss() is None  # before the first step
    with torch.no_grad():
        parts = []
        for tok, lab in tr._micro:
            tr.model(tok, lab)
            parts.append(tr.model.last_z_loss.item())
    tr.step()
    assert tr.describe()["loss"] == "CE label_smoothing=0.1 z_loss=0.0001"
    want = sum(parts) / 2
    assert want > 0 and abs(tr.last_z_loss() - want) < 1e-5 * want


def test_lm_flags_log_z_loss(tmp_path):
    out, train = _run(["--label-smoothing", "0.1", "--z-loss", "1e-4"], tmp_path, "opts")
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 2 and all("z_loss=" in l for l in lines), out
    assert len(train) == 2
    for e in train:
        assert e["z_loss"] > 0 and math.isfinite(e["z_loss"]) and e["z_loss"] < e["loss"]


def test_lm_without_flags_is_unchanged(tmp_path):
    out, train = _run([], tmp_path, "plain")
    assert "z_loss" not in out
    assert len(train) == 2 and all("z_loss" not in e for e in train)
    out0, train0 = _run(["--label-smoothing", "0", "--z-loss", "0"], tmp_path, "zero")
    assert "z_loss" not in out0 and all("z_loss" not in e for e in train0)
    assert _final(out0) == _final(out)


def test_parse_args():
    from pytorch_operator_1_amd.train import lm

    a = lm.parse_args([])
    assert a.label_smoothing == 0.0 and a.z_loss == 0.0
    a = lm.parse_args(["--model", "resnet50", "--label-smoothing", "0.1"])
    assert a.label_smoothing == 0.1
    for bad in (["--label-smoothing", "1"], ["--label-smoothing", "-0.1"], ["--z-loss", "-1"],
                ["--model", "resnet50", "--z-loss", "1e-4"]):
        with pytest.raises(SystemExit):
            lm.parse_args(bad)


def test_resnet_label_smoothing():
    from pytorch_operator_1_amd.train.bench_models import ResNetTrainer

    dev = torch.device("cpu")
    tr = ResNetTrainer(dev, batch_size=2, image_size=32, label_smoothing=0.1)
    assert "label_smoothing=0.1" in tr.describe()["loss"]
    tr.step()
    assert math.isfinite(tr.last_loss())
    assert ResNetTrainer(dev, batch_size=2, image_size=32).describe()["loss"] == "CE"
    with pytest.raises(ValueError):
        ResNetTrainer(dev, batch_size=2, image_size=32, label_smoothing=1.0)
