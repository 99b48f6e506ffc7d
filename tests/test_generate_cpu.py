"""KV-cache generation on the CPU path: the torch implementations of the
decode ops (the reference of the GPU tests), ``Llama.prefill`` /
``decode_step`` / ``generate`` with ``impl="torch"``, ``LlamaTrainer.sample``
and the ``--sample-*`` flags of train/lm.py."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from decode_util import SAMPLE_SETTINGS, relerr, sample_batch, sample_logits, teacher_forced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_LINE = re.compile(r"sample step (\d+)\tprompt=\[([\d, ]*)\]\ttokens=\[([\d, ]*)\]")


def _tiny():
    from pytorch_operator_1_amd.models.llama import Llama

    torch.manual_seed(0)
    return Llama("llama3-tiny", impl="torch", device="cpu", dtype=torch.float32)


def test_cached_decode_matches_full_forward():
    """fp32, impl="torch": the logits of prefill + cached decode steps equal
    the full forward's at the same positions up to fp32 reassociation."""
    model = _tiny()
    model.train()
    lens = [5, 20, 12]
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, model.cfg.vocab_size, (3, 20), generator=g)
    out, logits = model.generate(prompts, lens, max_new_tokens=9, return_logits=True)
    assert out.shape == (3, 9) and out.dtype == torch.int64 and logits.shape == (3, 9, model.cfg.vocab_size)
    assert torch.equal(out, logits.argmax(-1))
    want = teacher_forced(model, prompts, lens, out)
    for b in range(3):
        e = relerr(logits[b], want[b])
        assert e < 1e-4, (b, e)
    # the padding of a short prompt is harmless: the row alone gives the same tokens
    alone = model.generate(prompts[:1, :5], max_new_tokens=9)
    assert torch.equal(alone, out[:1])
    # sampling is a function of the seed
    a = model.generate(prompts, lens, max_new_tokens=6, temperature=0.8, top_k=20, seed=3)
    b = model.generate(prompts, lens, max_new_tokens=6, temperature=0.8, top_k=20, seed=3)
    c = model.generate(prompts, lens, max_new_tokens=6, temperature=0.8, top_k=20, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert model.training and model.last_z_loss is None and all(p.grad is None for p in model.parameters())


def test_rope_kv_append_and_attention_decode_torch():
    from pytorch_operator_1_amd.ops import llm

    B, H, Hkv, D, max_len = 3, 4, 2, 16, 10
    torch.manual_seed(0)
    cos, sin = llm.rope_tables(max_len, D, 10000.0, "cpu")
    lens = torch.tensor([0, 7, 10], dtype=torch.int32)  # the last row is full
    kc, vc = torch.randn(B, Hkv, max_len, D), torch.randn(B, Hkv, max_len, D)
    k0, v0 = kc.clone(), vc.clone()
    qkv = torch.randn(B, (H + 2 * Hkv) * D)
    q0 = qkv.clone()
    assert llm.rope_kv_append(qkv, cos, sin, kc, vc, lens, H, Hkv) is qkv
    x = q0.view(B, H + 2 * Hkv, D)
    for b, p in ((0, 0), (1, 7)):
        c, s = torch.cat([cos[p], cos[p]]), torch.cat([sin[p], sin[p]])
        rot = x[b, :H + Hkv] * c + torch.cat([-x[b, :H + Hkv, D // 2:], x[b, :H + Hkv, :D // 2]], -1) * s
        torch.testing.assert_close(qkv.view(B, -1, D)[b, :H], rot[:H])
        torch.testing.assert_close(kc[b, :, p], rot[H:])
        assert torch.equal(vc[b, :, p], x[b, H + Hkv:])
    assert torch.equal(qkv[2], q0[2])  # a full row is left alone entirely
    touched = torch.zeros(B, Hkv, max_len, D, dtype=torch.bool)
    touched[0, :, 0] = touched[1, :, 7] = True
    assert torch.equal(kc[~touched], k0[~touched]) and torch.equal(vc[~touched], v0[~touched])
    # attention over the valid prefix only: NaN in the tail must not show
    lens2 = torch.tensor([0, 1, 8], dtype=torch.int32)
    kn, vn = kc.clone(), vc.clone()
    for b, n in enumerate(lens2.tolist()):
        kn[b, :, n:] = float("nan")
        vn[b, :, n:] = float("nan")
    o = llm.attention_decode(qkv, kn, vn, lens2, H, Hkv).view(B, H, D)
    assert torch.isfinite(o).all() and torch.equal(o[0], torch.zeros(H, D))
    torch.testing.assert_close(o[1], vn[1, :, 0].repeat_interleave(H // Hkv, 0))
    q = qkv.view(B, -1, D)[2, :H]
    k = kc[2, :, :8].repeat_interleave(H // Hkv, 0)
    v = vc[2, :, :8].repeat_interleave(H // Hkv, 0)
    want = torch.softmax(torch.einsum("hd,hkd->hk", q, k) * D ** -0.5, -1)[:, :, None].mul(v).sum(1)
    torch.testing.assert_close(o[2], want)
    assert not llm.attention_decode_supported(8, 2, 32) and llm.attention_decode_supported(32, 8, 128)
    assert llm.attention_decode_supported(4, 2, 64) and not llm.attention_decode_supported(16, 1, 128)


@pytest.mark.parametrize("V", [8, 1000, 2048])
def test_torch_sample_rules(V):
    from pytorch_operator_1_amd.ops import llm

    z, planted = sample_logits(V)
    tok = llm.sample(z)
    assert tok.dtype == torch.int64 and torch.equal(tok, z.float().argmax(-1))
    for r, want in planted.items():
        assert tok[r].item() == want
    for T, k in SAMPLE_SETTINGS:
        zz, u, want, kept = sample_batch(z, T, k)
        got = llm.sample(zz, u, temperature=T, top_k=k)
        assert torch.equal(got, want), (T, k)
        if 1 < k < V:
            assert all(n >= k for n in kept) and kept[0] > k  # the planted tie at the threshold is kept
    # bookkeeping: out[b, step], done rows emit eos, a row that draws eos sets done, advance
    B = z.shape[0]
    eos = int(tok[0])
    out = torch.full((B, 3), -1, dtype=torch.int64)
    cur = torch.zeros(B, dtype=torch.int64)
    step = torch.tensor([1], dtype=torch.int32)
    done = torch.tensor([0, 0, 1, 0], dtype=torch.int32)
    lens = torch.tensor([4, 5, 6, 7], dtype=torch.int32)
    assert llm.sample(z, cur=cur, out=out, step=step, done=done, eos_id=eos, lens=lens, advance=True) is cur
    want = tok.clone()
    want[2] = eos
    assert torch.equal(cur, want) and torch.equal(out[:, 1], want)
    assert (out[:, 0] == -1).all() and (out[:, 2] == -1).all()
    assert done.tolist() == [1, int(tok[1]) == eos, 1, int(tok[3]) == eos]
    assert step.item() == 2 and lens.tolist() == [5, 6, 7, 8]
    with pytest.raises(ValueError):
        llm.sample(z, temperature=0.5)  # no uniforms


def test_generate_refuses_what_does_not_fit():
    from pytorch_operator_1_amd.models.llama import KVCache

    model = _tiny()  # max_seq_len 256
    prompts = torch.zeros(2, 200, dtype=torch.int64)
    with pytest.raises(ValueError, match="max_seq_len"):
        model.generate(prompts, max_new_tokens=57)
    with pytest.raises(ValueError, match="max_seq_len"):
        model.generate(prompts[:, :100], [100, 60], max_new_tokens=157)
    with pytest.raises(ValueError, match="cache"):
        model.generate(prompts[:, :8], max_new_tokens=9, cache=KVCache(model.cfg, 2, 16, "cpu", torch.float32))
    with pytest.raises(ValueError):
        model.generate(prompts[:, :8], [8, 9], max_new_tokens=2)
    with pytest.raises(ValueError):
        model.generate(prompts[:, :8], max_new_tokens=0)
    cache = KVCache(model.cfg, 2, 17, "cpu", torch.float32)
    out = model.generate(prompts[:, :8], [8, 3], max_new_tokens=9, cache=cache)  # exactly fits
    assert out.shape == (2, 9) and cache.lens.tolist() == [16, 11] and cache.step.item() == 9


def test_eos_rows_keep_emitting_eos():
    model = _tiny()
    prompts = torch.arange(12).reshape(2, 6)
    free = model.generate(prompts, max_new_tokens=8)
    eos = int(free[0, 2])
    out = model.generate(prompts, max_new_tokens=8, eos_id=eos)
    first = (free[0] == eos).nonzero()[0, 0].item()
    assert torch.equal(out[0, :first + 1], free[0, :first + 1]) and (out[0, first:] == eos).all()
    if not (free[1] == eos).any():
        assert torch.equal(out[1], free[1])


def test_trainer_sample_and_parse_args():
    from pytorch_operator_1_amd.train import lm
    from pytorch_operator_1_amd.train.bench_models import LlamaTrainer

    tr = LlamaTrainer(torch.device("cpu"), model="llama3-tiny", batch_size=2, seq_len=32, lr=3e-3)
    tr.step()
    state = {k: v.clone() for k, v in tr.checkpoint_tensors().items()}
    prompt, tokens = tr.sample(prompt_len=8, new_tokens=5)
    assert prompt == tr._heldout_batches(1)[0][0][0, :8].tolist()
    assert isinstance(tokens, list) and len(tokens) == 5 and all(0 <= t < tr.cfg.vocab_size for t in tokens)
    assert tr.sample(prompt_len=8, new_tokens=5) == (prompt, tokens)
    now = tr.checkpoint_tensors()
    assert all(torch.equal(now[k], state[k]) for k in state) and tr.model.training
    with pytest.raises(ValueError):
        tr.sample(prompt_len=33)
    a = lm.parse_args([])
    assert (a.sample_interval, a.sample_tokens, a.sample_prompt_len, a.temperature, a.top_k, a.sample_seed) == \
        (0, 32, 16, 0.0, 0, 0)
    a = lm.parse_args(["--model", "llama3-mini", "--sample-interval", "2", "--sample-tokens", "4", "--top-k", "5",
                       "--temperature", "0.5", "--sample-seed", "9", "--sample-prompt-len", "3"])
    assert (a.sample_interval, a.sample_tokens, a.sample_prompt_len, a.temperature, a.top_k, a.sample_seed) == \
        (2, 4, 3, 0.5, 5, 9)
    assert lm.parse_args(["--model", "resnet50"]).sample_interval == 0
    for bad in (["--model", "resnet50", "--sample-interval", "2"], ["--model", "resnet50", "--sample-tokens", "4"],
                ["--model", "resnet50", "--temperature", "0.5"], ["--model", "resnet50", "--top-k", "3"],
                ["--model", "resnet50", "--sample-seed", "1"], ["--model", "resnet50", "--sample-prompt-len", "4"],
                ["--sample-interval", "-1"], ["--sample-tokens", "0"], ["--temperature", "-1"], ["--top-k", "-2"],
                ["--sample-interval", "1", "--seq-len", "8", "--sample-prompt-len", "9"]):
        with pytest.raises(SystemExit):
            lm.parse_args(bad)


def _run(extra, tmp_path, name):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    metrics = tmp_path / f"{name}.jsonl"
    env.update(PYTHONPATH=ROOT, OMP_NUM_THREADS="2", PTO_METRICS_FILE=str(metrics))
    cmd = [sys.executable, "-m", "pytorch_operator_1_amd.train.lm", "--no-cuda", "--model", "llama3-tiny", "--steps",
           "3", "--log-interval", "3", "--seq-len", "32"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, [json.loads(l) for l in metrics.read_text().splitlines()]


def test_lm_cli_sample_lines_and_metrics(tmp_path):
    off, ev_off = _run([], tmp_path, "off")
    assert "sample step" not in off and not [e for e in ev_off if e["event"] == "sample"]
    args = ["--sample-interval", "2", "--sample-tokens", "6", "--sample-prompt-len", "8", "--temperature", "0.9",
            "--top-k", "40", "--sample-seed", "5"]
    out, events = _run(args, tmp_path, "on")
    lines = SAMPLE_LINE.findall(out)
    assert [l[0] for l in lines] == ["2", "3"], out  # every 2 steps, and once after the last
    evs = [e for e in events if e["event"] == "sample"]
    assert [e["step"] for e in evs] == [2, 3]
    for e, l in zip(evs, lines):
        toks = [int(t) for t in l[2].split(",")]
        assert len(l[1].split(",")) == 8 and len(toks) == 6 and all(0 <= t < 1024 for t in toks)
        assert e["tokens"] == toks and e["seed"] == 5 and e["top_k"] == 40
        assert "samples_per_sec" not in e
    # sampling changes nothing training reads, and the same seed reproduces the samples
    assert re.search(r"final_loss=(\S+)", out).group(1) == re.search(r"final_loss=(\S+)", off).group(1)
    again, _ = _run(args, tmp_path, "again")
    assert SAMPLE_LINE.findall(again) == lines
