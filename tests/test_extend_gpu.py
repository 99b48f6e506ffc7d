"""Multi-token extend on the device (csrc/kernels/attn_extend.hip): the MFMA
extend attention against an fp32 reference, the T-token cache append against
``rope_``, and chunked prefill / ``Llama.extend`` / ``generate(prefill_chunk=)``
end to end."""
import pytest
import torch

from decode_util import relerr, teacher_forced

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 1, 128), (2, 8, 2, 128), (2, 4, 4, 128), (2, 8, 1, 128), (2, 4, 2, 64), (1, 8, 1, 64)]
HIST = (0, 1, 60, 63, 64, 65, 129, 1000)
SPLITS = (1, 2, 7, 16)  # 16: chunk 64 at max_len <= 1024, so 60 + 8 straddles a split and short rows leave splits empty
NAN = float("nan")


def reference(q, kc, vc, lens, n_new, T, H):
    """Per-row softmax over [0, lens[b] + t + 1) in fp32 on the same bf16 values; zeros for tokens that are not live."""
    B, Hkv, max_len, D = kc.shape
    out = torch.zeros(B, T, H, D, device=q.device)
    for b in range(B):
        n = max(0, min(n_new[b], max_len - lens[b]))
        if n == 0:
            continue
        end = lens[b] + n
        k = kc[b, :, :end].float().repeat_interleave(H // Hkv, 0)
        v = vc[b, :, :end].float().repeat_interleave(H // Hkv, 0)
        s = torch.einsum("thd,hkd->htk", q[b * T:b * T + n, :H * D].float().view(n, H, D), k) * D ** -0.5
        seen = torch.arange(end, device=q.device)[None, :] <= lens[b] + torch.arange(n, device=q.device)[:, None]
        out[b, :n] = torch.einsum("htk,hkd->thd", torch.softmax(s.masked_fill(~seen, -float("inf")), -1), v)
    return out.view(B * T, H * D)


def poisoned(kc, vc, lens, n_new):
    """NaN at and past lens[b] + live tokens: it must never be read."""
    kn, vn = kc.clone(), vc.clone()
    for b, (n, m) in enumerate(zip(lens, n_new)):
        kn[b, :, n + m:] = NAN
        vn[b, :, n + m:] = NAN
    return kn, vn


def check(q, kc, vc, lens, n_new, T, H, Hkv, splits=SPLITS):
    from pytorch_operator_1_amd.ops import llm

    B, D = kc.shape[0], kc.shape[3]
    kn, vn = poisoned(kc, vc, lens, n_new)
    lt = torch.tensor(lens, device="cuda", dtype=torch.int32)
    nt = torch.tensor(n_new, device="cuda", dtype=torch.int32)
    want = reference(q, kc, vc, lens, n_new, T, H)
    live = torch.tensor([t < min(n_new[b], kc.shape[2] - lens[b]) for b in range(B) for t in range(T)], device="cuda")
    for ns in splits:
        o = llm.attention_extend(q, kn, vn, lt, nt, T, H, Hkv, n_splits=ns)
        assert o.shape == (B * T, H * D) and o.dtype == torch.bfloat16
        assert torch.isfinite(o).all(), (lens, ns)
        err = (o.float() - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-30)
        assert err[live].max() < 1e-2, (lens, ns, err[live].max().item())
        assert torch.equal(o[~live], torch.zeros_like(o[~live])), (lens, ns)
        for b, n in enumerate(lens):
            if n == 0 and n_new[b] > 0:  # the first token sees one key: V[0] to bf16 rounding
                v0 = vn[b, :, 0].repeat_interleave(H // Hkv, 0).reshape(-1).float()
                torch.testing.assert_close(o[b * T].float(), v0, atol=0, rtol=2 ** -8)
        assert torch.equal(o, llm.attention_extend(q, kn, vn, lt, nt, T, H, Hkv, n_splits=ns)), (lens, ns)
    return kn, vn, lt, nt, want, live


@pytest.mark.parametrize("max_len", [64, 320, 4160])
@pytest.mark.parametrize("T", [1, 5, 8, 9, 33])
@pytest.mark.parametrize("B,H,Hkv,D", SHAPES)
def test_attention_extend_against_fp32(B, H, Hkv, D, T, max_len):
    from pytorch_operator_1_amd.ops import llm

    assert llm.attention_extend_supported(H, Hkv, D)
    torch.manual_seed(0)
    q = torch.randn(B * T, H * D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    cand = sorted({n for n in HIST if n + T <= max_len} | {max_len - T})
    cand += cand[:-len(cand) % B]  # fill the last group
    for i in range(0, len(cand), B):
        kn, vn, lt, nt, want, _ = check(q, kc, vc, cand[i:i + B], [T] * B, T, H, Hkv)
    # the default split count, through the fused QKV row layout
    qkv = torch.cat([q, torch.full((B * T, 2 * Hkv * D), NAN, device="cuda", dtype=torch.bfloat16)], 1)
    assert relerr(llm.attention_extend(qkv, kn, vn, lt, nt, T, H, Hkv), want) < 1e-2


@pytest.mark.parametrize("H,Hkv,D,T", [(8, 2, 128, 8), (4, 2, 64, 9), (8, 1, 128, 5)])
def test_attention_extend_ragged_chunk(H, Hkv, D, T):
    """n_new = [T, 2, 0] and a row that runs off the end of the cache: rows that are not live are exactly zero."""
    B, max_len = 4, 320
    torch.manual_seed(1)
    q = torch.randn(B * T, H * D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    q[T + 2:2 * T] = NAN  # a padded token's q row may hold anything
    *_, live = check(q, kc, vc, [60, 129, 5, max_len - 3], [T, 2, 0, T], T, H, Hkv)
    assert live.view(B, T).sum(1).tolist() == [T, 2, 0, 3]


@pytest.mark.parametrize("B,H,Hkv,D", [(2, 8, 2, 128), (2, 4, 2, 64)])
def test_attention_extend_running_max_moves_every_slab(B, H, Hkv, D):
    """The ramp of test_attention_decode_running_max_moves_every_tile at T = 8: the running max grows in every slab."""
    T, max_len = 8, 4160
    torch.manual_seed(2)
    qv = torch.randn(B, Hkv, 1, D, device="cuda")
    qv = qv / qv.norm(dim=-1, keepdim=True)
    ramp = torch.arange(max_len, device="cuda").float()[None, None, :, None] * 0.05 * D ** 0.5  # score = 0.05 * j
    kc = (qv * ramp + 0.1 * torch.randn(B, Hkv, max_len, D, device="cuda")).bfloat16()
    vc = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    q = qv.expand(B, Hkv, H // Hkv, D).reshape(B, 1, H * D).expand(B, T, H * D).reshape(B * T, H * D).bfloat16()
    for lens in ([max_len - T, 1000], [129, 3000]):
        check(q, kc, vc, lens, [T] * B, T, H, Hkv)


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 128), (4, 2, 64), (2, 1, 128)])
def test_rope_kv_extend_is_bitwise_rope(H, Hkv, D):
    from pytorch_operator_1_amd.ops import llm

    B, T, max_len = 4, 5, 40
    W = (H + 2 * Hkv) * D
    torch.manual_seed(3)
    cos, sin = llm.rope_tables(max_len, D, 500000.0, "cuda")
    lens, n_new = [0, 17, 37, 40], [5, 3, 5, 5]  # row 2 runs off the end mid-chunk, row 3 is full
    lt = torch.tensor(lens, device="cuda", dtype=torch.int32)
    nt = torch.tensor(n_new, device="cuda", dtype=torch.int32)
    q0 = torch.randn(B * T, W, device="cuda", dtype=torch.bfloat16)
    k0 = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    v0 = torch.randn(B, Hkv, max_len, D, device="cuda", dtype=torch.bfloat16)
    for table in (max_len, 20):  # a table shorter than the cache bounds the positions too
        qkv, kc, vc = q0.clone(), k0.clone(), v0.clone()
        assert llm.rope_kv_extend(qkv, cos[:table].contiguous(), sin[:table].contiguous(), kc, vc, lt, nt, T, H,
                                  Hkv) is qkv
        touched = torch.zeros(B, Hkv, max_len, dtype=torch.bool, device="cuda")
        for b in range(B):
            for t in range(T):
                r, p = b * T + t, lens[b] + t
                if t >= n_new[b] or p >= table:
                    assert torch.equal(qkv[r], q0[r]), (b, t)
                    continue
                buf = torch.zeros(max_len, W, device="cuda", dtype=torch.bfloat16)
                buf[p] = q0[r]
                want = llm.rope_(buf, cos, sin, max_len, H + Hkv, D)[p].view(H + 2 * Hkv, D)
                got = qkv[r].view(H + 2 * Hkv, D)
                assert torch.equal(got[:H], want[:H]), (b, t)  # the query heads, rotated in place
                assert torch.equal(kc[b, :, p], want[H:H + Hkv]), (b, t)  # K rotated
                assert torch.equal(vc[b, :, p], q0[r].view(-1, D)[H + Hkv:]), (b, t)  # V copied
                assert torch.equal(got[H:], q0[r].view(-1, D)[H:])  # the row's own K/V columns stay
                touched[b, :, p] = True
        assert touched.sum().item() == Hkv * (11 if table == max_len else 8)
        assert torch.equal(kc[~touched], k0[~touched]) and torch.equal(vc[~touched], v0[~touched])


def _models(name):
    from pytorch_operator_1_amd.models.llama import CONFIGS, Llama, LlamaConfig

    cfg = CONFIGS["llama3-mini"] if name == "hd128" else LlamaConfig(
        dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=1024, ffn_dim=512, max_seq_len=512)
    torch.manual_seed(0)
    model = Llama(cfg, impl="hip", device="cuda")
    truth = Llama(cfg, impl="torch", device="cuda", dtype=torch.float32)
    truth.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    return model, truth


@pytest.mark.parametrize("name", ["hd128", "hd64"])
def test_chunked_prefill_extend_generate_end_to_end(name):
    """Chunked prefill and a continuation on the filled cache are as close to an fp32 model as the bf16 full
    forward is (test_generate_end_to_end's factor 2); generate(prefill_chunk=) follows its own logits, replays
    from a graph bitwise and leaves the training state alone.  Measured values: profiles/extend.md."""
    from pytorch_operator_1_amd.models.llama import KVCache

    model, truth = _models(name)
    model.train()
    lens = [5, 128, 37]
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, model.cfg.vocab_size, (3, 128), generator=g).cuda()
    lt = torch.tensor(lens, device="cuda", dtype=torch.int32)
    out, logits = model.generate(prompts, lens, max_new_tokens=6, return_logits=True, prefill_chunk=16)
    assert torch.equal(out, logits.float().argmax(-1))
    assert torch.equal(model.generate(prompts, lens, max_new_tokens=6, graph=True, prefill_chunk=16), out)
    want = teacher_forced(truth, prompts, lens, out[:, :5])  # positions lens-1 .. lens+3
    full = teacher_forced(model, prompts, lens, out[:, :5])
    e_full0 = relerr(full[:, 0], want[:, 0])
    for c in (16, 48):
        cache = KVCache(model.cfg, 3, 160, "cuda")
        z = model.prefill(prompts, lt, cache, chunk=c)
        e = relerr(z, want[:, 0])
        print(f"extend {name}: chunk={c} e_chunked={e:.3e} e_full={e_full0:.3e}")
        assert cache.lens.tolist() == lens
        assert e <= 2 * e_full0, (c, e, e_full0)
    z = model.extend(out[:, :4], cache, logits="all")  # continuation: logits at lens .. lens+3
    e_ext, e_full = relerr(z, want[:, 1:]), relerr(full[:, 1:], want[:, 1:])
    print(f"extend {name}: continuation e_extend={e_ext:.3e} e_full={e_full:.3e}")
    assert z.shape == (3, 4, model.cfg.vocab_size) and cache.lens.tolist() == [n + 4 for n in lens]
    assert e_ext <= 2 * e_full, (e_ext, e_full)
    assert model.training and model.last_z_loss is None and all(p.grad is None for p in model.parameters())
