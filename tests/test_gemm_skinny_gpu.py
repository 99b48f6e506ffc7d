"""The skinny bf16 MFMA GEMM of the decode linears (csrc/kernels/gemm_skinny.hip)
against fp64 on the CPU, its bit rules, and generation on it end to end."""
import pytest
import torch

from decode_util import relerr, teacher_forced

pytestmark = pytest.mark.gpu

SENT = 777.0
SHAPES = [(16, 32), (48, 96), (32, 4160)]  # one tile, one step / steps no wave or split count divides / long K
DTYPES = (torch.bfloat16, torch.float32)


def strided(t, pad=8):
    """``t`` on the device as a view of a wider buffer: row stride = columns + pad."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def run(x, w, ns, dtype, swiglu=False):
    """skinny_nt into a sentinel-filled strided ``out`` with two spare rows;
    returns the result and checks that nothing else was written."""
    from pytorch_operator_1_amd.ops import gemm

    M, cols = x.shape[0], w.shape[0] // (2 if swiglu else 1)
    buf = torch.full((M + 2, cols + 8), SENT, dtype=dtype, device="cuda")
    gemm.skinny_nt(x, w, out=buf[:M, :cols], swiglu=swiglu, n_splits=ns)
    assert (buf[M:] == SENT).all() and (buf[:, cols:] == SENT).all()
    return buf[:M, :cols].clone()


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 3, 16])
def test_skinny_against_fp64(M, N, K, ns):
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    # integers in [-3, 3]: every sum is below 2^24, so fp32 is exact
    xi = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    wi = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16)
    exact = (xi.double() @ wi.double().t()).float()
    xr = torch.randn(M, K, generator=g).to(torch.bfloat16)
    wr = torch.randn(N, K, generator=g).to(torch.bfloat16)
    truth = xr.double() @ wr.double().t()
    bound = K * 2.0 ** -24 * (xr.double().abs() @ wr.double().abs().t())  # any-order fp32 summation
    xi_d, wi_d, xr_d, wr_d = strided(xi), strided(wi), strided(xr), strided(wr)
    for dtype in DTYPES:
        y = run(xi_d, wi_d, ns, dtype)
        assert torch.equal(y.cpu(), exact.to(dtype)), dtype
        y = run(xr_d, wr_d, ns, dtype)
        tol = bound + (2.0 ** -8 * truth.abs() if dtype == torch.bfloat16 else 0)
        err = (y.cpu().double() - truth).abs()
        print(f"M={M} N={N} K={K} ns={ns} {dtype}: max err/bound {(err / tol).max().item():.3f}")
        assert (err <= tol).all()
        assert torch.equal(run(xr_d, wr_d, ns, dtype), y)  # a repeated call
        for m in range(M):  # row m does not depend on M or on the other rows
            assert torch.equal(run(xr_d[m:m + 1], wr_d, ns, dtype)[0], y[m]), m


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("F,K", [(16, 32), (48, 96), (16, 4160)])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_fused_swiglu_equals_unfused(M, F, K, ns):
    from pytorch_operator_1_amd.ops import llm

    g = torch.Generator().manual_seed(F + K + M)
    x = strided(torch.randn(M, K, generator=g).to(torch.bfloat16))
    w = strided((torch.randn(2 * F, K, generator=g) * K ** -0.5).to(torch.bfloat16))
    fused = run(x, w, ns, torch.bfloat16, swiglu=True)
    assert fused.shape == (M, F) and fused.abs().max() > 0
    assert torch.equal(fused, llm.swiglu(run(x, w, ns, torch.bfloat16)))


def test_refusals_leave_out_untouched():
    from pytorch_operator_1_amd.ops import gemm

    def refused(M, N, K, misalign=False):
        xb = torch.ones(M, K + 8, dtype=torch.bfloat16, device="cuda")
        x = xb[:, 4:4 + K] if misalign else xb[:, :K]
        w = torch.ones(N, K, dtype=torch.bfloat16, device="cuda")
        out = torch.full((M, N), SENT, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError, match="unsupported shape or layout"):
            gemm.skinny_nt(x, w, out=out)
        assert (out == SENT).all()
        return True

    assert refused(17, 16, 32) and refused(1, 24, 32) and refused(1, 16, 48) and refused(2, 16, 32, misalign=True)
    with pytest.raises(RuntimeError, match="unsupported"):  # F = 24
        gemm.skinny_nt(torch.ones(1, 32, dtype=torch.bfloat16, device="cuda"),
                       torch.ones(48, 32, dtype=torch.bfloat16, device="cuda"), swiglu=True)


@pytest.mark.parametrize("name", ["hd128", "hd64"])
def test_generate_on_the_skinny_kernel(name, monkeypatch):
    """test_generate_end_to_end's accuracy and graph checks with every decode
    linear (and the head) on the skinny kernel."""
    from pytorch_operator_1_amd.models.llama import CONFIGS, Llama, LlamaConfig
    from pytorch_operator_1_amd.ops import gemm

    cfg = CONFIGS["llama3-mini"] if name == "hd128" else LlamaConfig(
        dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=1024, ffn_dim=512, max_seq_len=512)
    torch.manual_seed(0)
    model = Llama(cfg, impl="hip", device="cuda")
    truth = Llama(cfg, impl="torch", device="cuda", dtype=torch.float32)
    truth.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    calls = []
    real = gemm.skinny_nt
    monkeypatch.setattr(gemm, "skinny_nt", lambda *a, **kw: calls.append(kw.get("swiglu")) or real(*a, **kw))
    monkeypatch.setenv("PTO_SKINNY", "1")
    lens, n_new = [5, 128, 37], 12
    prompts = torch.randint(0, cfg.vocab_size, (3, 128), generator=torch.Generator().manual_seed(1)).cuda()
    out, logits = model.generate(prompts, lens, max_new_tokens=n_new, return_logits=True)
    # per step 4 linears per layer, one of them fused, and the head; the prefill's head too
    assert len(calls) == (n_new - 1) * (4 * cfg.n_layers + 1) + 1 and calls.count(True) == (n_new - 1) * cfg.n_layers
    assert torch.equal(out, logits.float().argmax(-1))
    want = teacher_forced(truth, prompts, lens, out)
    e_full = relerr(teacher_forced(model, prompts, lens, out), want)
    e_dec = relerr(logits, want)
    print(f"generate {name} PTO_SKINNY=1: e_full={e_full:.3e} e_dec={e_dec:.3e}")
    assert e_dec <= 2 * e_full, (e_dec, e_full)
    assert torch.equal(model.generate(prompts, lens, max_new_tokens=n_new, graph=True), out)
    assert torch.equal(model.generate(prompts, lens, max_new_tokens=n_new, temperature=0.7, top_k=50, seed=11,
                                      graph=True),
                       model.generate(prompts, lens, max_new_tokens=n_new, temperature=0.7, top_k=50, seed=11))
