"""The any-row MX GEMM's shape rules and CPU paths (ops/gemm.py mx_takes, mx_nt,
linear_mx) and the refusal to release the weights of a CPU model."""
import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("rows,n_out,k_in,swiglu,want", [
    (1, 32, 128, False, True), (17, 96, 4224, False, True), (1 << 20, 32, 128, False, True),
    (0, 32, 128, False, False), (17, 48, 128, False, False), (17, 32, 96, False, False),
    (17, 32, 192, False, False), (17, 64, 128, True, True), (17, 96, 128, True, False)])
def test_mx_takes(rows, n_out, k_in, swiglu, want):
    from pytorch_operator_1_amd.ops import gemm

    assert gemm.mx_takes(rows, n_out, k_in, swiglu) is want


@pytest.mark.parametrize("swiglu", [False, True])
@pytest.mark.parametrize("fmt", ["mxfp4", "mxfp8"])
def test_cpu_paths_equal_the_dequantised_product(fmt, swiglu):
    from pytorch_operator_1_amd.ops import gemm

    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 17, 128, generator=g).to(torch.bfloat16)
    q = gemm.quantize_mx(torch.randn(64, 128, generator=g).to(torch.bfloat16), fmt)
    want = F.linear(x, gemm.dequantize_mx(q))
    if swiglu:  # ops.llm.swiglu's arithmetic: the gate rounded to bf16 before the product
        gate, up = want.float().chunk(2, dim=-1)
        want = ((gate * torch.sigmoid(gate)).to(torch.bfloat16).float() * up).to(torch.bfloat16)
    assert torch.equal(gemm.linear_mx(x, q, swiglu=swiglu), want)
    assert torch.equal(gemm.mx_nt(x.view(34, 128), q, swiglu=swiglu), want.view(34, -1))


def test_release_needs_a_hip_model():
    from pytorch_operator_1_amd.models.llama import Llama, LlamaConfig

    cfg = LlamaConfig(dim=128, n_layers=1, n_heads=2, n_kv_heads=1, vocab_size=64, ffn_dim=128, max_seq_len=32)
    model = Llama(cfg, impl="torch", device="cpu")
    before = [m.weight.clone() for m in model.linear_modules()]
    with pytest.raises(ValueError, match="keep_bf16=False"):
        model.quantize_weights("mxfp4", keep_bf16=False)
    assert all(torch.equal(m.weight, b) for m, b in zip(model.linear_modules(), before))
    assert not any(hasattr(m, "weight_mx") for m in model.linear_modules())
