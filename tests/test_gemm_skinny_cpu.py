"""The Python side of the skinny decode GEMM (ops/gemm.py): shape rules, the
PTO_SKINNY plan, the CPU path of skinny_nt, and generation on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from pytorch_operator_1_amd.ops import gemm


@pytest.mark.parametrize("rows,n_out,k_in,swiglu,takes", [
    (1, 16, 32, False, True), (16, 128256, 4096, False, True), (3, 48, 96, False, True),
    (0, 16, 32, False, False), (17, 16, 32, False, False), (1, 24, 32, False, False), (1, 16, 48, False, False),
    (4, 32, 64, True, True), (4, 48, 64, True, False),  # F = 24
])
def test_skinny_takes_and_plan(rows, n_out, k_in, swiglu, takes, monkeypatch):
    assert gemm.skinny_takes(rows, n_out, k_in, swiglu) is takes
    if swiglu:
        return
    monkeypatch.delenv("PTO_SKINNY", raising=False)
    assert gemm.SKINNY_AUTO == frozenset() and gemm.skinny_plan(rows, n_out, k_in) == "lib"
    monkeypatch.setattr(gemm, "SKINNY_AUTO", frozenset({(n_out, k_in)}))
    for mode, want in (("auto", takes), ("1", takes), ("0", False)):
        monkeypatch.setenv("PTO_SKINNY", mode)
        assert gemm.skinny_plan(rows, n_out, k_in) == ("hip" if want else "lib"), mode
    monkeypatch.setenv("PTO_SKINNY", "yes")
    with pytest.raises(ValueError, match="PTO_SKINNY"):
        gemm.skinny_plan(rows, n_out, k_in)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_skinny_nt_cpu_path(dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 96, generator=g).to(dtype)
    w = (torch.randn(64, 96, generator=g) * 0.1).to(dtype)
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    want = F.linear(x.double(), w.double())
    y = gemm.skinny_nt(x, w)
    assert y.dtype == dtype and y.shape == (3, 64)
    torch.testing.assert_close(y.double(), want, rtol=tol, atol=tol)
    out = torch.zeros(3, 32, dtype=dtype)
    assert gemm.skinny_nt(x, w, out=out, swiglu=True) is out
    torch.testing.assert_close(out.double(), F.silu(want[:, :32]) * want[:, 32:], rtol=2 * tol, atol=tol)
    # linear_decode on CPU tensors is the plain linear whatever the switch says
    assert torch.equal(gemm.linear_decode(x, w), F.linear(x, w))


def test_cpu_generation_ignores_the_switch(monkeypatch):
    from pytorch_operator_1_amd.models.llama import Llama

    torch.manual_seed(0)
    model = Llama("llama3-tiny", impl="torch", device="cpu", dtype=torch.float32)
    prompts = torch.randint(0, 1024, (2, 9), generator=torch.Generator().manual_seed(1))
    monkeypatch.delenv("PTO_SKINNY", raising=False)
    want = model.generate(prompts, max_new_tokens=5)
    monkeypatch.setenv("PTO_SKINNY", "1")
    assert torch.equal(model.generate(prompts, max_new_tokens=5), want)
