"""ops/gemm.py / csrc/kernels/gemm_bf16.hip: the bf16 MFMA GEMM in its three
forms against a float64 product computed on the host -- exactly on integer
operands and to fp32-accumulation accuracy on real ones -- plus what it must
leave alone (rows and columns outside the result), strided operands,
repeatability, the refusal of unsupported shapes, the autograd ``linear``
built on it and the Llama model routed through it (``PTO_GEMM=1``)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# (M, N, K) as in ops/gemm.py: NT C[M,N] = A[M,K] B[N,K]^T, NN C[M,K] = A[M,N] B[N,K], TN C[N,K] = A[M,N]^T B[M,K]
NT_SHAPES = [
    (1, 64, 64),         # one row; a single k-tile: the pipeline's prologue meets its epilogue
    (77, 64, 128),       # ragged rows; both LDS buffers
    (256, 192, 192),     # a third k-tile reuses buffer 0; N no multiple of 128
    (257, 320, 64),      # one row spills into a new tile
    (640, 384, 256),     # 15 tiles: no multiple of 8 (a non-bijective XCD remap drops or doubles tiles)
    (128, 128, 4096),    # a long contraction
    (2048, 1024, 512),   # many tiles per XCD
    (3900, 4160, 128),   # the output at which NN and TN change to the 256 x 256 tile (NT keeps 128 x 128: 31 x 33 tiles)
]
NN_SHAPES = [(1, 64, 64), (77, 128, 192), (257, 192, 64), (640, 256, 384), (128, 4096, 128),
             (3900, 128, 4160)]   # 16 x 17 tiles of 256 x 256 (>= 256: the large tile), ragged rows, a quarter tile of columns
TN_SHAPES = [(64, 64, 64), (128, 192, 64), (192, 64, 320), (4096, 128, 128), (512, 1024, 640),
             (64, 72, 64),        # output rows a multiple of 8 only
             (128, 3912, 4160)]   # the large tile, output rows a multiple of 8 only
CASES = [("nt", s) for s in NT_SHAPES] + [("nn", s) for s in NN_SHAPES] + [("tn", s) for s in TN_SHAPES]
IDS = [f"{f}-{s[0]}-{s[1]}-{s[2]}" for f, s in CASES]
RAGGED = [(f, s) for f, s in CASES if f != "tn" and s[0] % 128]


def _fn(form):
    from pytorch_operator_1_amd.ops import gemm

    return {"nt": gemm.gemm_nt, "nn": gemm.gemm_nn, "tn": gemm.gemm_tn}[form]


def _operand_shapes(form, shape):
    M, N, K = shape
    return {"nt": ((M, K), (N, K)), "nn": ((M, N), (N, K)), "tn": ((M, N), (M, K))}[form]


def _out_shape(form, shape):
    M, N, K = shape
    return {"nt": (M, N), "nn": (M, K), "tn": (N, K)}[form]


@functools.lru_cache(maxsize=None)
def _case(form, shape, kind):
    """Host bf16 operands and their float64 product, computed once per
    (form, shape, kind) and shared (never modified)."""
    g = torch.Generator().manual_seed(1000 * CASES.index((form, shape)) + (kind == "int"))
    sa, sb = _operand_shapes(form, shape)
    if kind == "int":  # integers in [-2, 2]: exact in bf16, every partial sum exact in fp32
        a = torch.randint(-2, 3, sa, generator=g).to(torch.bfloat16)
        b = torch.randint(-2, 3, sb, generator=g).to(torch.bfloat16)
    else:
        a = torch.randn(sa, generator=g).to(torch.bfloat16)
        b = torch.randn(sb, generator=g).to(torch.bfloat16)
    ad, bd = a.double(), b.double()
    ref = {"nt": lambda: ad @ bd.t(), "nn": lambda: ad @ bd, "tn": lambda: ad.t() @ bd}[form]()
    return a, b, ref


def _dev(form, shape, kind):
    a, b, ref = _case(form, shape, kind)
    return a.to(DEV), b.to(DEV), ref


@pytest.mark.parametrize("form,shape", CASES, ids=IDS)
def test_exact_on_integers(form, shape):
    """|partial sums| <= 4 * 4096 < 2^24: any fp32 summation order is exact, so
    the fp32 output equals the float64 reference bit for bit and the bf16
    output is its round-to-nearest-even."""
    a, b, ref = _dev(form, shape, "int")
    got32 = _fn(form)(a, b, out_dtype=torch.float32)
    assert got32.dtype == torch.float32 and got32.shape == _out_shape(form, shape)
    g = got32.double().cpu()
    print(f"{form} {shape}: fp32 mismatches {int((g != ref).sum())} of {ref.numel()}")
    assert torch.equal(g, ref)
    got16 = _fn(form)(a, b)
    assert got16.dtype == torch.bfloat16
    want16 = ref.to(torch.bfloat16)
    print(f"{form} {shape}: bf16 mismatches {int((got16.cpu() != want16).sum())} of {ref.numel()}")
    assert torch.equal(got16.cpu(), want16)


@pytest.mark.parametrize("form,shape", CASES, ids=IDS)
def test_real_values(form, shape):
    """Standard-normal operands.  fp32 accumulation over a contraction of at
    most 4096 is within ~3.5e-7 * sum|a b| of the float64 sum, two orders of
    magnitude inside 2^-12 of the largest element; a bf16 partial sum is not.
    The bf16 output adds one rounding, at most 2^-9 relative: bound 2^-8."""
    a, b, ref = _dev(form, shape, "real")
    scale = ref.abs().max().item()
    e32 = (_fn(form)(a, b, out_dtype=torch.float32).double().cpu() - ref).abs().max().item() / scale
    e16 = (_fn(form)(a, b).double().cpu() - ref).abs().max().item() / scale
    print(f"{form} {shape}: max|got - ref| / max|ref| fp32 {e32:.3e} (bound {2 ** -12:.3e}), "
          f"bf16 {e16:.3e} (bound {2 ** -8:.3e})")
    assert e32 <= 2 ** -12
    assert e16 <= 2 ** -8


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form,shape", CASES, ids=IDS)
def test_nothing_outside_the_result_is_written(form, shape, dtype):
    """The output is the first rows and a column slice of a larger tensor
    filled with a sentinel: the result is right and the sentinel is intact
    (the edge tiles of a ragged M store under a mask)."""
    a, b, ref = _dev(form, shape, "int")
    R, C = _out_shape(form, shape)
    big = torch.full((R + 5, C + 16), -7.0, device=DEV, dtype=dtype)
    out = big[:R, 8:8 + C]
    assert _fn(form)(a, b, out=out) is out
    torch.cuda.synchronize()
    host = big.cpu()
    assert torch.equal(host[:R, 8:8 + C].double(), ref.to(dtype).double())
    mask = torch.ones_like(host, dtype=torch.bool)
    mask[:R, 8:8 + C] = False
    assert bool((host[mask] == -7.0).all()), f"{int((host[mask] != -7.0).sum())} sentinel elements overwritten"


def test_ragged_cases_are_covered():
    assert len(RAGGED) >= 8  # every NT / NN shape whose M is no multiple of the tile is in the parametrised cases


@pytest.mark.parametrize("form,shape", CASES, ids=IDS)
def test_strided_operands(form, shape):
    """A and B as column slices of wider matrices (row strides above the
    widths): bit for bit the contiguous result."""
    a, b, _ = _dev(form, shape, "real")
    wa = torch.full((a.shape[0], a.shape[1] + 24), float("nan"), device=DEV, dtype=torch.bfloat16)
    wb = torch.full((b.shape[0], b.shape[1] + 40), float("nan"), device=DEV, dtype=torch.bfloat16)
    wa[:, 8:8 + a.shape[1]] = a
    wb[:, 16:16 + b.shape[1]] = b
    av, bv = wa[:, 8:8 + a.shape[1]], wb[:, 16:16 + b.shape[1]]
    assert av.stride(0) > a.shape[1] and bv.stride(0) > b.shape[1]
    for dt in (torch.float32, torch.bfloat16):
        assert torch.equal(_fn(form)(av, bv, out_dtype=dt), _fn(form)(a, b, out_dtype=dt))


@pytest.mark.parametrize("form,shape", CASES, ids=IDS)
def test_repeatable(form, shape):
    a, b, _ = _dev(form, shape, "real")
    assert torch.equal(_fn(form)(a, b, out_dtype=torch.float32), _fn(form)(a, b, out_dtype=torch.float32))
    assert torch.equal(_fn(form)(a, b), _fn(form)(a, b))


def _raw(form, a_ptr, lda, b_ptr, ldb, out, M, N, K):
    from pytorch_operator_1_amd.ops import _lib

    return _lib.lib().pto_gemm_bf16(form, a_ptr, lda, b_ptr, ldb, out.data_ptr(), out.stride(0), 1, M, N, K,
                                    _lib.stream_ptr(DEV))


def test_refusal():
    """N = 96, K = 40, a row stride of 4 and a base pointer off by 2 bytes:
    the launcher returns -1 and writes nothing; gemm_nt raises."""
    from pytorch_operator_1_amd.ops import _lib, gemm

    buf = torch.zeros(128 * 128 + 8, device=DEV, dtype=torch.bfloat16)
    a = buf[:64 * 64].view(64, 64)
    out = torch.full((64, 128), -7.0, device=DEV, dtype=torch.float32)
    L = _lib.lib()
    assert L.pto_gemm_bf16_supported(0, 64, 64, 64, 64, 64, 128) == 1
    assert _raw(0, a.data_ptr(), 64, a.data_ptr(), 64, out, 64, 64, 64) == 0  # the accepted neighbour of the cases below
    torch.cuda.synchronize()
    assert bool((out[:, :64] == 0).all()) and bool((out[:, 64:] == -7.0).all())
    out.fill_(-7.0)
    p = a.data_ptr()
    bad = [
        ("N=96", (0, p, 64, p, 64, out, 64, 96, 64), (0, 64, 96, 64, 64, 64, 128)),
        ("K=40", (0, p, 40, p, 40, out, 64, 64, 40), (0, 64, 64, 40, 40, 40, 128)),
        ("lda=4", (0, p, 4, p, 64, out, 64, 64, 64), (0, 64, 64, 64, 4, 64, 128)),
        ("ldb=4", (0, p, 64, p, 4, out, 64, 64, 64), (0, 64, 64, 64, 64, 4, 128)),
        ("A+2B", (0, p + 2, 64, p, 64, out, 64, 64, 64), None),
        ("B+2B", (0, p, 64, p + 2, 64, out, 64, 64, 64), None),
        ("NN contraction 96", (1, p, 96, p, 64, out, 64, 96, 64), (1, 64, 96, 64, 96, 64, 128)),
        ("TN contraction 40", (2, p, 64, p, 64, out, 40, 64, 64), (2, 40, 64, 64, 64, 64, 128)),
        ("form 3", (3, p, 64, p, 64, out, 64, 64, 64), (3, 64, 64, 64, 64, 64, 128)),
    ]
    for name, args, sup in bad:
        assert _raw(*args) == -1, name
        if sup is not None:
            assert L.pto_gemm_bf16_supported(*sup) == 0, name
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(a, buf[:96 * 64].view(96, 64))
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(buf[:64 * 40].view(64, 40), buf[:64 * 40].view(64, 40))
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(torch.as_strided(buf, (64, 64), (4, 1)), a)
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(buf[1:1 + 64 * 64].view(64, 64), a)
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(a, a, out=torch.empty(64, 128, device=DEV, dtype=torch.bfloat16)[:, 1:65])  # out off by 2 bytes
    with pytest.raises(TypeError):
        gemm.gemm_nt(a.float(), a.float())


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("with_wt", [True, False], ids=["wt", "no-wt"])
def test_linear_autograd(monkeypatch, with_wt):
    """gemm.linear under PTO_GEMM=1 on x[77,192], w[128,192] against fp32
    autograd on the bf16-rounded operands.  77 rows are no multiple of 64, so
    the weight gradient's contraction is one the launcher refuses and the plan
    leaves that GEMM to the library; that dw is gemm_tn(dy, x) bit for bit is
    therefore checked at 128 rows, where all three GEMMs run on the kernel."""
    from pytorch_operator_1_amd.ops import gemm

    monkeypatch.setenv("PTO_GEMM", "1")
    g = torch.Generator().manual_seed(77)
    x = torch.randn(77, 192, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    w = torch.randn(128, 192, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    dy = torch.randn(77, 128, generator=g).to(torch.bfloat16).to(DEV)
    # 77 rows: the weight gradient's contraction is no multiple of 64, so the plan keeps it on the library
    assert [gemm.gemm_plan(k, 77, 128, 192) for k in gemm.KINDS] == ["hip", "hip", "lib"]
    wt = w.detach().t().contiguous() if with_wt else None
    y = gemm.linear(x, w, wt)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    xf, wf = x.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    yf = F.linear(xf, wf)
    rx, rw = torch.autograd.grad(yf, (xf, wf), dy.float())
    print(f"wt={with_wt}: relerr y {relerr(y, yf):.2e} dx {relerr(dx, rx):.2e} dw {relerr(dw, rw):.2e}")
    assert relerr(y, yf) < 1e-2 and relerr(dx, rx) < 1e-2 and relerr(dw, rw) < 1e-2
    assert torch.equal(y, gemm.gemm_nt(x.detach(), w.detach()))
    assert torch.equal(dx, gemm.gemm_nt(dy, wt) if with_wt else gemm.gemm_nn(dy, w.detach()))
    # 128 rows: all three GEMMs on the kernel
    x2 = torch.randn(128, 192, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    dy2 = torch.randn(128, 128, generator=g).to(torch.bfloat16).to(DEV)
    assert gemm.gemm_plan("wgrad", 128, 128, 192) == "hip"
    dx2, dw2 = torch.autograd.grad(gemm.linear(x2, w, wt), (x2, w), dy2)
    assert torch.equal(dw2, gemm.gemm_tn(dy2, x2.detach()))
    (rw2,) = torch.autograd.grad(F.linear(x2.detach().float(), wf), (wf,), dy2.float())
    assert relerr(dw2, rw2) < 1e-2


def test_linear_drops_a_stashed_transpose(monkeypatch):
    from pytorch_operator_1_amd.ops import gemm, llm

    monkeypatch.setenv("PTO_GEMM", "1")
    x = torch.randn(128, 64, device=DEV).bfloat16()
    w = torch.randn(64, 64, device=DEV).bfloat16().requires_grad_()
    st = llm.TStash()
    y = gemm.linear(x, w, None, True, st)
    st.t = torch.empty(64, 128, device=DEV, dtype=torch.bfloat16)
    dy = torch.randn(128, 64, device=DEV).bfloat16()
    (dw,) = torch.autograd.grad(y, (w,), dy)
    assert st.t is None
    assert torch.equal(dw, gemm.gemm_tn(dy, x))


def _model_run(seed=5):
    from pytorch_operator_1_amd.models.llama import Llama, synthetic_tokens

    torch.manual_seed(seed)
    m = Llama("llama3-tiny", impl="hip", device=DEV)
    tok, lab = synthetic_tokens(2, 128, m.cfg.vocab_size, DEV)
    loss = m(tok, lab)
    loss.backward()
    return m, loss.item()


def test_llama_on_the_kernel_matches_the_library(monkeypatch):
    """Llama-3-tiny, 2 x 128 tokens, same seed: PTO_GEMM=1 against PTO_GEMM=0
    within the bounds test_llama_hip_matches_torch_impl sets for two bf16
    implementations of the same math; under PTO_GEMM=1 every linear GEMM runs
    on the kernel and no module carries a W^T copy."""
    from pytorch_operator_1_amd.ops import gemm

    calls = {"nt": 0, "nn": 0, "tn": 0}
    for name in calls:
        real = getattr(gemm, "gemm_" + name)

        def spy(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(gemm, "gemm_" + name, spy)
    monkeypatch.setenv("PTO_GEMM", "0")
    b, lb = _model_run()
    assert calls == {"nt": 0, "nn": 0, "tn": 0}
    monkeypatch.setenv("PTO_GEMM", "1")
    monkeypatch.setenv("PTO_WT", "0")
    a, la = _model_run()
    n_lin = len(a.linear_modules())
    assert calls == {"nt": n_lin, "nn": n_lin, "tn": n_lin}, calls
    assert not any(hasattr(m, "weight_t") for m in a.modules())
    print(f"loss kernel {la:.5f} library {lb:.5f}")
    assert abs(la - lb) < 2e-2
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        e = relerr(pa.grad, pb.grad)
        print(f"{n}: relerr {e:.2e}")
        assert e < 5e-2, n


def test_llama_on_the_kernel_with_transposed_weights(monkeypatch):
    """With W^T copies attached the input gradients take the NT form from
    them, and w13 gets no stash."""
    from pytorch_operator_1_amd.models.llama import Llama, synthetic_tokens
    from pytorch_operator_1_amd.ops import gemm, llm

    monkeypatch.setenv("PTO_GEMM", "1")
    made = []
    real_init = llm.TStash.__init__

    def init(self):
        made.append(self)
        real_init(self)

    monkeypatch.setattr(llm.TStash, "__init__", init)
    torch.manual_seed(5)
    m = Llama("llama3-tiny", impl="hip", device=DEV)
    m.enable_transposed_dgrad()
    tok, lab = synthetic_tokens(2, 128, m.cfg.vocab_size, DEV)
    loss = m(tok, lab)
    loss.backward()
    assert not made
    ref, lref = _model_run()
    assert abs(loss.item() - lref) < 2e-2
    for (n, pa), pb in zip(m.named_parameters(), ref.parameters()):
        assert relerr(pa.grad, pb.grad) < 5e-2, n
    monkeypatch.setenv("PTO_GEMM", "0")
    m.zero_grad()
    m(tok, lab).backward()
    assert len(made) == len(m.layers)  # the library path still gets its stash
