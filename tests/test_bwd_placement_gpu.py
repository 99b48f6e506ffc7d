"""k_bwd_all's XCD-affine block placement and the transposed fc1 update
tile (MI355X only).

The placement map is checked on the host through the kernel's own
``bwd_role_id``; the backward is compared BIT FOR BIT with a reference made
of separate launches of the stand-alone kernels on the same random inputs;
the transposed dW1 tile with the untransposed routine it replaced.

The bitwise reference, role by role (deterministic mode, ``wpart`` given):
  * conv2 wgrad: ``k_conv2_bwd``'s wgrad part launched once per 5-sample
    chunk on a zeroed buffer (one atomic add onto +0 per element is exact),
    the partial tiles then added in chunk order starting from 0 -- the sum
    the last arriver forms;
  * conv2 bias: ``k_conv2_bwd``'s bias part;
  * conv1 replicas (one per sample): ``k_conv2_bwd``'s dgrad part with its
    fused conv1 wgrad, launched per sample on a zeroed slot.  (The
    stand-alone ``k_conv1_bwd`` sums the same terms in another order, so it
    cannot be a bitwise reference of the fused form and is not used.)
  * fc1 / fc2: ``k_linear_bwd_weight`` + ``k_colsum``;
  * SGD: the flat multi-tensor launch ``k_ddp_sgd`` (the same ``sgd_elem``).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
WCHUNK, ICG = 5, 10  # samples per conv2-wgrad block, dgrad blocks per sample (mnist_kernels.hip)


def _L():
    from pytorch_operator_1_amd.ops import _lib

    return _lib, _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------ 1. the map ----
@pytest.mark.parametrize("dpair", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 8, 13, 64])
def test_block_map_is_a_bijection(B, dpair):
    """Every role's logical ids are exactly 0..T-1, each once, and the blocks
    of one XCD slot (blockIdx % 8) hold one contiguous run of the logical ids
    of each placed role (A, B, D), the runs following each other in slot
    order.  C and F keep their plain rank."""
    _, L = _L()
    cap = 4096
    role = (ctypes.c_int * cap)()
    lid = (ctypes.c_int * cap)()
    n = L.pto_bwd_block_map(B, dpair, role, lid, cap)
    want = {0: 13, 1: 17, 2: -(-B // WCHUNK) * 32, 3: B * ICG, 4: 200 if dpair else 400}
    assert n == sum(want.values())
    role, lid = list(role[:n]), list(lid[:n])
    assert all(0 <= r <= 4 for r in role)
    for r, T in want.items():
        ids = [lid[i] for i in range(n) if role[i] == r]
        assert sorted(ids) == list(range(T)), (r, T)
        if r < 2:  # C, F: the plain rank
            assert ids == list(range(T))
            continue
        nxt = 0
        for x in range(8):
            run = sorted(lid[i] for i in range(n) if role[i] == r and i % 8 == x)
            assert run == list(range(nxt, nxt + len(run))), (r, x)
            nxt += len(run)
            # slot sizes differ by at most one
            assert T // 8 <= len(run) <= -(-T // 8)
        assert nxt == T


# ------------------------------------------------- 2. bitwise backward ----
def _inputs(B, seed):
    """Random activations / codes of a step at batch B and a flat parameter
    buffer (params, momentum, grads + conv1 replica tail) like the
    trainer's."""
    from pytorch_operator_1_amd.models.mnist import param_offsets

    g = torch.Generator(device="cpu").manual_seed(seed)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).to(DEV)

    def codes(n):
        return torch.randint(0, 5, (n,), generator=g, dtype=torch.uint8).to(DEV)

    offs, total = param_offsets()
    t = dict(B=B, offs=offs, total=total)
    t["g2"], t["code2"] = rnd(B * 800, scale=0.1), codes(B * 800)
    t["a1p"], t["code1"] = rnd(B * 2880).clamp_min(0), codes(B * 2880)
    t["x"] = rnd(B * 784)
    t["dh1"] = rnd(B * 500, scale=0.1) * (torch.rand(B * 500, generator=g) < 0.6).to(DEV)
    t["a2p"], t["h1"] = rnd(B * 800).clamp_min(0), rnd(B * 500).clamp_min(0)
    t["dl"] = rnd(B * 10, scale=0.1)
    p = torch.zeros(total, device=DEV)
    m = torch.zeros(total, device=DEV)
    for name, (off, shape) in offs.items():
        n = math.prod(shape)
        p[off:off + n] = rnd(n, scale=0.05)
        m[off:off + n] = rnd(n, scale=0.01)
    t["p"], t["m"] = p, m
    t["c1"] = offs["conv1.weight"][0]
    t["stride"] = total - t["c1"]
    t["bias_off"] = offs["conv1.bias"][0] - t["c1"]
    t["lr"] = torch.tensor([0.03], device=DEV)
    return t


_OFF_ORDER = ("fc2.weight", "fc2.bias", "fc1.weight", "fc1.bias", "conv2.weight", "conv2.bias", "conv1.weight",
              "conv1.bias")
_OPT = (0.5, 1e-4, 1.0, 0)  # momentum, weight decay, grad scale, nesterov


def _run_bwd_all(t, grads_only, det=True):
    """pto_bwd_all on fresh copies; returns (p, m, arbuf, ctr, bidx, pending, hz)."""
    lib, L = _L()
    B, total = t["B"], t["total"]
    p, m = t["p"].clone(), t["m"].clone()
    nrep = B if det else 8
    ar = torch.zeros(total + max(1, nrep - 1) * t["stride"], device=DEV)
    ctr = torch.zeros(32, device=DEV, dtype=torch.int32)
    bidx = torch.zeros(1, device=DEV, dtype=torch.int64)
    pending = torch.zeros(1, device=DEV, dtype=torch.int32)
    hz = torch.ones(B * 500, device=DEV)
    wpart = torch.full((-(-B // WCHUNK) * 25000,), float("nan"), device=DEV) if det else None
    w2f = p[t["offs"]["conv2.weight"][0]:][:25000].clone()
    offs = [t["offs"][n][0] for n in _OFF_ORDER]
    rc = L.pto_bwd_all(t["g2"].data_ptr(), t["code2"].data_ptr(), t["a1p"].data_ptr(), w2f.data_ptr(),
                       t["x"].data_ptr(), t["code1"].data_ptr(), t["dh1"].data_ptr(), t["a2p"].data_ptr(),
                       t["h1"].data_ptr(), t["dl"].data_ptr(), p.data_ptr(), ar.data_ptr(), m.data_ptr(), *offs,
                       ctr.data_ptr(), None if grads_only else bidx.data_ptr(), 3,
                       None if grads_only else pending.data_ptr(), B, t["lr"].data_ptr(), *_OPT,
                       ar[total:].data_ptr(), nrep, t["stride"], int(grads_only), lib.ptr(wpart), hz.data_ptr(),
                       B * 500, lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return p, m, ar, ctr, bidx, pending, hz


_REF = {}


def _reference(B):
    """Gradients (flat buffer + one conv1 replica per sample) and the SGD
    result of the separate-launch reference; computed once per B."""
    if B in _REF:
        return _REF[B]
    lib, L = _L()
    t = _inputs(B, 100 + B)
    s = lib.stream_ptr()
    total, offs, c1 = t["total"], t["offs"], t["c1"]
    ar = torch.zeros(total + max(1, B - 1) * t["stride"], device=DEV)
    g = ar[:total]
    w2 = t["p"][offs["conv2.weight"][0]:][:25000].clone()

    def at(name):
        return g[offs[name][0]:].data_ptr()

    # conv2 wgrad: per chunk on a zeroed buffer, summed in chunk order from 0
    gw2 = torch.zeros(25000, device=DEV)
    for b0 in range(0, B, WCHUNK):
        nb = min(WCHUNK, B - b0)
        part = torch.zeros(25000, device=DEV)
        rc = L.pto_conv2_bwd(t["g2"][b0 * 800:].data_ptr(), t["code2"][b0 * 800:].data_ptr(),
                             t["a1p"][b0 * 2880:].data_ptr(), None, part.data_ptr(), None, None, nb, 1, None, None,
                             None, None, None, s)
        assert rc == 0
        gw2 = gw2 + part
    g[offs["conv2.weight"][0]:][:25000] = gw2
    # conv2 bias
    assert L.pto_conv2_bwd(t["g2"].data_ptr(), t["code2"].data_ptr(), None, None, None, at("conv2.bias"), None, B, 4,
                           None, None, None, None, None, s) == 0
    # conv1: one replica per sample (replica 0 = the flat conv1 range)
    for b in range(B):
        slot = g[c1:] if b == 0 else ar[total + (b - 1) * t["stride"]:]
        assert L.pto_conv2_bwd(t["g2"][b * 800:].data_ptr(), t["code2"][b * 800:].data_ptr(), None, w2.data_ptr(),
                               None, None, None, 1, 2, t["x"][b * 784:].data_ptr(), None,
                               t["code1"][b * 2880:].data_ptr(), slot.data_ptr(),
                               slot[t["bias_off"]:].data_ptr(), s) == 0
    # fc1, fc2
    assert L.pto_linear_bwd(t["dh1"].data_ptr(), t["a2p"].data_ptr(), None, None, at("fc1.weight"), at("fc1.bias"),
                            B, 500, 800, s) == 0
    assert L.pto_linear_bwd(t["dl"].data_ptr(), t["h1"].data_ptr(), None, None, at("fc2.weight"), at("fc2.bias"),
                            B, 10, 500, s) == 0
    torch.cuda.synchronize()
    # SGD on everything below conv1 (conv1's update stays owed after k_bwd_all)
    p, m, gs = t["p"].clone(), t["m"].clone(), g.clone()
    assert L.pto_mnist_ddp_sgd(p.data_ptr(), gs.data_ptr(), m.data_ptr(), total, c1, total, None, 1,
                               t["lr"].data_ptr(), *_OPT, None, 1, s) == 0
    torch.cuda.synchronize()
    _REF[B] = (t, ar, p, m)
    return _REF[B]


def _conv1_slots(t, ar):
    """The written elements (500 weights + 20 biases) of every conv1 replica."""
    B, total, st, bo = t["B"], t["total"], t["stride"], t["bias_off"]
    out = []
    for b in range(B):
        slot = ar[t["c1"]:] if b == 0 else ar[total + (b - 1) * st:]
        out.append(torch.cat([slot[:500], slot[bo:bo + 20]]))
    return torch.stack(out)


@pytest.mark.parametrize("grads_only", [0, 1])
@pytest.mark.parametrize("B", [1, 8, 13, 64])
def test_bwd_all_bitwise_vs_separate_launches(B, grads_only):
    """Deterministic k_bwd_all == the separate-launch reference, bit for bit:
    parameters, momentum and conv1 replicas (fused optimizer), or every
    gradient (grads-only).  B = 8 / 13: two / three wgrad chunks per tile
    (arrival counters + consume path); B = 1 / 13: role sizes that are no
    multiple of 8."""
    t, ar_ref, p_ref, m_ref = _reference(B)
    c1 = t["c1"]
    p, m, ar, ctr, bidx, pending, hz = _run_bwd_all(t, grads_only)
    assert _same(_conv1_slots(t, ar), _conv1_slots(t, ar_ref)), "conv1 replicas"
    assert int(ctr.abs().sum()) == 0, "arrival counters re-armed"
    assert float(hz.abs().max()) == 0.0, "split-fc1 buffer re-zeroed"
    if grads_only:
        for name, (off, shape) in t["offs"].items():
            if name.startswith("conv1"):
                continue
            n = math.prod(shape)
            assert _same(ar[off:off + n], ar_ref[off:off + n]), name
        assert _same(p, t["p"]) and _same(m, t["m"]), "grads-only touched a parameter"
        assert int(bidx) == 0 and int(pending) == 0
        return
    for name, (off, shape) in t["offs"].items():
        n = math.prod(shape)
        if name.startswith("conv1"):  # owed: applied by the next forward
            assert _same(p[off:off + n], t["p"][off:off + n]) and _same(m[off:off + n], t["m"][off:off + n]), name
            continue
        assert _same(p[off:off + n], p_ref[off:off + n]), name
        assert _same(m[off:off + n], m_ref[off:off + n]), name + " momentum"
    assert _same(p[:c1], p_ref[:c1]) and _same(m[:c1], m_ref[:c1])  # padding included
    assert int(bidx) == 1 and int(pending) == 1
    c2 = t["offs"]["conv2.weight"][0]
    assert float(ar[c2:c2 + 25000].abs().max()) == 0.0  # conv2.weight's gradient slot left zero


# --------------------------------------------------------- 3. fc1 tile ----
@pytest.mark.parametrize("opt", [(0.5, 0.0, 1.0, 0), (0.9, 1e-3, 0.5, 1)], ids=["momentum", "nesterov-wd"])
@pytest.mark.parametrize("B", [64, 5])
def test_fc1_tile_transposed_is_bitwise(B, opt):
    """The transposed dW1 update (dw1_tile_t) == the untransposed tile
    routine == the grads-only GEMM store followed by the flat SGD launch, on
    fc1.weight and its momentum; the two gradient stores agree too.  B = 5: a
    partial k round."""
    lib, L = _L()
    s = lib.stream_ptr()
    g = torch.Generator(device="cpu").manual_seed(7 + B)
    n = 500 * 800
    dh1 = (torch.randn(B * 500, generator=g) * 0.1 * (torch.rand(B * 500, generator=g) < 0.6)).to(DEV)
    a2p = torch.randn(B * 800, generator=g).clamp_min(0).to(DEV)
    p0 = (torch.randn(n + 64, generator=g) * 0.05).to(DEV)
    m0 = (torch.randn(n + 64, generator=g) * 0.01).to(DEV)
    lr = torch.tensor([0.03], device=DEV)

    def tiles(form, store):
        p, m, go = p0.clone(), m0.clone(), torch.full((n + 64,), float("nan"), device=DEV)
        rc = L.pto_dw1_tiles(dh1.data_ptr(), a2p.data_ptr(), p.data_ptr(), m.data_ptr(),
                             go.data_ptr() if store else None, B, lr.data_ptr(), *opt, form, s)
        assert rc == 0
        torch.cuda.synchronize()
        return p, m, go

    p_u, m_u, _ = tiles(0, False)
    p_t, m_t, _ = tiles(1, False)
    assert not _same(p_u[:n], p0[:n])
    assert _same(p_t[:n], p_u[:n]) and _same(m_t[:n], m_u[:n])
    assert _same(p_t[n:], p0[n:]) and _same(m_t[n:], m0[n:])  # nothing written past the matrix
    pg, mg, g_u = tiles(0, True)
    _, _, g_t = tiles(1, True)
    assert _same(pg, p0) and _same(mg, m0)
    assert _same(g_t[:n], g_u[:n]) and bool(torch.isnan(g_t[n:]).all())
    # the stored gradient through the flat SGD launch ([n, n + 64) stands in for its conv1 range)
    g_u[n:] = 0
    p_s, m_s = p0.clone(), m0.clone()
    assert L.pto_mnist_ddp_sgd(p_s.data_ptr(), g_u.data_ptr(), m_s.data_ptr(), n + 64, n, n + 64, None, 1,
                               lr.data_ptr(), *opt, None, 1, s) == 0
    torch.cuda.synchronize()
    assert _same(p_t[:n], p_s[:n]) and _same(m_t[:n], m_s[:n])
    p_p, m_p, _ = tiles(2, False)  # the tile-pair form of the same role
    assert _same(p_p[:n], p_t[:n]) and _same(m_p[:n], m_t[:n])


# ------------------------------------------------- 4. default (atomic) ----
def test_default_mode_one_step_matches_stock_pytorch():
    """One fused step at B = 64 in the default (atomic) mode against stock
    PyTorch autograd + torch.optim.SGD, with the fused step's tolerance of
    test_kernels_gpu.py."""
    from pytorch_operator_1_amd.train.fused_step import FusedMnistTrainer
    from pytorch_operator_1_amd.train.runner import EagerMnistTrainer

    dev = torch.device(DEV)
    fused = FusedMnistTrainer(dev, batch_size=64, dataset_size=640, seed=1, graph="none")
    eager = EagerMnistTrainer(dev, batch_size=64, dataset_size=640, seed=1)
    assert not fused.deterministic
    fused.step()
    eager.step()
    torch.cuda.synchronize()
    assert abs(fused.last_loss() - eager.last_loss()) < 1e-4
    for name, ref in eager.model.state_dict().items():
        got = fused.p[name]
        err = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()
        assert err < 1e-4, (name, err)
