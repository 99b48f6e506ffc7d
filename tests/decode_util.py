"""Shared inputs and references of the generation tests
(test_generate_cpu.py, test_decode_gpu.py): the sampler's planted logits and
its fp64 inverse-CDF reference, and the teacher-forced logits of a model."""
import torch

SAMPLE_ROWS = 4
SAMPLE_SETTINGS = [(1.0, 0), (0.7, 0), (0.7, 50), (1.3, 1)]
MIN_PROB = 2e-3  # tokens tested: probability >= this, so the CDF midpoint is >= 1e-3 from a boundary


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def sample_logits(V: int):
    """``randn * 4`` rounded to bf16, seed 0, with planted ties: row 1 has a
    new maximum at V//4 and again at 3*V//4 (the lower index must win), row 2
    repeats its maximum at index V-1 and row 3 at index 0; row 0 has a tie
    at the top-50 threshold.  Returns the bf16
    logits and the expected greedy tokens of the planted rows."""
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(SAMPLE_ROWS, V, generator=g) * 4).to(torch.bfloat16)
    top = (z[1].float().max() + 1).to(torch.bfloat16)
    z[1, V // 4] = top
    z[1, 3 * V // 4] = top
    first2 = int(z[2].float().argmax())
    z[2, V - 1] = z[2, first2]
    z[3, 0] = z[3].float().max().to(torch.bfloat16)
    if V > 50:  # row 0: the 50th and 51st largest are equal, so top-k 50 keeps at least 51
        order = z[0].float().sort(descending=True, stable=True).indices
        z[0, order[50]] = z[0, order[49]]
    return z, {1: V // 4, 2: first2, 3: 0}


def sample_cases(z_row, temperature: float, top_k: int):
    """fp64 reference of one row: ``(tokens, u, kept)`` -- every kept token
    with probability >= MIN_PROB and the midpoint of its CDF interval, which
    must draw exactly that token; ``kept`` is the size of the kept set."""
    zd = z_row.double()
    V = zd.numel()
    kept = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        kept = zd >= zd.sort(descending=True).values[top_k - 1]
    p = torch.where(kept, torch.exp((zd - zd.max()) / temperature), torch.zeros_like(zd))
    p = p / p.sum()
    cdf = p.cumsum(0)
    idx = torch.nonzero(kept & (p >= MIN_PROB))[:, 0]
    u = (cdf[idx] - p[idx] / 2).float()
    return idx, u, int(kept.sum())


def sample_batch(z, temperature: float, top_k: int):
    """All cases of all rows as one batch: logits ``[N, V]``, ``u [N]``,
    expected tokens ``[N]``, and the kept-set size of every source row."""
    rows, us, toks, kept = [], [], [], []
    for r in range(z.shape[0]):
        idx, u, n = sample_cases(z[r], temperature, top_k)
        assert idx.numel() >= (1 if top_k == 1 else 2), (r, idx.numel())
        rows.append(z[r:r + 1].expand(idx.numel(), -1))
        us.append(u)
        toks.append(idx)
        kept.append(n)
    return torch.cat(rows).contiguous(), torch.cat(us), torch.cat(toks), kept


def teacher_forced(model, prompts, lens, out):
    """Full-sequence logits of ``model`` at the positions that produced
    ``out``: row b runs ``prompt[:lens[b]] + out[b]`` and yields the logits at
    ``lens[b] - 1 .. lens[b] - 2 + n_new`` -> ``[B, n_new, V]``."""
    res = []
    n_new = out.shape[1]
    with torch.no_grad():
        for b, L in enumerate(lens):
            seq = torch.cat([prompts[b, :L], out[b]])[None]
            res.append(model(seq)[0, L - 1:L - 1 + n_new])
    return torch.stack(res)
