"""Inputs and reference formulas shared by tests/test_lm_eval_cpu.py and
tests/test_lm_eval_gpu.py (not a test module).

``planted_case(V)``: 96 rows of ``(3*randn).bfloat16()`` logits with random
labels, and eight planted rows, because a random label is almost never the
argmax (a kernel that returned zero counts would pass) and almost always
ties with other bf16 logits at a large V:

====  ====================================================  ==================
row   content                                               expected
====  ====================================================  ==================
0     label = the first argmax                              rank 0
1     row maximum + 1 at columns 1 and V-2, label V-2       rank 1 (tie: the
                                                            lower index wins)
2     row 1 again, label 1                                  rank 0
3     40, 39, ..., 35 at six columns, label on the 36       rank 4: top-5 hit
4     row 3 again, label on the 35                          rank 5: a miss
5     label = ignore_index                                  skipped
6     label V-1
7     label 0
====  ====================================================  ==================
"""
import torch

M = 96
K = 5
PLANTED_RANKS = {0: 0, 1: 1, 2: 0, 3: 4, 4: 5}


def ignore_index(V):
    return -1 if V == 1000 else -100  # one vocabulary runs a non-default ignore_index


_cases = {}


def planted_case(V):
    """(bf16 logits [M, V], int64 labels [M]) on the CPU, made once and never written."""
    if V not in _cases:
        g = torch.Generator(device="cpu").manual_seed(7 + V)
        z = (3 * torch.randn(M, V, generator=g)).bfloat16()
        y = torch.randint(0, V, (M,), generator=g)
        zf = z.float()
        y[0] = int((zf[0] == zf[0].max()).nonzero()[0])
        top = (zf[1].max() + 1).bfloat16()
        assert float(top) > float(zf[1].max())
        z[1, 1] = top
        z[1, V - 2] = top
        y[1] = V - 2
        z[2] = z[1]
        y[2] = 1
        pos = [V - 1, 0, V // 2, 3, V - 3, 1]
        assert len(set(pos)) == 6
        for p, v in zip(pos, (40.0, 39.0, 38.0, 37.0, 36.0, 35.0)):
            z[3, p] = v
        y[3] = pos[4]
        z[4] = z[3]
        y[4] = pos[5]
        y[5] = ignore_index(V)
        y[6] = V - 1
        y[7] = 0
        _cases[V] = (z, y)
    return _cases[V]


def ref_rows(z, y, ii):
    """(row_loss fp32, row_rank int64, valid) from the formulas of the
    issue, on the values of ``z`` as stored; ignored rows: loss 0, rank -1."""
    valid = y != ii
    yc = torch.where(valid, y, torch.zeros_like(y))
    zy = z.gather(1, yc[:, None])
    idx = torch.arange(z.shape[1], device=z.device)[None, :]
    rank = (z > zy).sum(1) + ((z == zy) & (idx < yc[:, None])).sum(1)
    loss = torch.logsumexp(z.float(), dim=-1) - zy[:, 0].float()
    return torch.where(valid, loss, torch.zeros_like(loss)), torch.where(valid, rank, torch.full_like(rank, -1)), valid


def close(a, b):
    """The bound of this kernel family (tests/test_ce_options_gpu.py)."""
    return abs(a - b) < 1e-3 * max(1.0, b)


def rows_close(a, b):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() < 1e-3 * b.clamp_min(1.0)).all())
