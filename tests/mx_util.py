"""Shared inputs of the MX tests (test_gemm_mx_cpu.py, test_gemm_mx_gpu.py)."""
import torch

FP4 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
SPECIAL_K = 288  # 9 blocks


def special_blocks(fmt: str):
    """fp32 ``[6, 288]`` of bf16-exact values and the expected scale byte of
    each row's first block.  Rows 0 / 1: every representable element value
    times 2^3 / 2^-5, each block led by the largest; row 2: ties; row 3:
    values above the largest element; row 4: zeros; row 5: amax a power of
    two.  Rows 2..5 use their first block only."""
    if fmt == "mxfp4":
        vals = torch.tensor(FP4 + tuple(-v for v in FP4))
        top, ties, sat, e5 = 6.0, [4.0, 2.5, 3.5, 0.25, 0.75, -2.5, 5.0, 1.25], [7.5, -7.0], 118
    else:
        codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
        vals = codes.view(torch.float8_e4m3fn).float()
        top, ties, sat, e5 = 448.0, [448.0, 272.0, 304.0, -272.0], [500.0, -480.0], 112
    body = torch.zeros(9 * 31)
    body[:vals.numel()] = vals
    every = torch.cat([torch.full((9, 1), top), body.view(9, 31)], dim=1).reshape(-1)
    w = torch.zeros(6, SPECIAL_K)
    w[0], w[1] = every * 8, every / 32
    w[2, :len(ties)] = torch.tensor(ties)
    w[3, :2] = torch.tensor(sat)
    w[5, :2] = torch.tensor([2.0 ** -7, 2.0 ** -9])
    return w, [130, 122, 127, 127, 127, e5]
