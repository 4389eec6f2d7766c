"""Inputs of the wide fused ArcFace head tests (D up to 512, any batch size), shared by
test_arcface_fused_wide_cpu.py (which shows on the CPU that the gradient bound separates a correct
kernel from one that drops a staged tile) and test_arcface_fused_wide_gpu.py (which runs the kernels
on the same inputs)."""
import torch

S, M = 30.0, 0.5
GO = 0.37

# (B, C, D): see the GPU test's docstring for what each one exercises
WIDE_SHAPES = [
    (70, 130, 512),
    (64, 700, 300),
    (130, 1100, 512),
    (2112, 130, 256),
    (2112, 130, 512),
    (6208, 70, 100),
]


def seed_of(B, C, D):
    return 9000 + B + C + D


def bwd_tile(Dp):
    """Classes (dX) / rows (dW) per staged tile of the backward kernels: 32 at Dp = 512, else 64."""
    return 32 if Dp == 512 else 64


def inputs(B, C, D, dtype, seed):
    """Features x [B, D] in ``dtype``, fp32 class weights W [C, D], labels [B]: rows 0..2 have cos ~ 1
    with their class (the margin's sin -> 0 guard), labels 0 and C - 1 occur, rows 5 and 6 carry the
    invalid labels -1 and C + 3."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=gen)
    W = torch.randn(C, D, generator=gen) * 0.05
    lab = torch.randint(0, C, (B,), generator=gen)
    lab[0], lab[1] = 0, C - 1
    x[:3] = W[lab[:3]]
    lab[5], lab[6] = -1, C + 3
    return x.to(dtype), W, lab
