"""Case table of the head widths beyond 32 and 64 (shared by tests/test_attention_head_dims_host.py and
tests/test_attention_head_dims_gpu.py): hd = 128 runs natively, every other multiple of 8 zero-padded to the next kernel width.
The recipe is `attention_parity.make_case`'s (that one reads its own CASES): from torch.Generator().manual_seed(seed),
qkv = randn(T, 3, H, hd) with q, k scaled by 0.8 and v by 0.8, dout = randn, both rounded to bf16; ALiBi slopes, scale hd ** -0.5 of the
TRUE width; the dropout counter is attention_parity's (SEED, OFFSET).  The model, the metric and the bounds are attention_parity's,
unchanged.  641 tokens = five key blocks and one token: both LDS buffers are reused, the late query blocks cross the diagonal, the last
block has one token."""
import numpy as np
import torch

from oracle import kernels as K

CASES = {
    'ragged128': dict(seed=2000, H=2, hd=128, lens=[641, 1, 127, 129], p_drop=0.0),
    'drop128': dict(seed=2001, H=2, hd=128, lens=[385, 33], p_drop=0.1),
    'ragged16': dict(seed=2002, H=8, hd=16, lens=[641, 1, 127, 129], p_drop=0.0),
    'ragged96': dict(seed=2003, H=2, hd=96, lens=[385, 33], p_drop=0.0),
    'ragged8': dict(seed=2004, H=4, hd=8, lens=[385, 33], p_drop=0.0),
}


def make_case(name):
    c = CASES[name]
    H, hd, lens = c['H'], c['hd'], c['lens']
    g = torch.Generator().manual_seed(c['seed'])
    T = sum(lens)
    qkv = torch.randn(T, 3, H, hd, generator=g)
    qkv[:, :2] *= 0.8
    qkv[:, 2] *= 0.8
    dout = torch.randn(T, H, hd, generator=g)
    cu = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32)
    pos = torch.cat([torch.arange(n) for n in lens])
    return dict(name=name, H=H, hd=hd, lens=lens, qkv=qkv.to(torch.bfloat16), dout=dout.to(torch.bfloat16), cu=cu,
                slopes=K.alibi_slopes(H), scale=hd ** -0.5, p_drop=c['p_drop'], pos=pos)


def mutant_tile(case):
    """The harness's mutant for these cases: the first 32-key tile is lost for the last 64 queries of the longest sequence."""
    return (32, max(case['lens']) - 64)
