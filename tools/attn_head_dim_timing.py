"""Times the cgpt attention kernels per head width at the shape of the csrc/attention.hip header: 32 sequences of 1026 tokens plus 32
of one token at embedding width 256, in the layouts H x hd = 8 x 32, 4 x 64, 2 x 128 and 16 x 16 (the last runs zero-padded on the
32-wide kernels, so its pad / unpad passes are timed on their own).

    python tools/attn_head_dim_timing.py [--runs 20] [--warmup 5] [--layouts 8x32,4x64]

Forward, dQ and dK/dV are per-dispatch kernel times (the library's profiling events, `ops.profile_enable`), one sample per run; the
pad / unpad passes are stream-event intervals around one call each (they include the launch gap).  Printed: the median over the runs
with the minimum and maximum, TFLOP/s of the causal-half flops of the TRUE width (2, 3 and 4 products of n^2 / 2 * hd multiply-adds per
sequence and head for forward, dQ and dK/dV) and their fraction of the dense bf16 MFMA peak (2500 TFLOP/s).  One process, one device.
--layouts restricts the rows (a parent commit without the 128-wide kernels runs 8x32,4x64)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
import torch                                                   # noqa: E402
from offpolicy_rnn.hip import ops                              # noqa: E402

PEAK_TFLOPS = 2500.0
ROWS, LONG = 32, 1026
KERNELS = (('fwd', 1.0), ('dq', 1.5), ('dkv', 2.0))


def med(xs):
    return f'{statistics.median(xs):7.1f} us [{min(xs):6.1f} .. {max(xs):6.1f}]'


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--layouts', default='8x32,4x64,2x128,16x16')
    args = ap.parse_args()
    assert args.runs >= 10, 'the median of at least 10 runs'
    lens = [1, LONG] * ROWS
    T = sum(lens)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)
    for layout in args.layouts.split(','):
        H, hd = (int(v) for v in layout.split('x'))
        hdp = ops.attn_head_pad(hd) if hasattr(ops, 'attn_head_pad') else hd
        qkv = (torch.randn(T, 3, H, hd, device='cuda', generator=gen) * 0.5).to(torch.bfloat16).requires_grad_(True)
        dout = torch.randn(T, H, hd, device='cuda', generator=gen).to(torch.bfloat16)
        slopes = torch.tensor([2.0 ** (-8.0 * (i + 1) / H) for i in range(H)], device='cuda')
        flops = 2.0 * sum(n * n for n in lens) * H * hd       # one pair of products over the causal half
        samples = {k: [] for k, _ in KERNELS}
        ops.profile_enable(True)
        ops.profile_collect()
        for run in range(args.warmup + args.runs):
            out = ops.attn_varlen(qkv, cu, max(lens), slopes)
            out.backward(dout)
            torch.cuda.synchronize()
            prof = ops.profile_collect()
            if run >= args.warmup:
                for k, _ in KERNELS:
                    n, us = prof[f'attn_{k}_kernel']
                    assert n == 1
                    samples[k].append(us)
        ops.profile_enable(False)
        print(f'H x hd = {H} x {hd}' + (f' (kernels at {hdp})' if hdp != hd else '') + f', T = {T}, median of {args.runs} runs [min .. max]:')
        for k, mult in KERNELS:
            tf = flops * mult / statistics.median(samples[k]) * 1e-6
            print(f'  {k:4s} {med(samples[k])}   {tf:6.1f} TFLOP/s = {100 * tf / PEAK_TFLOPS:4.1f} % of the bf16 MFMA peak')
        if hdp != hd:
            passes = {'pad qkv': [], 'pad dout': [], 'unpad out': [], 'unpad dqkv': []}
            x, d4 = qkv.detach(), dout.view(T, 1, H, hd)
            for run in range(args.warmup + args.runs):
                t1, wide = event_us(lambda: ops._head_pad(x, hdp))
                t2, dwide = event_us(lambda: ops._head_pad(d4, hdp))
                t3, _ = event_us(lambda: ops._head_unpad(dwide, hd))
                t4, _ = event_us(lambda: ops._head_unpad(wide, hd))
                if run >= args.warmup:
                    for key, t in zip(passes, (t1, t2, t3, t4)):
                        passes[key].append(t)
            for key, xs in passes.items():
                print(f'  {key:10s} {med(xs)}')


if __name__ == '__main__':
    main()
