"""The persistent GRU scans stand-alone, HIP events.  GPU box.

  python tools/prof_gru.py [B L H]          forward and backward time per step at B x L x H (default 64 x 1043 x 256)
  python tools/prof_gru.py --nets N         N (1 to 4) independent forward recurrences: ONE launch (ops.gru_seq_multi) next to N single
                                            launches issued back to back on one stream, us per step, at 64 x 1027 x 256 and 8 x 131 x 256
"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
import torch
from offpolicy_rnn.hip import ops


def multi(n_net, reps=7):
    for B, L, H in ((64, 1027, 256), (8, 131, 256)):
        g = torch.Generator(device='cuda').manual_seed(0)
        jobs = [(torch.randn(B, L, 3 * H, device='cuda', generator=g), torch.randn(3 * H, H, device='cuda', generator=g) / H ** 0.5,
                 torch.zeros(3 * H, device='cuda'), None, False) for _ in range(n_net)]

        def one_launch():
            ops.gru_seq_multi(jobs)

        def back_to_back():
            for gi, w, b, h0, _ in jobs:
                ops.gru_seq(gi, w, b, h0)

        res = {}
        with torch.no_grad():
            for name, fn in (('one launch', one_launch), ('single launches back to back', back_to_back)):
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                times = []
                for _ in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times.append(a.elapsed_time(b) * 1e3 / L)
                times.sort()
                res[name] = (times[len(times) // 2], times[0], times[-1])
        form = ops.gru_multi_form(n_net, B, H)
        print(f'N {n_net} B {B} L {L} H {H} ({"persistent" if form else "per-step"} multi form): ' +
              '  '.join(f'{k} {v[0]:.2f} us/step (min {v[1]:.2f}, max {v[2]:.2f}; layout launch and memset included)' for k, v in res.items()))


if '--nets' in sys.argv:
    multi(int(sys.argv[sys.argv.index('--nets') + 1]))
    sys.exit(0)

B, L, H = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (64, 1043, 256)
g = torch.Generator(device='cuda').manual_seed(0)
gi = torch.randn(B, L, 3 * H, device='cuda', generator=g).requires_grad_(True)
whh = (torch.randn(3 * H, H, device='cuda', generator=g) / H ** 0.5).requires_grad_(True)
bhh = torch.zeros(3 * H, device='cuda', requires_grad=True)
ref = torch.nn.GRU(H, H, batch_first=True).cuda()
for _ in range(2):
    out = ops.gru_seq(gi, whh, bhh)
    y = out[0] if isinstance(out, tuple) else out
    y.sum().backward()
torch.cuda.synchronize()
ops.profile_enable(True); ops.profile_collect()
for _ in range(5):
    out = ops.gru_seq(gi, whh, bhh)
    y = out[0] if isinstance(out, tuple) else out
    y.sum().backward()
torch.cuda.synchronize()
prof = ops.profile_collect(); ops.profile_enable(False)
print(f'B {B} L {L} H {H}: ' +
      '  '.join(f'{k} {v[1] / 1e3:.3f} ms = {v[1] / L:.2f} us/step' for k, v in prof.items() if k.startswith('gru')))
