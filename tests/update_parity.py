"""The comparison that holds a whole update to the fp64 oracle trainer (shared by tests/test_update_parity_bound.py, which runs the
fp32 oracle through it on the CPU, and tests/test_update_published_width_gpu.py, which runs the product through it on the GPU).

Compared: the gradients of every parameter tensor of the actor and the critic, through the first-moment buffer of AdamW after the
first step (`exp_avg` = (1 - beta1) * g exactly), and the logged scalars.  Parameters are NOT compared: after the first AdamW step a
parameter is p0 - lr * g / (|g| + eps), which checks little more than the sign of each gradient element and is not robust for
elements with |g| near eps.

Bounds (fixed here, for both users):
  per parameter tensor t of a network   max |got - ref| <= MOMENT_BOUND * max(max |ref_t|, FLOOR * G),   G = the largest max |ref_t| of
                                        that network.  MOMENT_BOUND = 2e-4 is the bar tests/test_baseline_sizes_gpu.py holds the
                                        published tower's parameter gradients to; the fp32 oracle against the fp64 oracle measures at
                                        most 3e-6 at D = 256 (test_update_parity_bound.py asserts <= MOMENT_BOUND / 10).
  FLOOR = 1e-4                          a tensor that is zero by cancellation (or receives no gradient at all) cannot be held to its own
                                        size; at most MAX_UNDER_FLOOR = 8 tensors per network may sit below it (smamba at 64 x 128: 7 / 8).
  logged scalars, first update          pytest.approx(rel=2e-4, abs=1e-6)   (log_alpha is of size 1e-4, hence the absolute term)
  logged scalars, second update         pytest.approx(rel=2e-3, abs=5e-4)   (tests/test_trainer_gpu.py's bar for chained updates)
"""
import pytest
import torch

MOMENT_BOUND = 2e-4
FLOOR = 1e-4
MAX_UNDER_FLOOR = 8
LOG_TOL = ((2e-4, 1e-6), (2e-3, 5e-4))         # (rel, abs) of the first / second update's logged scalars


def oracle_moments(net, opt):
    """{'module.key': exp_avg} of an oracle network ({module: {key: tensor}}) from its torch AdamW.  A parameter that no loss reaches
    has no optimizer state: its gradient is zero.  Copies: the optimizer's next step rewrites its buffers in place."""
    out = {}
    for m, d in net.items():
        for k, p in d.items():
            st = opt.state.get(p, {})
            out[f'{m}.{k}'] = st['exp_avg'].detach().to(torch.float64, copy=True) if 'exp_avg' in st else torch.zeros_like(p, dtype=torch.float64)
    return out


def product_moments(store, opt):
    """{'module.key': m} of a FlatAdamW over a FlatParameterStore, cut with the store's slices (host fp64 copies)."""
    names = [f'{mn}.{k}' for mn, mod in store.modules.items() for k, _ in mod.named_parameters()]
    assert len(names) == len(store.slices)
    m = opt.m.detach().cpu().double()
    return {nm: m[o:o + n].view(p.shape) for nm, (p, o, n) in zip(names, store.slices)}


def _val(v):
    return v[0] if isinstance(v, tuple) else v


def compare_update(label, got_moments, ref_moments, got_logs, ref_logs):
    """got_moments / ref_moments: {network name: {tensor name: first moment}}; got_logs / ref_logs: the log dicts of the first (and,
    optionally, second) update.  Prints one MEASURED line per network and one for the scalars; returns a report whose `failures` is
    the list of everything out of bounds (empty = pass) - the callers assert on it after everything was printed."""
    rep = dict(failures=[], worst={}, under_floor={}, worst_scalar=None)
    for net, ref in ref_moments.items():
        got = got_moments[net]
        if set(got) != set(ref):
            rep['failures'].append(f'{net}: tensor names differ: {sorted(set(got) ^ set(ref))}')
            continue
        G = max(r.abs().max().item() for r in ref.values())
        worst, worst_name, under = 0.0, None, []
        for nm, r in ref.items():
            g = got[nm].double().reshape(r.shape)
            size = r.abs().max().item()
            if size < FLOOR * G:
                under.append((nm, size / G))
            err = (g - r).abs().max().item() / max(size, FLOOR * G)
            if not err <= worst:                          # a NaN becomes the worst
                worst, worst_name = err, nm
            if not err <= MOMENT_BOUND:
                rep['failures'].append(f'{net} {nm}: max|got - ref| / max(max|ref|, {FLOOR:g} G) = {err:.3e} > {MOMENT_BOUND:g} '
                                       f'(max|ref| = {size:.3e}, G = {G:.3e})')
        if len(under) > MAX_UNDER_FLOOR:
            rep['failures'].append(f'{net}: {len(under)} tensors below the floor (at most {MAX_UNDER_FLOOR})')
        rep['worst'][net], rep['under_floor'][net] = (worst, worst_name), under
        print(f'MEASURED {label} {net} first moments: worst tensor {worst_name} = {worst:.3e} of max(max|ref_t|, {FLOOR:g} G) '
              f'(bound {MOMENT_BOUND:g}), G = {G:.3e}, {len(ref)} tensors, {len(under)} below the floor: '
              + ', '.join(f'{nm} ({s:.1e} G)' for nm, s in under))
    for it, (gl, rl) in enumerate(zip(got_logs, ref_logs)):
        rel, ab = LOG_TOL[it]
        worst, worst_key = 0.0, None
        for k, want in rl.items():
            if k not in gl:
                rep['failures'].append(f'update {it} log: {k} missing')
                continue
            g, w = float(_val(gl[k])), float(_val(want))
            frac = abs(g - w) / max(rel * abs(w), ab)
            if not frac <= worst:
                worst, worst_key = frac, k
            if not g == pytest.approx(w, rel=rel, abs=ab):
                rep['failures'].append(f'update {it} log {k}: got {g!r}, want {w!r} (rel {rel:g}, abs {ab:g})')
        if it == 0:
            rep['worst_scalar'] = (worst, worst_key)
        print(f'MEASURED {label} logged scalars of update {it}: worst {worst_key} at {worst:.3f} of its tolerance (rel {rel:g}, abs {ab:g})')
    return rep
