#!/usr/bin/env python3
"""Generate the fixtures of the ensemble sequence layers `elru-<E>` / `econv1d[_<K>]-<E>` by IMPORTING THE REFERENCE (build container only).

    python tests/golden/generate_ensemble_golden.py   # needs the reference tree; writes ensemble_layers.npz, train_elru_sac.npz,
                                                      # train_elru_td3.npz, train_econv1d_sac.npz and train_ensemble_meta.json

The stubs and helpers are those of generate_golden.py (imported, not edited); like that file this one holds data plumbing only, no
reference source text.  Everything runs on the CPU.

ensemble_layers.npz - per id (`elru-3`, `econv1d_3-3`) and input form (`m`: member-major [3, 2, 10, 8]; `s`: shared [2, 10, 8], read by every
member), prefix `<id>|<form>|`: `p|<key>` the state dict of `RNNBase(8, 8, [], ['linear'], [id])` (zero biases replaced by draws), `x`, `h0`
(a live carried-in state), `y`, `h` (the returned state), `w` (the recorded output gradient), `dx`, `g|<key>` (gradient of every parameter).
`start` / `mask` [2, 10, 1] are shared by all recordings: a start flag inside row 0, a masked token in row 1.

train_<name>.npz - the recipe of generate_golden.gen_models_and_train at D = 16 (width 32 puts one file above 1 MB): construction under seed
100, ring of lengths [T, 5, 7, T, 4, 9, 6] from `RandomState(ring_seed)`, seed 200 in front of three `train_one_batch()` calls;
value_embedding_layer_type = ['efc-4', <id>, 'efc-4'], value_layer_type = ['efc-4'] * 3, redq_m = 2, policy stacks ['fc', 'gilr', 'fc'].
Arrays: `policy0|`, `value0|`, `policy3|`, `value3|`, `target3|`, `log_alpha3`.  The Gaussian draws are those of torch's CPU generator
behind `manual_seed(200)`, which is how the tests of the other trainer fixtures reproduce them.  train_ensemble_meta.json holds per
recording the settings, `ring_seed`, `skip_len`, `logs` and, per critic module, the state-dict keys and shapes.

The ring's stream.  generate_mlp_golden.py describes how an element whose first gradient is rounding residue takes a whole AdamW step of
+-lr by the summation order of the reference's GEMM library, so that its recorded value is no property of the algorithm.  Its rule (walk
`RandomState(9), RandomState(10), ...` until no element's first gradient is below RESIDUE of the largest of its tensor) is applied here if,
and only if, an element otherwise misses the trainers' bar in the reference-against-reference sense: every recording is made twice, the
second time with every initial parameter scaled by 1 +- PERTURB (a rounding-sized change), and the two sets of networks are compared
at rtol 2e-3 / atol 2e-5, their logs at rel 2e-3 / abs 5e-4.  A stream is kept when nothing misses; the number of residue elements
of the kept stream is printed and stored in the meta file for the record (with these stacks - 24 576-element first layers - every
stream has some, which is why the test is the perturbed twin and not their count).
"""
import json
import os

import numpy as np
import torch

import generate_golden as G

LENS_TAIL = [5, 7, None, 4, 9, 6]
RESIDUE = 1e-5
PERTURB = 3e-7
D = 16
TRAIN = {'elru_sac': ('elru-4', 'sac'), 'elru_td3': ('elru-4', 'td3'), 'econv1d_sac': ('econv1d_3-4', 'sac')}


def gen_layers():
    from offpolicy_rnn.models.rnn_base import RNNBase
    out = {}
    E, B, L, C = 3, 2, 10, 8
    g = torch.Generator().manual_seed(17)
    start = torch.zeros(B, L, 1)
    start[:, 0] = 1
    start[0, 6] = 1
    mask = torch.ones(B, L, 1)
    mask[1, 4] = 0
    for lid in ('elru-3', 'econv1d_3-3'):
        for form, shape in (('m', (E, B, L, C)), ('s', (B, L, C))):
            torch.manual_seed(3)
            net = RNNBase(C, C, [], ['linear'], [lid])
            with torch.no_grad():
                for n_, p_ in net.named_parameters():
                    if 'bias' in n_ and p_.abs().sum() == 0:
                        p_.copy_(torch.randn(p_.shape, generator=g) * 0.1)
            hid = net.make_rnd_init_state(B, torch.device('cpu'))
            hid.set_rnn_start(start)
            hid.set_mask(mask)
            x = torch.randn(*shape, generator=g).requires_grad_(True)
            w = torch.randn(E, B, L, C, generator=g)
            pre = f'{lid}|{form}|'
            out[pre + 'h0'] = G.t2n(hid[0])
            y, h, _ = net.meta_forward(x, hid)
            assert tuple(y.shape) == (E, B, L, C)
            (y * w).sum().backward()
            out[pre + 'x'], out[pre + 'w'], out[pre + 'y'], out[pre + 'h'], out[pre + 'dx'] = G.t2n(x), G.t2n(w), G.t2n(y), G.t2n(h[0]), G.t2n(x.grad)
            for n_, p_ in net.named_parameters():
                out[pre + f'g|{n_}'] = G.t2n(p_.grad)
            for n_, p_ in net.state_dict().items():
                out[pre + f'p|{n_}'] = G.t2n(p_)
    out['start'], out['mask'] = G.t2n(start), G.t2n(mask)
    np.savez_compressed(os.path.join(G.OUT, 'ensemble_layers.npz'), **out)
    print('ensemble layers ok:', len(out), 'arrays')


def record(name, lid, algo, ring_seed, perturb=False):
    from offpolicy_rnn.algorithm.sac_full_length_rnn_redq_sep_optim import SACFullLengthRNNREDQ_SEP_OPTIM
    from offpolicy_rnn.algorithm.td3_full_length_rnn_redq_sep_optim import TD3FullLengthRNNREDQ_SEP_OPTIM
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import Transition
    obs, act, T = G.ENV['obs'], G.ENV['act'], G.ENV['T']
    lens = [T] + [T if n is None else n for n in LENS_TAIL]
    torch.manual_seed(100)
    np.random.seed(100)
    par = G.make_parameter('gilr', D=D, algo=algo, sac_batch_size=int(sum(lens) * 0.6), redq_m=2,
                           value_embedding_layer_type=['efc-4', lid, 'efc-4'], value_layer_type=['efc-4'] * 3)
    alg = (SACFullLengthRNNREDQ_SEP_OPTIM if algo == 'sac' else TD3FullLengthRNNREDQ_SEP_OPTIM)(par)
    if perturb:                           # the reference-against-reference twin: same run from parameters a rounding away
        gen = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for net in (alg.policy, alg.values[0]):
                for p in net.parameters(True):
                    p.mul_(1 + PERTURB * (torch.randint(0, 2, p.shape, generator=gen) * 2 - 1).to(p.dtype))
        for v, t in zip(alg.values, alg.target_values):
            t.copy_weight_from(v, 0.0)
    out = {}
    out.update(G.flat_sd(alg.policy.state_dict(), 'policy0|'))
    out.update(G.flat_sd(alg.values[0].state_dict(), 'value0|'))
    shapes = {mod: {k: list(v.shape) for k, v in d.items()} for mod, d in alg.values[0].state_dict().items()}
    rs = np.random.RandomState(ring_seed)
    for n in lens:
        o, a, r = G.synth_traj(rs, n, obs, act)
        G.push_traj(alg.replay_buffer, Transition, o, a, r, early_done=(n != T))
    residue = []

    def watch_first_step(optimizer, net_name, net):
        step = optimizer.step

        def first_step(*a, **k):
            for mod, module in net.contextual_modules.items():
                for key, p in module.named_parameters():
                    if p.grad is not None and p.grad.abs().max() > 0:
                        gr = p.grad.detach().abs().reshape(-1)
                        for i in torch.nonzero((gr > 0) & (gr < RESIDUE * gr.max())).reshape(-1).tolist():
                            residue.append([net_name, mod, key, i])
            optimizer.step = step
            return step(*a, **k)

        optimizer.step = first_step

    watch_first_step(alg.optimizer_value, 'value', alg.values[0])
    watch_first_step(alg.optimizer_policy, 'policy', alg.policy)
    torch.manual_seed(200)
    np.random.seed(200)
    logs = []
    for _ in range(3):
        log = alg.train_one_batch()
        alg.grad_num += 1
        logs.append({k: (float(v[0]) if isinstance(v, tuple) else float(v)) for k, v in log.items()})
    assert all(np.isfinite(v) for log in logs for v in log.values())
    out.update(G.flat_sd(alg.policy.state_dict(), 'policy3|'))
    out.update(G.flat_sd(alg.values[0].state_dict(), 'value3|'))
    out.update(G.flat_sd(alg.target_values[0].state_dict(), 'target3|'))
    out['log_alpha3'] = G.t2n(alg.log_sac_alpha)
    entry = dict(rnn=lid, algo=algo, lens=lens, D=D, ring_seed=ring_seed, sac_batch_size=par.sac_batch_size, redq_m=2, logs=logs,
                 skip_len=alg._get_skip_len(), nest=bool(alg.allow_nest_stack), value_shapes=shapes,
                 value_state_width=[int(w) for w in alg.values[0].embedding_network.rnn_hidden_state_input_size],
                 value_nparam=int(sum(p.numel() for p in alg.values[0].parameters())))
    alg.process_pool.shutdown()
    return out, entry, residue


def misses(out, entry, twin, twin_entry):
    """Elements / log entries of a recording that its perturbed twin does not reproduce at the trainers' bar."""
    bad = []
    for k, v in out.items():
        if k.startswith(('policy3|', 'value3|', 'target3|', 'log_alpha3')):
            far = np.abs(v - twin[k]) > 2e-5 + 2e-3 * np.abs(twin[k])
            bad += [(k, int(i)) for i in np.flatnonzero(far)]
    for it, (a, b) in enumerate(zip(entry['logs'], twin_entry['logs'])):
        bad += [(it, k) for k in a if abs(a[k] - b[k]) > max(5e-4, 2e-3 * abs(b[k]))]
    return bad


def gen_train():
    meta = {}
    for name, (lid, algo) in TRAIN.items():
        for ring_seed in range(9, 9 + 64):
            out, entry, found = record(name, lid, algo, ring_seed)
            twin, twin_entry, _ = record(name, lid, algo, ring_seed, perturb=True)
            bad = misses(out, entry, twin, twin_entry)
            print('train', name, 'ring stream', ring_seed, ':', len(found), 'first-step gradients that are rounding residue;',
                  len(bad), 'elements miss the bar against the perturbed twin', bad[:8])
            if not bad:
                break
        assert not bad, 'no ring stream whose recording its perturbed twin reproduces'
        entry['residue_elements'] = len(found)
        np.savez_compressed(os.path.join(G.OUT, f'train_{name}.npz'), **out)
        meta[name] = entry
        print('train', name, entry['logs'][-1]['critic_loss'], 'skip', entry['skip_len'])
    with open(os.path.join(G.OUT, 'train_ensemble_meta.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    assert os.path.isdir(G.REF), f'{G.REF} not found: fixtures can only be regenerated in the build container'
    G.install_stubs()
    torch.set_num_threads(4)
    gen_layers()
    gen_train()
