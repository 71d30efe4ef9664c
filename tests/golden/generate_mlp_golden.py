#!/usr/bin/env python3
"""Generate the fixtures of the memoryless REDQ trainer by IMPORTING THE REFERENCE (build container only).

    python tests/golden/generate_mlp_golden.py        # needs the reference tree, writes train_mlp_redq.npz and train_mlp_meta.json

The stubs and helpers are those of generate_golden.py (imported, not edited); like that file this one holds data plumbing only, no
reference source text.  The reference's `SAC_MLP_REDQ_EnsembleQ` runs on the CPU: obs 5 / act 3 / T 12, D = 32, `efc-4` critic embedding
and head stacks, `fc` policy stacks, no separate 128-wide input encoders (`state_action_encoder = False`: with them one critic snapshot alone is
180 KB), `redq_m = 2`, `sac_batch_size = 16`, trajectories of lengths [12, 5, 7, 12, 4, 9, 6] pushed from
`RandomState(ring_seed)` (below; tests rebuild the ring from the same stream), the seeds of `gen_models_and_train` (100 for construction, 200 in front
of the updates).  Two recordings; they share their initial networks, every other array of train_mlp_redq.npz is prefixed with the
recording's name and `|`:

    utd3   utd = 3, policy_utd = 1, no gradient clipping
    utd4   utd = 4, policy_utd = 2, value_max_gradnorm = 0.5, policy_max_gradnorm = 0.05 (both clips bite: the actor schedule and clipping)

    policy0|<module>|<key>, value0|...                the initial networks (state dicts; the target critic starts as a copy of value0)
    <rec>|noise<k>                                    the k-th Gaussian draw of the three `train_one_batch()` calls, in call order: per pass
                                                      the target's policy sample, then - on passes with an actor step - the actor's
    <rec>|policy3|..., <rec>|value3|..., <rec>|target3|...   the networks behind the third call
    <rec>|log_alpha3                                  `log_sac_alpha` behind the third call

train_mlp_meta.json holds per recording the settings, `ring_seed`, the number of draws and `logs`, the three returned log dicts.

The ring's stream.  AdamW's first step is lr g / (|g| + eps): for a parameter element whose first gradient is what rounding left of
terms that cancel, its sign - a whole step of +-lr - is the summation order of the reference's GEMM library, and the recorded value of
that element is no property of the algorithm (with `RandomState(9)` one critic weight has a first gradient of -9.4e-8 beside 0.07 in
its column; a relative perturbation of 3e-7 on the reference's own GEMM outputs moves its final value by 1.1e-4).  The generator
therefore looks, in the reference alone, at every element's gradient at its optimizer's first step, and takes the first stream
`RandomState(9), RandomState(10), ...` for which no element of either recording has a non-zero gradient below RESIDUE (1e-5) of the
largest of its tensor.  It asserts that the recordings it writes have none, so tests hold EVERY element to the trainers' bar.
"""
import json
import os

import numpy as np
import torch

import generate_golden as G

LENS = [12, 5, 7, 12, 4, 9, 6]
RESIDUE = 1e-5
RECORDINGS = {'utd3': dict(utd=3, policy_utd=1, value_max_gradnorm=None, policy_max_gradnorm=None),
              'utd4': dict(utd=4, policy_utd=2, value_max_gradnorm=0.5, policy_max_gradnorm=0.05)}


def record(name, over, ring_seed):
    """One recording -> (its arrays, its meta entry, the residue elements [network, module, key, flat index])."""
    from offpolicy_rnn.algorithm.sac_mlp_redq_ensemble_q import SAC_MLP_REDQ_EnsembleQ
    from offpolicy_rnn.buffers.replay_memory import Transition
    obs, act, T = G.ENV['obs'], G.ENV['act'], G.ENV['T']
    out = {}
    torch.manual_seed(100)
    np.random.seed(100)
    par = G.make_parameter('fc', alg_name='sac_mlp_redq_ensemble_q', sac_batch_size=16, redq_m=2, rnn_fix_length=0,
                           value_embedding_layer_type=['efc-4'] * 3, value_layer_type=['efc-4'] * 3,
                           policy_embedding_layer_type=['fc'] * 3, policy_layer_type=['fc'] * 3, state_action_encoder=False, **over)
    alg = SAC_MLP_REDQ_EnsembleQ(par)
    pre = f'{name}|'
    out.update(G.flat_sd(alg.policy.state_dict(), 'policy0|'))
    out.update(G.flat_sd(alg.values[0].state_dict(), 'value0|'))
    rs = np.random.RandomState(ring_seed)
    for n in LENS:
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
    draws = []
    randn_like = torch.randn_like

    def recording_randn_like(t, *a, **k):
        z = randn_like(t, *a, **k)
        draws.append(G.t2n(z))
        return z

    torch.manual_seed(200)
    np.random.seed(200)
    torch.randn_like = recording_randn_like
    try:
        logs = [{k: float(v) for k, v in alg.train_one_batch().items()} for _ in range(3)]
    finally:
        torch.randn_like = randn_like
    assert all(np.isfinite(v) for log in logs for v in log.values())
    for k, z in enumerate(draws):
        out[f'{pre}noise{k}'] = z.astype(np.float32)
    out.update(G.flat_sd(alg.policy.state_dict(), pre + 'policy3|'))
    out.update(G.flat_sd(alg.values[0].state_dict(), pre + 'value3|'))
    out.update(G.flat_sd(alg.target_values[0].state_dict(), pre + 'target3|'))
    out[pre + 'log_alpha3'] = G.t2n(alg.log_sac_alpha)
    if hasattr(alg, 'process_pool'):
        alg.process_pool.shutdown()
    entry = dict(over, lens=LENS, ring_seed=ring_seed, sac_batch_size=16, redq_m=2, ensemble=4, draws=len(draws), logs=logs)
    return out, entry, residue


def gen_mlp_train():
    for ring_seed in range(9, 9 + 64):
        out, meta, found = {}, {}, []
        for name, over in RECORDINGS.items():
            arrays, meta[name], residue = record(name, over, ring_seed)
            assert all(np.array_equal(out.get(k, v), v) for k, v in arrays.items() if k.startswith(('policy0|', 'value0|')))   # same seed, same stacks
            out.update(arrays)
            found += residue
        print('ring stream', ring_seed, ':', len(found), 'first-step gradients that are rounding residue', found)
        if not found:
            break
    assert not found, 'no ring stream without a residue element'
    np.savez_compressed(os.path.join(G.OUT, 'train_mlp_redq.npz'), **out)
    with open(os.path.join(G.OUT, 'train_mlp_meta.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print('train mlp: ring stream', ring_seed, {name: (m['draws'], m['logs'][-1]['critic_loss']) for name, m in meta.items()})


if __name__ == '__main__':
    assert os.path.isdir(G.REF), f'{G.REF} not found: fixtures can only be regenerated in the build container'
    G.install_stubs()
    torch.set_num_threads(4)
    gen_mlp_train()
