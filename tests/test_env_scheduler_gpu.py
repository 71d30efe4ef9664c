"""The evaluation scheduler of the environment kernels (csrc/env_step.hip `eval_step_kernel`) on the two episode counts the other files
leave out together, for both environments: a row with `n_episodes == 0`, idle from the very first init, next to a row that asks for more
than J episodes and is clamped to J.  Against the replicas on the host twins (test_tmaze_env_gpu.py, test_wind_env_gpu.py), every buffer
after every call, floats through their bits: no tolerance."""
import numpy as np
import pytest
import torch

import test_tmaze_env_gpu as tmaze_tests
import test_wind_env_gpu as wind_tests

pytestmark = pytest.mark.gpu
B, J, T = 3, 2, 2


def _tmaze(rs, n):
    goals = rs.choice([-1, 1], size=(B, J)).astype(np.int32)
    return tmaze_tests.Replica(B, 0, T - 1, goals, n), goals, lambda block: block[:, 0], lambda: rs.randint(0, 4, size=B)


def _wind(rs, n):
    winds = rs.uniform(-0.08, 0.08, size=(B, J, 2))
    return wind_tests.Replica(B, T, winds, n), winds, lambda block: block[:, 1:3], lambda: rs.uniform(-1.5, 1.5, size=(B, 2))


@pytest.mark.parametrize('mod, make', [(tmaze_tests, _tmaze), (wind_tests, _wind)], ids=['tmaze', 'wind'])
def test_a_row_idle_from_init_next_to_a_row_clamped_to_J(mod, make, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops
    monkeypatch.setattr(mod, 'J', J)                            # the replica's tables are J wide
    n = np.array([0, J + 2, 1], dtype=np.int32)                 # idle from the start | more than its J payloads | idle after one episode
    rep, payload, action, draw = make(np.random.RandomState(7), n)
    assert rep.cfg['episode_length'] == T and rep.n.tolist() == [0, J, 1]
    d = mod._device(rep, payload, n)                            # the device sees the counts as asked for
    mod._call(ops, rep.cfg, True, torch.full((B, mod.LD_ACTION), float('nan'), device='cuda'), d)
    rep.init()
    mod._assert_equal(rep, d, 'init')
    running = []
    for s in range(J * T + 2):                                  # two more than row 1 needs: every row idle at the end
        block = np.full((B, mod.LD_ACTION), mod.GAP, dtype=np.float32)
        action(block)[...] = draw()                             # the columns the entry reads, gaps around them
        mod._call(ops, rep.cfg, False, torch.from_numpy(block).cuda(), d)
        rep.step(action(block))
        mod._assert_equal(rep, d, f'step {s}')
        running.append((rep.flags == 0).tolist())
    assert not any(r[0] for r in running) and (rep.ep_len[0] == -77).all()                     # row 0 never ran, its slots untouched
    assert (rep.ep_len[1] == T).all() and sum(r[1] for r in running) == J * T - J              # row 1: exactly J episodes, then idle
    assert rep.ep_len[2].tolist() == [T, -77] and (rep.flags == 1).all()
