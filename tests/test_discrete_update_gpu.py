"""The discrete-action update routed through the HIP head, value and loss kernels (`RESEL_DISCRETE_FUSED`, default on) against the
torch spelling it replaces (`RESEL_DISCRETE_FUSED=0`), on the committed fixtures `gru_sac_discrete` / `gilr_sac_discrete` (5-wide
observations, 12-step rows): three eager updates from the same seeds, the ATen ops one update dispatches, the advance of the device
generator, and the update graph."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ['gru_sac_discrete', 'gilr_sac_discrete']
DISCRETE_ONLY = ('aten::_softmax', 'aten::argmax', 'aten::gather')      # in the package these occur in the discrete blocks only


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _state(alg):
    return {'policy': alg.policy.store.flat.detach().clone().cpu(), 'value': alg.values[0].store.flat.detach().clone().cpu(),
            'target value': alg.target_values[0].store.flat.detach().clone().cpu()}


def _inside(event, name):
    """Whether the dispatcher reached `event` from inside an op called `name`.  The head's unused `torch.multinomial` draw stays with
    the switch on, and a one-sample multinomial is itself an exponential race decided by an `aten::argmax`; that nested call is the
    draw's own business, so the census counts what the update calls, not what multinomial calls."""
    parent = event.cpu_parent
    while parent is not None:
        if parent.name == name:
            return True
        parent = parent.cpu_parent
    return False


_RUNS = {}


def run(name, fused):
    """Three eager updates of the fixture with the switch set -> logs, final parameters, the device generator after the first update and
    the names of everything the second update sent through the ATen dispatcher (the first is the warm-up).  Once per (fixture, switch)."""
    if (name, fused) in _RUNS:
        return _RUNS[(name, fused)]
    from torch.profiler import profile, ProfilerActivity
    from test_host_logic import discrete_alg
    before = os.environ.get('RESEL_DISCRETE_FUSED')
    os.environ['RESEL_DISCRETE_FUSED'] = '1' if fused else '0'
    try:
        torch.manual_seed(100)
        np.random.seed(100)
        alg, _, _ = discrete_alg(name)
        assert alg.device.type == 'cuda' and alg.discrete_env
        torch.manual_seed(200)
        np.random.seed(200)
        logs, rng, seen = [], None, None
        for it in range(3):
            if it == 1:
                with profile(activities=[ProfilerActivity.CPU]) as prof:
                    logs.append(dict(alg.train_one_batch()))
                    torch.cuda.synchronize()
                seen = {e.name for e in prof.events() if not _inside(e, 'aten::multinomial')}
            else:
                logs.append(dict(alg.train_one_batch()))
            alg.grad_num += 1
            if it == 0:
                torch.cuda.synchronize()
                rng = torch.cuda.get_rng_state(alg.device).clone()
        out = dict(logs=logs, state=_state(alg), rng=rng, seen=seen)
    finally:
        if before is None:
            del os.environ['RESEL_DISCRETE_FUSED']
        else:
            os.environ['RESEL_DISCRETE_FUSED'] = before
    _RUNS[(name, fused)] = out
    return out


_val = lambda v: v[0] if isinstance(v, tuple) else v


@pytest.mark.parametrize('name', NAMES)
def test_fused_update_equals_the_torch_spelling(ops, name):
    """Logs rel 2e-3 / abs 2e-4, parameters rtol 2e-3 / atol 2e-5: what tests/test_host_logic.py applies to these fixtures."""
    on, off = run(name, True), run(name, False)
    worst = 0.0
    for it, (a, b) in enumerate(zip(on['logs'], off['logs'])):
        assert set(a) == set(b)
        for k in a:
            va, vb = _val(a[k]), _val(b[k])
            worst = max(worst, abs(va - vb) / max(abs(vb), 1e-1))
            assert va == pytest.approx(vb, rel=2e-3, abs=2e-4), (it, k, va, vb)
    print(f'\n[{name}] largest log difference (relative to max(|plain|, 0.1)): {worst:.3e}')
    for nm in on['state']:
        a, b = on['state'][nm].numpy(), off['state'][nm].numpy()
        print(f'[{name}] {nm}: largest parameter difference {np.abs(a - b).max():.3e} (largest |parameter| {np.abs(b).max():.3e})')
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-5, err_msg=nm)


@pytest.mark.parametrize('name', NAMES)
def test_fused_update_dispatches_no_discrete_aten_ops(ops, name):
    on, off = run(name, True)['seen'], run(name, False)['seen']
    print(f'\n[{name}] ATen ops of one update: {len([n for n in off if n.startswith("aten::")])} distinct with the switch off, '
          f'{len([n for n in on if n.startswith("aten::")])} with it on; gone: {sorted(off - on)}')
    for op in DISCRETE_ONLY:
        assert op in off, op                                          # the torch spelling is what the switch turns back on
        assert op not in on, op
    assert 'aten::multinomial' in on and 'aten::multinomial' in off   # the unused draw stays: it advances the generator


@pytest.mark.parametrize('name', NAMES)
def test_device_generator_advances_alike(ops, name):
    assert torch.equal(run(name, True)['rng'], run(name, False)['rng'])


@pytest.mark.parametrize('rnn', ['gru', 'gilr'])
def test_graphed_fused_update_equals_the_eager_update(ops, rnn, monkeypatch):
    """tests/test_discrete_rollout_gpu.py::test_graphed_discrete_update_equals_the_eager_update with the switch pinned on: its trainer
    (batches of one recurring shape, so the second update is recorded and the third replayed) and its tolerance."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from test_discrete_rollout_gpu import _update_alg
    monkeypatch.setenv('RESEL_DISCRETE_FUSED', '1')

    def state(alg):
        return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(),
                alg.target_values[0].store.flat.detach().clone(), alg.log_sac_alpha.detach().clone()]

    eager = _update_alg(rnn)
    logs_e = []
    for _ in range(3):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _update_alg(rnn)
    assert GraphedUpdate.refusal(graphed) is None
    g = GraphedUpdate(graphed, warmup=1)
    logs_g = []
    try:
        for _ in range(3):
            logs_g.append(dict(g.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        assert len(g.graphs) == 1 and g.eager_fallbacks == 1
    finally:
        g.close()
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), state(graphed), state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg)
        for k in le:
            ve, vg = _val(le[k]), _val(lg[k])
            assert abs(ve - vg) <= 2e-5 * max(1.0, abs(ve)), (k, ve, vg)
