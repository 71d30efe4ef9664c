"""The environments that exist as kernels (csrc/env_step.hip), one record each: everything `DeviceEnvEval` (utility/policy_eval.py) and
`DeviceCollector` (utility/device_collect.py) need to know about the environment they step inside the policy step's graph.

A record says which observation / action widths it steps, which policy head it reads and which of its output columns, how many bytes of
device state a row has and how they are viewed, what an episode's init payload is (the T-Maze's goal side, Wind's wind vector, Catch's
fruit and basket columns), which two `ops` entries run it, and how the state comes back into the host environment object.
`device_env_kind(env)` finds the record of an environment object (None: it has no device step)."""
import numpy as np
import torch

from . import catch, tmaze, wind


class DeviceEnvKind:
    """What the records share.  Every kernel keeps three consecutive int32 next to its environment's own state - steps of the episode,
    episodes started, running (csrc/env_step.hip `BLEN`, `BSTARTED`, `BRUNNING`) - at byte `book_offset` of a row's state."""

    @staticmethod
    def episode_length(cfg) -> int:
        return int(cfg['episode_length'])

    @classmethod
    def finished(cls, state_np):
        """state_np: the row's state bytes on the host -> (steps taken, still running)."""
        book = state_np[cls.book_offset:cls.book_offset + 12].view(np.int32)
        return int(book[0]), bool(book[2])


class TMazeKind(DeviceEnvKind):
    """Discrete T-Maze (env_utils/tmaze.py): int32 words x, y, goal_y, oracle_visited, t, ep_len, episodes_started, running."""
    obs_dim, act_dim = 2, 4
    categorical, policy_words = True, 'a categorical one'
    state_bytes = 4 * 8
    payload_dtype, payload_np, payload_width = torch.int32, np.int32, 1
    book_offset = 4 * 5

    @staticmethod
    def steps(env) -> bool:
        return tmaze.device_steppable(env)

    @staticmethod
    def policy_ok(policy) -> bool:
        return bool(getattr(policy, 'categorical', False))

    @staticmethod
    def action(out_dev, sampled: bool):
        """The head's output columns the kernel reads: the mode index (evaluation) or the sampled one (rollout)."""
        return out_dev[:, 1 if sampled else 0]

    @staticmethod
    def state_views(block, B):
        """uint8 [B * state_bytes] -> the state tensors the `ops` entries take."""
        return (block.view(torch.int32).view(B, 8),)

    @staticmethod
    def eval_step(ops, cfg, init, action, payload, n_ep, state, ret_acc, ep_ret, ep_len, in_dev, flags):
        ops.tmaze_step(cfg, init, action, payload[:, :, 0], n_ep, state[0], ret_acc, ep_ret, ep_len, in_dev, flags)

    @staticmethod
    def collect_step(ops, cfg, name2range, init, action, payload, state, ret_acc, traj, max_episode_steps, in_dev):
        ops.tmaze_collect_step(cfg, name2range, init, action, payload[:, 0], state[0], ret_acc, traj, max_episode_steps, in_dev)

    @staticmethod
    def eval_payloads(envs, n, draw_task):
        """The payload of episodes 0 .. n - 1 (episode k runs on row k % rows), drawn as the host loop draws: each row's own stream, in
        the row's episode order."""
        rows = len(envs)
        out = [None] * n
        for r, env in enumerate(envs):
            for k in range(r, n, rows):
                out[k] = (env.draw_goal(),)
        return out

    @staticmethod
    def eval_extras(n) -> dict:
        return {}

    @staticmethod
    def behind_reset(env) -> bool:
        return env.time_step == 0 and env.x == env.oracle_length and env.y == 0

    @staticmethod
    def current_payload(env):
        return (env.goal_y,)

    @staticmethod
    def next_payload(alg):
        """`env_reset()`'s draw for the next training episode, recorded in the environment object."""
        alg.env.goal_y = alg.env.draw_goal()
        return (alg.env.goal_y,)

    @staticmethod
    def sync_env(env, state, row, o, a):
        """The environment object's fields from the device state; -> (state_np, last_state_np, last_action_np) as the host loop holds them
        mid-episode.  row: the step's input row (fp32)."""
        st = state[0][0].cpu().numpy()
        env.x, env.y, env.goal_y, env.oracle_visited, env.time_step = int(st[0]), int(st[1]), int(st[2]), bool(st[3]), int(st[4])
        return (row[:o].copy().reshape(1, -1), row[o:2 * o].copy().reshape(1, -1), row[2 * o:2 * o + a].astype(np.float64).reshape(1, -1))


class WindKind(DeviceEnvKind):
    """Wind-v0 (env_utils/wind.py): doubles x, y, wind_x, wind_y, last_x, last_y, then int32 words clock, ep_len, episodes_started, running."""
    obs_dim, act_dim = 2, 2
    categorical, policy_words = False, 'a tanh-Gaussian SAC one'
    state_bytes = 8 * 6 + 4 * 4
    payload_dtype, payload_np, payload_width = torch.float64, np.float64, 2
    book_offset = 8 * 6 + 4 * 1

    @staticmethod
    def steps(env) -> bool:
        return wind.device_steppable(env)

    @staticmethod
    def policy_ok(policy) -> bool:                           # (TD3's deterministic policy with clipped noise keeps the host loop)
        return not bool(getattr(policy, 'categorical', False)) and not hasattr(policy, 'sample_std')

    @staticmethod
    def action(out_dev, sampled: bool):
        """mean | sample | logp: the evaluation reads the mean, the rollout the sample."""
        return out_dev[:, 2:4] if sampled else out_dev[:, 0:2]

    @staticmethod
    def state_views(block, B):
        return block[:B * 48].view(torch.float64).view(B, 6), block[B * 48:].view(torch.int32).view(B, 4)

    @staticmethod
    def eval_step(ops, cfg, init, action, payload, n_ep, state, ret_acc, ep_ret, ep_len, in_dev, flags):
        ops.wind_step(cfg, init, action, payload, n_ep, state[0], state[1], ret_acc, ep_ret, ep_len, in_dev, flags)

    @staticmethod
    def collect_step(ops, cfg, name2range, init, action, payload, state, ret_acc, traj, max_episode_steps, in_dev):
        ops.wind_collect_step(cfg, name2range, init, action, payload, state[0], state[1], ret_acc, traj, max_episode_steps, in_dev)

    @staticmethod
    def eval_payloads(envs, n, draw_task):
        """One task per episode from the evaluator's private stream, in the order the host scheduler hands episodes out: exactly n draws."""
        return [tuple(envs[k % len(envs)].winds[draw_task()]) for k in range(n)]

    @staticmethod
    def eval_extras(n) -> dict:
        """What the wrapper's info adds to the host loop's result: the last report of an episode is `done_mdp = True`."""
        return {'done_mdpTest': [1.0] * n}

    @staticmethod
    def behind_reset(env) -> bool:
        return env.step_count == 0 and not env._state.any()

    @staticmethod
    def current_payload(env):
        return tuple(env.get_current_task())

    @staticmethod
    def next_payload(alg):
        """`env_reset()`'s draw for the next training episode: one task from the global numpy stream."""
        alg.env.reset(alg.draw_train_task())
        return tuple(alg.env.get_current_task())

    @staticmethod
    def sync_env(env, state, row, o, a):
        ps, words = state[0][0].cpu().numpy(), state[1][0].cpu().numpy()
        env._state, env._wind, env.step_count = ps[0:2].copy(), ps[2:4].copy(), int(words[0])
        env.done_mdp = env.step_count >= env._max_episode_steps
        return ps[0:2].copy().reshape(1, -1), ps[4:6].copy().reshape(1, -1), row[2 * o:2 * o + a].copy().reshape(1, -1)


class CatchKind(DeviceEnvKind):
    """Catch-<runs>-v0 (env_utils/catch.py), runs <= 40: int32 words fruit_row, fruit_col, basket, catch_count, t, accumulated, ep_len,
    episodes_started, running, a pad word, then the episode's draws ns[40] | ms[40] - the payload, which the kernel's reset copies into the
    row because a soft reset reads it in mid-episode."""
    obs_dim, act_dim = 49, 3
    categorical, policy_words = True, 'a categorical one'
    MAX_RUNS, STATE_WORDS, DRAWS = 40, 90, 10               # RESEL_CATCH_MAX_RUNS, RESEL_CATCH_STATE_WORDS; DRAWS: the first word of ns
    state_bytes = 4 * STATE_WORDS
    payload_dtype, payload_np, payload_width = torch.int32, np.int32, 2 * MAX_RUNS
    book_offset = 4 * 6

    steps = staticmethod(catch.device_steppable)
    # the categorical head, its mode / sample columns and an info-free evaluation, as the T-Maze's
    policy_ok, action, eval_extras = (staticmethod(f) for f in (TMazeKind.policy_ok, TMazeKind.action, TMazeKind.eval_extras))

    @classmethod
    def state_views(cls, block, B):
        return (block.view(torch.int32).view(B, cls.STATE_WORDS),)

    @staticmethod
    def eval_step(ops, cfg, init, action, payload, n_ep, state, ret_acc, ep_ret, ep_len, in_dev, flags):
        ops.catch_step(cfg, init, action, payload, n_ep, state[0], ret_acc, ep_ret, ep_len, in_dev, flags)

    @staticmethod
    def collect_step(ops, cfg, name2range, init, action, payload, state, ret_acc, traj, max_episode_steps, in_dev):
        ops.catch_collect_step(cfg, name2range, init, action, payload, state[0], ret_acc, traj, max_episode_steps, in_dev)

    @classmethod
    def _row(cls, ns, ms):
        """(ns, ms) of an episode -> the kernel's payload row: ns[40] | ms[40], zeros behind the runs."""
        out = np.zeros(2 * cls.MAX_RUNS, dtype=np.int32)
        out[:len(ns)], out[cls.MAX_RUNS:cls.MAX_RUNS + len(ms)] = ns, ms
        return out

    @classmethod
    def eval_payloads(cls, envs, n, draw_task):
        """As the T-Maze's: each row's own stream, in the row's episode order - the two draws its `reset()` makes."""
        rows = len(envs)
        out = [None] * n
        for r, env in enumerate(envs):
            for k in range(r, n, rows):
                out[k] = cls._row(*env.draw_fruits())
        return out

    @staticmethod
    def behind_reset(env) -> bool:
        return env.time_step == 0 and env.fruit_row == 0 and env.catch_count == 1 and env.accumulated == 0

    @classmethod
    def current_payload(cls, env):
        return cls._row(env.ns, env.ms)

    @classmethod
    def next_payload(cls, alg):
        """`env_reset()`'s draws for the next training episode, recorded in the environment object."""
        alg.env.ns, alg.env.ms = alg.env.draw_fruits()
        return cls._row(alg.env.ns, alg.env.ms)

    @classmethod
    def sync_env(cls, env, state, row, o, a):
        st = state[0][0].cpu().numpy()
        env.fruit_row, env.fruit_col, env.basket, env.catch_count, env.time_step, env.accumulated = (int(v) for v in st[:6])
        ns = st[cls.DRAWS:cls.DRAWS + cls.MAX_RUNS]
        env.ns, env.ms = ns[:env.runs].astype(np.int64), st[cls.DRAWS + cls.MAX_RUNS:][:env.runs].astype(np.int64)
        return (row[:o].copy().reshape(1, -1), row[o:2 * o].copy().reshape(1, -1), row[2 * o:2 * o + a].astype(np.float64).reshape(1, -1))


KINDS = (TMazeKind, WindKind)
GRID_KINDS = (CatchKind,)                                  # apart from KINDS: tests/test_wind_env_host.py holds every member of KINDS to a 2-wide observation


def device_env_kind(env):
    """The record of the kernel that steps `env`, or None."""
    for kind in KINDS + GRID_KINDS:
        if kind.steps(env):
            return kind
    return None
