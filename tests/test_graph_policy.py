"""The host bookkeeping of the update graphs (algorithm/graph_policy.py) without a GPU: the recording policy driven with key
sequences, the graph key spelled on a hand-made plan, the runs of neighbouring log slots.  The expected decisions are those of the
driver's launch path before the policy stood alone."""
from types import SimpleNamespace

from offpolicy_rnn.algorithm.graph_policy import (EAGER, RECORD, REPLAY, RecordingPolicy, exact_batch_key, exact_table_key, graph_key,
                                                  slot_runs)


def drive(policy, keys):
    """The driver's side of `decide`: a recording is stored under its key.  -> [(decision, evicted key)]"""
    out = []
    for key in keys:
        what, evicted = policy.decide(key)
        if what == RECORD:
            policy.recorded[key] = object()
        out.append((what, evicted))
    return out


def decisions(policy, keys):
    return [what for what, _ in drive(policy, keys)]


def test_warmup_then_the_second_visit_records():
    p = RecordingPolicy(warmup=3, max_graphs=4)
    assert decisions(p, 'AAAAAA') == [EAGER, EAGER, EAGER, RECORD, REPLAY, REPLAY]
    assert p.eager_fallbacks == 3 and p.steps == 6


def test_one_warmup_pass_as_the_benchmark_runs_it():
    p = RecordingPolicy(warmup=1, max_graphs=4)
    assert decisions(p, 'AAAA') == [EAGER, RECORD, REPLAY, REPLAY]
    assert p.eager_fallbacks == 1


def test_one_graph_two_shapes_the_capture_window_throttles():
    p = RecordingPolicy(warmup=0, max_graphs=1)
    # the fourth is throttled: one graph held and one recording (pass 2) inside the window
    assert drive(p, 'AABB') == [(EAGER, None), (RECORD, None), (EAGER, None), (EAGER, None)]
    assert decisions(p, 'B' * 253) == [EAGER] * 253 and p.steps == 257
    # pass 258: the recording of pass 2 has left the window of 256 passes
    assert drive(p, 'B') == [(RECORD, 'A')] and list(p.recorded) == ['B']
    assert p.seen['A'] == 2 - RecordingPolicy.RECAPTURE_HITS
    assert decisions(p, 'A' * 9) == [EAGER] * 9                                 # the window is full again
    assert p.seen['A'] == 3


def test_the_least_recently_used_recording_is_evicted():
    p = RecordingPolicy(warmup=0, max_graphs=2)
    assert decisions(p, 'AABBACC') == [EAGER, RECORD, EAGER, RECORD, REPLAY, EAGER, EAGER]      # the second C is throttled
    p.CAPTURE_WINDOW = 4
    assert drive(p, 'CCCC') == [(RECORD, 'B')] + [(REPLAY, None)] * 3           # B, not A: A was replayed after B was recorded
    assert list(p.recorded) == ['A', 'C']


def exact(i, actor=False):
    return (4, 30 + i, 29 + i, 7, actor)


def test_auto_switches_on_the_shape_after_the_last_one_the_graphs_hold():
    p = RecordingPolicy(warmup=0, buckets='auto')
    assert p.max_graphs == 4
    assert not any(p.tips(exact(i, actor)) for i in range(4) for actor in (False, True))        # the actor flag makes no shape
    assert p.buckets == 'auto'
    drive(p, 'AA')
    assert p.recorded and p.seen and p.captures
    assert p.tips(exact(4)) == 5
    assert (p.buckets, p.max_graphs) == ('on', 8)
    assert not p.recorded and not p.seen and not p.captures and not p.shapes

    p = RecordingPolicy(warmup=0, buckets='auto', sequences=2)
    assert p.max_graphs == 8 and not any(p.tips(exact(i)) for i in range(4))
    assert p.tips(exact(4)) and (p.buckets, p.max_graphs) == ('on', 16)

    p = RecordingPolicy(warmup=0, max_graphs=2, buckets='auto', sequences=2)
    assert not p.tips(exact(0)) and not p.tips(exact(0)) and p.buckets == 'auto'
    assert p.tips(exact(1)) == 2 and (p.buckets, p.max_graphs) == ('on', 2)

    p = RecordingPolicy(warmup=0, buckets='auto', can_bucket=False)             # attention layers without seq_buckets
    assert not any(p.tips(exact(i)) for i in range(40)) and p.buckets == 'auto' and not p.shapes


def test_counts_are_kept_for_the_most_recent_keys_only():
    p = RecordingPolicy(warmup=0)
    n = RecordingPolicy.SEEN_CAP + 10
    assert decisions(p, range(n)) == [EAGER] * n
    assert list(p.seen) == list(range(10, n)) and set(p.seen.values()) == {1}


def test_graph_key():
    pl = dict(nrow=6, longest=48, max_len=41, seg=SimpleNamespace(shape=(16, 4)))
    size = lambda n: SimpleNamespace(size=n)
    built = [(size(200), size(9), 41, None), (size(194), size(9), 40, None)]
    assert exact_batch_key(pl) == (6, 48, 41, 16) and exact_table_key(built) == (200, 9, 41, 194, 9, 40)
    assert graph_key(pl, (), False, True) == (6, 48, 41, 16, True)
    assert graph_key(pl, (), True, 0) == (6, 48, 16, False)
    assert graph_key(pl, exact_table_key(built), False, False) == (6, 48, 41, 16, 200, 9, 41, 194, 9, 40, False)
    assert graph_key(pl, (256, 17, 1), True, True) == (6, 48, 16, 256, 17, 1, True)
    assert [len(graph_key(pl, t, b, True)) for t, b in (((), False), ((), True), (exact_table_key(built), False), ((256, 17, 1), True))] \
        == [5, 4, 11, 7]


def test_slot_runs():
    runs = lambda slots: [slots[i:j] for i, j in slot_runs(slots)]
    assert runs([0, 1, 2, 5, 6, 9]) == [[0, 1, 2], [5, 6], [9]]
    assert runs([2, 0, 1]) == [[2], [0, 1]]                                     # ascending neighbours only
    assert runs([2, 1, 0]) == [[2], [1], [0]] and runs([4]) == [[4]] and runs([]) == []


def test_the_module_needs_no_torch():
    import ast
    import offpolicy_rnn.algorithm.graph_policy as gp
    tree = ast.parse(open(gp.__file__).read())
    names = {a.name.split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    names |= {(n.module or '').split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert 'torch' not in names
