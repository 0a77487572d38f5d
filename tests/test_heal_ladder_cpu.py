"""CPU: DiffNet's self-healing ladder as a table, driven through its two entry points — ``_guarded_handoffs`` (guard_mode 'same_call') and
``_check_deferred_own`` (guard_mode 'deferred').  The ladder makes no GPU call of its own: the library is replaced by a recorder of
(symbol, int arguments), the handle by a dummy pointer, and the health words / the launch path are scripted.  Every row runs on a fresh
net and asserts the switch calls in order, the ladder's state, the runs / restores (same_call) and the message.  The GPU side, with
injected give-ups: tests/test_gpu_handoff.py, tests/test_gpu_soak.py."""
import warnings
from ctypes import c_void_p

import pytest
import torch

from bisinger_amd import _lib
from tests.util import use_config

H2Q, H2, PARTS, SPLIT = 'bsg_diffnet_set_h2q', 'bsg_diffnet_set_h2', 'bsg_diffnet_set_parts', 'bsg_diffnet_set_split'


class Recorder:
    """Stands in for the loaded library: every entry records (symbol, its int arguments) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name,) + tuple(a for a in args if isinstance(a, int)))
            return 0
        return entry


@pytest.fixture
def net(monkeypatch):
    """-> (a fresh DiffNet on the CPU with a dummy handle, the recorder that _lib.load() returns)."""
    from bisinger_amd.diffnet import DiffNet
    use_config()
    rec = Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: rec)
    n = DiffNet(80)
    n._h, n._h_key = c_void_p(1), n._key()
    yield n, rec
    n._h = n._h_key = None      # the dummy pointer must never reach the library's destroy


def state(n, name):
    """A ladder attribute; absent (nothing has gone wrong yet) reads as False / 0."""
    return getattr(n, name, False)


def same_call(n, healths, path, uses=True, **pre):
    """One _guarded_handoffs call with scripted (give, rng) reads -> (runs, restores, warnings).  `path`: the launch form every event
    is read with, or a list, one per event."""
    for k, v in pre.items():
        setattr(n, k, v)
    script = list(healths)
    paths = iter(path) if isinstance(path, list) else None
    n.uses_handoffs = lambda B, T: uses
    n.take_health = lambda: script.pop(0)
    n.last_path = lambda: next(paths) if paths else path
    n.gemm_range_take = lambda: 0
    runs, restores = [], []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        n._guarded_handoffs(lambda: runs.append(1), 1, 320, lambda: restores.append(1))
    assert not script, 'a scripted health read was not taken'
    return len(runs), len(restores), [str(x.message) for x in w]


class Reads:
    """Stands in for the _DeferredWord of a handle: `words` are the completed reads, oldest first."""

    def __init__(self, words):
        self.words, self.dropped = [list(w) for w in words], 0

    def armed(self):
        return True

    def take(self, block):
        w, self.words = self.words, []
        return w

    def drop_pending(self):
        self.dropped += 1


def deferred(n, words, path, **pre):
    """One _check_deferred_own(True) over the reads `words` -> (the Reads stub, health takes, the BsgError's text or None)."""
    for k, v in pre.items():
        setattr(n, k, v)
    takes = []
    n._deferred = Reads(words)
    n.take_health = lambda: takes.append(1) or (0, 0)
    n.last_path = lambda: path
    try:
        n._check_deferred_own(True)
    except _lib.BsgError as e:
        return n._deferred, len(takes), str(e)
    return n._deferred, len(takes), None


# ---------------------------------------------------------------------------------------------------- same_call: the range tier
def test_same_call_range_event_of_the_16_row_launch_takes_the_32_row_launch(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(0, 5), (0, 0)], 'stack_h2q')
    assert rec.calls == [(H2Q, 0)]
    assert state(n, '_h2q_range_off') is True and state(n, '_h2q_strikes') == 1      # nothing is bound: True stands for the condition
    assert state(n, '_h2_range_off') is False and not state(n, '_h2_strikes')
    assert (runs, restores) == (2, 1)
    assert len(msgs) == 1 and all(s in msgs[0] for s in ('5 waves', '3750', '32-row launch', '60000', 'about 8 % slower')), msgs
    assert 'fp32 matrix pipe' not in msgs[0]
    assert not state(n, 'split_disabled') and not state(n, 'parts_disabled')


def test_same_call_range_event_remembers_the_bound_condition(net):
    n, rec = net
    cond = torch.zeros(1, 4, 8)
    n._bound = (cond, cond._version, 1, 8)
    same_call(n, [(0, 5), (0, 0)], 'stack_h2q_tail')
    assert rec.calls == [(H2Q, 0)] and n._h2q_range_off is cond


def test_same_call_range_event_with_the_16_row_launch_already_off_takes_the_fp32_pipe(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(0, 5), (0, 0)], 'stack_h2q', _h2q_range_off=True)
    assert rec.calls == [(H2, 0)]
    assert state(n, '_h2_range_off') is True and state(n, '_h2_strikes') == 1 and not state(n, '_h2q_strikes')
    assert (runs, restores) == (2, 1)
    assert len(msgs) == 1 and all(s in msgs[0] for s in ('60000', 'fp16 range of the split-fp16 launch', 'fp32 matrix pipe')), msgs


def test_same_call_range_event_of_the_32_row_launch_takes_the_fp32_pipe(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(0, 5), (0, 0)], 'stack_h2')
    assert rec.calls == [(H2, 0)]
    assert state(n, '_h2_range_off') is True and state(n, '_h2_strikes') == 1
    assert state(n, '_h2q_range_off') is False and not state(n, '_h2q_strikes')
    assert (runs, restores) == (2, 1)
    assert len(msgs) == 1 and 'stack_h2' in msgs[0] and '60000' in msgs[0], msgs


def test_same_call_range_tiers_one_per_repeat(net):
    """The 32-row launch trips too: the second repeat goes down to the fp32 pipe."""
    n, rec = net
    runs, restores, msgs = same_call(n, [(0, 5), (0, 7), (0, 0)], ['stack_h2q', 'stack_h2'])
    assert rec.calls == [(H2Q, 0), (H2, 0)] and (runs, restores) == (3, 2) and len(msgs) == 2
    assert '3750' in msgs[0] and '7 waves' in msgs[1] and 'fp32 matrix pipe' in msgs[1], msgs
    assert state(n, '_h2q_strikes') == 1 and state(n, '_h2_strikes') == 1


# ---------------------------------------------------------------------------------------------------- same_call: the give-up tier
def test_same_call_give_up_of_a_part_launch_takes_the_part_forms_off(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(3, 0), (0, 0)], 'stack_h2_quad', _clean_calls_parts=7)
    assert rec.calls == [(PARTS, 0)]
    assert state(n, 'parts_disabled') is True and state(n, '_clean_calls_parts') == 0 and not state(n, 'split_disabled')
    assert (runs, restores) == (2, 1)
    assert len(msgs) == 1 and all(s in msgs[0] for s in ('3 inter-workgroup hand-offs gave up', 'part launch', 'stack_h2_quad',
                                                         str(n.CLEAN_CALLS_TO_REENABLE))), msgs


def test_same_call_give_up_of_a_part_launch_with_part_forms_off_takes_every_hand_off_launch_off(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(3, 0), (0, 0)], 'stack_h2_quad', parts_disabled=True, _clean_calls=9)
    assert rec.calls == [(SPLIT, 0)]
    assert state(n, 'split_disabled') is True and state(n, '_clean_calls') == 0 and state(n, 'parts_disabled') is True
    assert (runs, restores) == (2, 1)
    assert len(msgs) == 1 and 'hand-offs gave up' in msgs[0] and 'part launch' not in msgs[0], msgs


def test_same_call_give_up_of_another_launch_takes_every_hand_off_launch_off(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(3, 0), (0, 0)], 'split2')
    assert rec.calls == [(SPLIT, 0)]
    assert state(n, 'split_disabled') is True and state(n, '_clean_calls') == 0 and not state(n, 'parts_disabled')
    assert (runs, restores) == (2, 1)
    assert len(msgs) == 1 and all(s in msgs[0] for s in ('3 inter-workgroup hand-offs gave up', str(n.CLEAN_CALLS_TO_REENABLE),
                                                         'fp32 matrix pipe')) and 'part launch' not in msgs[0], msgs


def test_same_call_event_with_split_launches_off_is_an_error(net):
    n, rec = net
    for k, v in dict(uses_handoffs=lambda B, T: True, last_path=lambda: 'split2', gemm_range_take=lambda: 0).items():
        setattr(n, k, v)
    script = [(3, 0), (1, 0)]
    n.take_health = lambda: script.pop(0)
    runs = []
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        with pytest.raises(_lib.BsgError, match='1 inter-workgroup hand-offs gave up with split launches off'):
            n._guarded_handoffs(lambda: runs.append(1), 1, 320, None)
    assert rec.calls == [(SPLIT, 0)] and len(runs) == 2 and state(n, 'split_disabled') is True


def test_same_call_give_up_and_range_event_together_heal_the_give_up_only(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(3, 2), (0, 0)], 'stack_h2_quad')
    assert rec.calls == [(PARTS, 0)]
    assert state(n, 'parts_disabled') is True
    assert state(n, '_h2_range_off') is False and state(n, '_h2q_range_off') is False
    assert not state(n, '_h2_strikes') and not state(n, '_h2q_strikes')
    assert (runs, restores) == (2, 1) and len(msgs) == 1 and 'part launch' in msgs[0]


def test_same_call_five_tiers_and_still_invalid_is_an_error(net):
    n, rec = net
    for k, v in dict(uses_handoffs=lambda B, T: True, last_path=lambda: 'stack_h2', gemm_range_take=lambda: 0,
                     take_health=lambda: (0, 5)).items():
        setattr(n, k, v)
    runs = []
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        with pytest.raises(_lib.BsgError, match='stayed invalid through every fallback tier'):
            n._guarded_handoffs(lambda: runs.append(1), 1, 320, None)
    assert rec.calls == [(H2, 0)] * 5 and len(runs) == 6 and state(n, '_h2_strikes') == 5


def test_same_call_shape_without_hand_offs_reads_nothing(net):
    n, rec = net
    assert same_call(n, [], 'layer', uses=False) == (1, 0, [])
    assert rec.calls == []


# ---------------------------------------------------------------------------------------------------- deferred
@pytest.mark.parametrize('words,path,calls,hints', [
    ([0, 5, 0], 'stack_h2q', [(H2Q, 0)], ['5 waves', '3750', '32-row launch']),
    ([0, 5, 0], 'stack_h2', [(H2, 0)], ['5 waves', 'fp32 matrix pipe']),
    ([3, 0, 0], 'stack_h2_quad', [(PARTS, 0)], ['3 inter-workgroup hand-offs gave up', 'part launch']),
    ([0, 0, 3], 'split2', [(SPLIT, 0)], ['3 inter-workgroup hand-offs gave up']),
    ([3, 0, 2], 'stack_h2_quad', [(SPLIT, 0)], ['5 inter-workgroup hand-offs gave up']),      # a split launch gave up as well: not the part tier
    ([3, 0, 0], 'split2', [(SPLIT, 0)], ['3 inter-workgroup hand-offs gave up']),
    ([3, 2, 0], 'stack_h2_quad', [(H2, 0), (PARTS, 0)], ['2 waves', 'fp32 matrix pipe', '3 inter-workgroup hand-offs gave up', 'part launch']),
])
def test_deferred_demotes_from_one_read_and_raises(net, words, path, calls, hints):
    n, rec = net
    reads, takes, err = deferred(n, [[0, 0, 0], words], path)      # cumulative words: the newest read says everything
    assert rec.calls == calls
    assert err is not None and 'PREVIOUS call' in err and all(h in err for h in hints), err
    assert ('part launch' in err) == ((PARTS, 0) in calls), err
    assert str(n.CLEAN_CALLS_TO_REENABLE) in err or not (words[0] or words[2])
    assert reads.dropped == 1 and takes == 1
    assert bool(state(n, 'parts_disabled')) == ((PARTS, 0) in calls) and bool(state(n, 'split_disabled')) == ((SPLIT, 0) in calls)
    assert state(n, '_h2q_strikes') == calls.count((H2Q, 0)) and state(n, '_h2_strikes') == calls.count((H2, 0))
    assert (state(n, '_h2q_range_off') is True) == ((H2Q, 0) in calls) and (state(n, '_h2_range_off') is True) == ((H2, 0) in calls)


def test_deferred_part_give_up_with_part_forms_off_takes_every_hand_off_launch_off(net):
    n, rec = net
    reads, takes, err = deferred(n, [[3, 0, 0]], 'stack_h2_quad', parts_disabled=True)
    assert rec.calls == [(SPLIT, 0)] and state(n, 'split_disabled') is True and state(n, '_clean_calls') == 0
    assert 'PREVIOUS call' in err and reads.dropped == 1


def test_deferred_range_event_with_the_16_row_launch_already_off(net):
    n, rec = net
    deferred(n, [[0, 5, 0]], 'stack_h2q', _h2q_range_off=True)
    assert rec.calls == [(H2, 0)] and state(n, '_h2_strikes') == 1 and not state(n, '_h2q_strikes')


def test_deferred_nothing_completed_or_no_handle_looks_at_nothing(net):
    n, rec = net
    assert deferred(n, [], 'stack_h2q')[1:] == (0, None) and rec.calls == []
    n._h = None
    reads, takes, err = deferred(n, [[3, 0, 0]], 'stack_h2_quad')
    assert (takes, err, reads.dropped, rec.calls) == (0, None, 0, []) and reads.words == [[3, 0, 0]]


# ---------------------------------------------------------------------------------------------------- clean calls
def test_same_call_clean_calls_bring_the_part_forms_back(net):
    n, rec = net
    N = n.CLEAN_CALLS_TO_REENABLE
    n.parts_disabled = True
    for i in range(N - 1):
        assert same_call(n, [(0, 0)], 'stack_h2q') == (1, 0, [])
    assert rec.calls == [] and n.parts_disabled is True and state(n, '_clean_calls_parts') == N - 1
    assert same_call(n, [(0, 0)], 'stack_h2q') == (1, 0, [])
    assert rec.calls == [(PARTS, 1)] and n.parts_disabled is False and n._clean_calls_parts == 0


def test_same_call_counts_a_clean_look_for_the_part_forms_on_the_first_look_only(net):
    n, rec = net
    runs, restores, msgs = same_call(n, [(0, 5), (0, 0)], 'stack_h2', parts_disabled=True, _clean_calls_parts=4)
    assert rec.calls == [(H2, 0)] and runs == 2 and n.parts_disabled is True and n._clean_calls_parts == 4


def test_same_call_clean_calls_bring_both_tiers_back_together(net):
    n, rec = net
    N = n.CLEAN_CALLS_TO_REENABLE

    def no_read():
        raise AssertionError('a demoted handle launches nothing that hands data over: no read, no wait')
    n.split_disabled, n.parts_disabled, n._clean_calls, n._clean_calls_parts = True, True, N - 2, 5
    n.uses_handoffs = n.take_health = lambda *a: no_read()
    runs = []
    n._guarded_handoffs(lambda: runs.append(1), 1, 320, None)
    assert rec.calls == [] and n._clean_calls == N - 1 and n.split_disabled is True and n._clean_calls_parts == 5
    n._guarded_handoffs(lambda: runs.append(1), 1, 320, None)
    assert rec.calls == [(SPLIT, 1), (PARTS, 1)] and len(runs) == 2
    assert (n.split_disabled, n.parts_disabled, n._clean_calls, n._clean_calls_parts) == (False, False, 0, 0)


def test_same_call_split_comes_back_alone_when_the_part_forms_are_on(net):
    n, rec = net
    n.split_disabled, n._clean_calls = True, n.CLEAN_CALLS_TO_REENABLE - 1
    n._guarded_handoffs(lambda: None, 1, 320, None)
    assert rec.calls == [(SPLIT, 1)] and n.split_disabled is False and n._clean_calls == 0


def test_deferred_clean_read_of_k_words_counts_k(net):
    n, rec = net
    N = n.CLEAN_CALLS_TO_REENABLE
    reads, takes, err = deferred(n, [[0, 0, 0]] * 3, 'stack_h2q', parts_disabled=True, split_disabled=True)
    assert (takes, err, reads.dropped, rec.calls) == (0, None, 0, [])
    assert n._clean_calls_parts == 3 and n._clean_calls == 3
    # the split comes back and brings the part forms with it
    n._clean_calls = N - 2
    assert deferred(n, [[0, 0, 0]] * 2, 'stack_h2q')[1:] == (0, None)
    assert rec.calls == [(SPLIT, 1), (PARTS, 1)]
    assert (n.split_disabled, n.parts_disabled, n._clean_calls, n._clean_calls_parts) == (False, False, 0, 0)


def test_deferred_clean_reads_bring_the_part_forms_back(net):
    n, rec = net
    N = n.CLEAN_CALLS_TO_REENABLE
    deferred(n, [[0, 0, 0]] * (N - 1), 'stack_h2q', parts_disabled=True)
    assert rec.calls == [] and n._clean_calls_parts == N - 1
    deferred(n, [[0, 0, 0]], 'stack_h2q')
    assert rec.calls == [(PARTS, 1)] and n.parts_disabled is False and n._clean_calls_parts == 0
    deferred(n, [[0, 0, 0]] * 4, 'stack_h2q')      # nothing is demoted: nothing is counted
    assert state(n, '_clean_calls_parts') == 0 and not state(n, '_clean_calls')


# ---------------------------------------------------------------------------------------------------- _rearm
def test_rearm_with_another_condition_tries_the_faster_launch_again(net):
    n, rec = net
    old, new = torch.zeros(1, 4, 8), torch.zeros(1, 4, 8)
    n._h2q_range_off, n._h2q_strikes = old, n.H2_STRIKES_MAX - 1
    n._rearm(old)
    assert rec.calls == [] and n._h2q_range_off is old      # the same condition: it would trip again
    n._rearm(new)
    assert rec.calls == [(H2Q, 1)] and n._h2q_range_off is False and n._h2q_strikes == n.H2_STRIKES_MAX - 1
    assert state(n, '_h2_range_off') is False


def test_rearm_after_the_last_strike_stays_demoted(net):
    n, rec = net
    old, new = torch.zeros(1, 4, 8), torch.zeros(1, 4, 8)
    n._h2q_range_off, n._h2q_strikes = old, n.H2_STRIKES_MAX
    n._h2_range_off, n._h2_strikes = True, 1
    n._rearm(new)
    assert rec.calls == [(H2, 1)] and n._h2q_range_off is new and n._h2_range_off is False


def test_rearm_inside_a_repeated_pass_keeps_the_fallback(net):
    n, rec = net
    old, new = torch.zeros(1, 4, 8), torch.zeros(1, 4, 8)
    n._h2q_range_off, n._h2_range_off = old, old
    st = _lib._state()
    st.in_retry = True
    try:
        n._rearm(new)
    finally:
        st.in_retry = False
    assert rec.calls == [] and n._h2q_range_off is new and n._h2_range_off is new
