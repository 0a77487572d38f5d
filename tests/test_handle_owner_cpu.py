"""CPU: the handle life cycle that _lib.HandleOwner gives the six handle owners (DiffNet, FastSpeech2MIDI for _FastSpeech2Base,
HifiGanGenerator, PitchExtractor, ParallelWaveGANGenerator, FFT) — the refusal of CPU parameters before the library is loaded,
release() / __del__ / last_path() / poison_workspace() against a recorder in the library's place — and the length normaliser
_lib.row_lengths.  No GPU and no built library."""
import gc
from ctypes import c_void_p

import pytest
import torch
import yaml

from bisinger_amd import _lib
from tests import pwg_ref
from tests.util import ROOT, use_config

torch.set_grad_enabled(False)


class _Enc:
    def __len__(self):
        return 65

    def pad(self):
        return 0


def _diffnet():
    from bisinger_amd.diffnet import DiffNet
    return DiffNet(80)


def _fs2():
    from bisinger_amd.fs2 import FastSpeech2MIDI
    return FastSpeech2MIDI(_Enc(), 80)


def _hifigan():
    from bisinger_amd.hifigan import HifiGanGenerator
    g = HifiGanGenerator(yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml')))
    g.remove_weight_norm()
    return g


def _pe():
    from bisinger_amd.pe import PitchExtractor
    return PitchExtractor()


def _pwg(fold=True):
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    g = ParallelWaveGANGenerator(**pwg_ref.params(False))
    if fold:
        g.remove_weight_norm()
    return g


def _fft():
    from bisinger_amd.candidate_decoder import FFT
    return FFT(256, 4, 9, 2)


#          builder   class name                  destroy                 last path                poison                                 has _bound
OWNERS = [(_diffnet, 'DiffNet', 'bsg_diffnet_destroy', 'bsg_diffnet_last_path', None, True),
          (_fs2, 'FastSpeech2MIDI', 'bsg_fs2midi_destroy', 'bsg_fs2midi_last_path', 'bsg_fs2midi_debug_poison_workspace', False),
          (_hifigan, 'HifiGanGenerator', 'bsg_hifigan_destroy', 'bsg_hifigan_last_path', 'bsg_hifigan_debug_poison_workspace', False),
          (_pe, 'PitchExtractor', 'bsg_pitchext_destroy', None, 'bsg_pitchext_debug_poison_workspace', False),
          (_pwg, 'ParallelWaveGANGenerator', 'bsg_pwg_destroy', 'bsg_pwg_last_path', 'bsg_pwg_debug_poison_workspace', False),
          (_fft, 'FFT', 'bsg_fftden_destroy', 'bsg_fftden_last_path', 'bsg_fftden_debug_poison_workspace', True)]
IDS = [o[1] for o in OWNERS]


class Recorder:
    """Stands in for the loaded library: every entry records (symbol, the handle values and ints it was given) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name,) + tuple(a.value if isinstance(a, c_void_p) else a for a in args if isinstance(a, (int, c_void_p))))
            return 0
        return entry


@pytest.fixture
def lib(monkeypatch):
    use_config()
    rec = Recorder()
    rec.loads = 0

    def load():
        rec.loads += 1
        return rec
    monkeypatch.setattr(_lib, 'load', load)
    return rec


@pytest.mark.parametrize('build,name,destroy,last_path,poison,bound', OWNERS, ids=IDS)
def test_cpu_parameters_are_refused_before_the_library_is_loaded(lib, build, name, destroy, last_path, poison, bound):
    m = build()
    with pytest.raises(_lib.BsgError, match=rf'^{name} .*no CPU path') as e:
        m.handle()
    assert 'contiguous float32' in str(e.value)      # one check and one wording for all six: the dtype too, PitchExtractor included
    assert lib.loads == 0 and lib.calls == [] and m._h is None and m._h_key is None


def test_pwg_in_the_weight_norm_layout_says_so_first(lib):
    g = _pwg(fold=False)
    with pytest.raises(_lib.BsgError, match=r'weight-norm layout: call remove_weight_norm\(\)'):
        g.handle()
    assert lib.loads == 0 and g._h is None


@pytest.mark.parametrize('build,name,destroy,last_path,poison,bound', OWNERS, ids=IDS)
def test_no_handle_nothing_to_ask_the_library(lib, build, name, destroy, last_path, poison, bound):
    m = build()
    assert '_h' not in m.__dict__ and '_h_key' not in m.__dict__      # class-level defaults
    m.poison_workspace()
    m.release()
    if name != 'DiffNet':      # DiffNet.last_path() creates the handle first (bench.py and the tools ask before the first call)
        assert m.last_path() == 'none'
    assert lib.loads == 0 and lib.calls == []
    assert (type(m).DESTROY, type(m).LAST_PATH, type(m).POISON) == (destroy, last_path, poison)
    for sym in (destroy, last_path, poison):
        assert sym is None or sym in _lib.declared_symbols()


@pytest.mark.parametrize('build,name,destroy,last_path,poison,bound', OWNERS, ids=IDS)
def test_release_destroys_once(lib, build, name, destroy, last_path, poison, bound):
    m = build()
    m._h, m._h_key = c_void_p(0x1234), m._key()
    if bound:
        m._bound = (torch.zeros(1), 0, 1, 1)
    m.release()
    assert lib.calls == [(destroy, 0x1234)]
    assert m._h is None and m._h_key is None and (not bound or m._bound is None)
    m.release()
    assert lib.calls == [(destroy, 0x1234)]


@pytest.mark.parametrize('build,name,destroy,last_path,poison,bound', OWNERS, ids=IDS)
def test_dropping_the_owner_destroys_its_handle(lib, build, name, destroy, last_path, poison, bound):
    m = build()
    m._h = c_void_p(0x77)
    del m
    gc.collect()
    assert lib.calls == [(destroy, 0x77)]


def test_del_swallows_what_release_raises(monkeypatch):
    use_config()

    def load():
        raise _lib.BsgError('no library')
    monkeypatch.setattr(_lib, 'load', load)
    m = _pe()
    m._h = c_void_p(0x77)
    with pytest.raises(_lib.BsgError):
        m.release()
    m.__del__()
    m._h = None


def test_forget_slots_finds_the_renamed_parameters(lib):
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    g = ParallelWaveGANGenerator(**pwg_ref.params(False))
    before = g._key()
    assert '_handle_slots' in g.__dict__
    g.remove_weight_norm()
    assert '_handle_slots' not in g.__dict__
    assert len(g._key()) < len(before)      # weight_g / weight_v -> weight


# ---------------------------------------------------------------------------------------------------- the length normaliser
def test_row_lengths_takes_lists_and_tensors():
    assert _lib.row_lengths([3, 1, 5], 3, 'who', T=5) == [3, 1, 5]
    got = _lib.row_lengths(torch.tensor([3, 1, 5]), 3, 'who', T=5)
    assert got == [3, 1, 5] and all(type(v) is int for v in got)
    assert _lib.row_lengths(torch.tensor([4], dtype=torch.int32), 1, 'who') == [4]
    assert _lib.row_lengths((2.0, 1), 2, 'who') == [2, 1]


def test_row_lengths_refuses_a_wrong_count():
    for lens in ([5, 4], torch.tensor([5, 4]), [5, 4, 3, 2]):
        with pytest.raises(_lib.BsgError) as e:
            _lib.row_lengths(lens, 3, 'X.forward', T=5)
        assert str(e.value) == f'X.forward: lengths has {len(lens)} entries for a batch of 3 rows'


def test_row_lengths_checks_the_values_only_with_T():
    with pytest.raises(_lib.BsgError) as e:
        _lib.row_lengths([5, 0, 3], 3, 'X.forward', T=5)
    assert str(e.value) == 'X.forward: lengths[1]=0 outside 1..T=5'
    with pytest.raises(_lib.BsgError) as e:
        _lib.row_lengths(torch.tensor([5, 4, 6]), 3, 'X.forward', T=5)
    assert str(e.value) == 'X.forward: lengths[2]=6 outside 1..T=5'
    # without T the values are the library's to check
    assert _lib.row_lengths([5, 0, 6], 3, 'X.forward') == [5, 0, 6]
    with pytest.raises(_lib.BsgError, match='lengths has 2 entries'):      # the count comes first
        _lib.row_lengths([0, 9], 3, 'X.forward', T=5)
