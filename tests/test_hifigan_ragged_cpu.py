"""CPU: what a ragged HiFi-GAN forward refuses before anything runs on the GPU (HifiGanGenerator.forward(lengths=),
bsg_hifigan_forward_ragged, forward_batch(ragged_vocoder=True)); the GPU side is tests/test_gpu_hifigan_ragged.py."""
import ctypes

import pytest
import torch
import yaml

from bisinger_amd import _lib
from bisinger_amd.hifigan import HifiGanGenerator
from tests.util import ROOT


@pytest.fixture(scope='module')
def gen():
    return HifiGanGenerator(yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml')))


@pytest.mark.parametrize('lens,msg', [
    ([5, 0], r'lengths\[1\]=0 outside 1\.\.T=5'),
    ([6, 5], r'lengths\[0\]=6 outside 1\.\.T=5'),
    (torch.tensor([5, 5, 5]), 'lengths has 3 entries for a batch of 2 rows'),
    ([5], 'lengths has 1 entries for a batch of 2 rows'),
])
def test_forward_refuses_bad_lengths_before_the_handle(gen, lens, msg):
    """The lengths are checked before the handle is built and before the output exists: on a machine without a GPU the refusal is the
    length's, not 'parameters must be on the GPU'."""
    with pytest.raises(_lib.BsgError, match=msg):
        gen(torch.zeros(2, 80, 5), lengths=lens)
    assert gen._h is None


def test_c_entry_points_refuse_null_arguments():
    lib = _lib.load()
    arr = (ctypes.c_int32 * 2)(1, 1)
    assert lib.bsg_hifigan_forward_ragged(None, None, None, None, 2, 5, None) == -22
    assert 'lengths_host is null' in lib.bsg_last_error().decode()
    assert lib.bsg_hifigan_forward_ragged(None, None, arr, None, 2, 5, None) == -22
    assert lib.bsg_hifigan_forward_nsf_ragged(None, None, None, None, None, None, None, 2, 5, None) == -22
    assert 'lengths_host is null' in lib.bsg_last_error().decode()
    assert lib.bsg_hifigan_debug_poison_workspace(None, None) == -22
    assert 'null handle' in lib.bsg_last_error().decode()


def test_forward_batch_refuses_ragged_vocoder_on_pwg(monkeypatch):
    """ragged_vocoder=True with a vocoder that is not the HiFi-GAN generator: NotImplementedError naming it, before any model runs."""
    from bisinger_amd import infer as inf
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    obj = object.__new__(inf.DiffSingerE2EInfer)
    obj.vocoder = object.__new__(ParallelWaveGANGenerator)
    monkeypatch.setitem(inf.hparams, 'vocoder', 'pwg')
    monkeypatch.setattr(obj, 'estimate_frames', lambda it: 1, raising=False)
    with pytest.raises(NotImplementedError, match=r"vocoder 'pwg' \(ParallelWaveGANGenerator\) has no ragged forward"):
        obj.forward_batch([{}], ragged_vocoder=True)
    obj.vocoder = object.__new__(HifiGanGenerator)      # hparams still name pwg: refused as well
    with pytest.raises(NotImplementedError, match='pwg'):
        obj._generate_wavs([{}], None, ragged_vocoder=True)
