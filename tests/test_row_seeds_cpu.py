"""CPU: what row-keyed sampler noise (ABI v22: bsg_philox_normal_rows, bsg_ddpm_sample_rows; row_seeds= / seeds=) refuses, without a GPU —
the null and range refusals of both entries through the loaded library (status and message, nothing enqueued: no device is touched before
them), the ValueErrors of the exclusive arguments (raised before any handle exists), and the header and the binding agreeing on v22."""
import os
import re
from ctypes import c_int32, c_uint64, c_void_p

import pytest
import torch

from bisinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
X = c_void_p(0x1000)      # a non-null "device pointer": every refusal below comes before anything reads or launches on it


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsg_last_error().decode()


def seeds(*v):
    return (c_uint64 * len(v))(*v)


def lens(*v):
    return (c_int32 * len(v))(*v)


def test_header_and_binding_agree_on_v22(lib):
    src = open(os.path.join(ROOT, 'include', 'bisinger_hip.h')).read()
    assert _lib.ABI_VERSION == 22 and re.search(r'#define BSG_ABI_VERSION 22\b', src)
    assert lib.bsg_abi_version() == 22
    for name in ('bsg_philox_normal_rows', 'bsg_ddpm_sample_rows'):
        assert name in _lib.declared_symbols() and re.search(rf'\bint {name}\(', src)


def test_philox_normal_rows_refusals(lib):
    assert lib.bsg_philox_normal_rows(None, 2, 80, 8, None, seeds(1, 2), 7, None) == EINVAL and 'null x' in err(lib)
    assert lib.bsg_philox_normal_rows(X, 2, 80, 8, None, None, 7, None) == EINVAL and 'null seeds_host' in err(lib)
    for B in (0, -3):
        assert lib.bsg_philox_normal_rows(X, B, 80, 8, None, seeds(1), 7, None) == EINVAL and f'B={B}' in err(lib)
    # n_b outside 1..T: the message names the row
    for bad, row in ((lens(8, 0, 4), 1), (lens(8, 8, 9), 2), (lens(-1, 8, 8), 0)):
        assert lib.bsg_philox_normal_rows(X, 3, 80, 8, bad, seeds(1, 2, 3), 7, None) == EINVAL
        assert f'lengths[{row}]={bad[row]} outside 1..T=8' in err(lib)
    # M n_b no multiple of 4 (bsg_philox_normal refuses that n too): the flat layout at n = 6, and T itself without lengths
    assert lib.bsg_philox_normal_rows(X, 2, 1, 8, lens(8, 6), seeds(1, 2), 7, None) == EINVAL
    assert 'row 1' in err(lib) and 'multiple of 4' in err(lib)
    assert lib.bsg_philox_normal_rows(X, 2, 3, 7, None, seeds(1, 2), 7, None) == EINVAL
    assert 'row 0' in err(lib) and 'multiple of 4' in err(lib)
    assert lib.bsg_philox_normal(X, 6, 1, 7, 0, None) == EINVAL      # the lone call's refusal of the same n


def test_ddpm_sample_rows_refusals(lib):
    s = _lib.Schedule()
    assert lib.bsg_ddpm_sample_rows(X, s, X, None, 3, 3, 2, 8, None) == EINVAL and 'null seeds_host' in err(lib)
    assert lib.bsg_ddpm_sample_rows(None, s, X, seeds(1, 2), 3, 3, 2, 8, None) == EINVAL and 'ddpm_sample_rows: null handle' in err(lib)


def test_exclusive_arguments_raise_before_any_handle():
    from bisinger_amd.diffusion import GaussianDiffusion
    from bisinger_amd.hifigan import HifiGanGenerator
    from bisinger_amd.infer import DiffSingerE2EInfer
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    from bisinger_amd.vocoders import PWG
    # (no instance is built: the checks come first in each method and read only their arguments)
    x = torch.zeros(2, 1, 80, 8)
    with pytest.raises(ValueError, match='row_seeds.*noise'):
        GaussianDiffusion.sample(None, None, x, noise=torch.zeros(3, 2, 80, 8), row_seeds=[1, 2])
    with pytest.raises(ValueError, match='3 entries for a batch of 2'):
        GaussianDiffusion.sample(None, None, x, row_seeds=[1, 2, 3])
    tok = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match='row_seeds.*noise'):
        GaussianDiffusion.forward(None, tok, infer=True, noise=torch.zeros(5, 2, 80, 8), row_seeds=[1, 2])
    mel = torch.zeros(2, 80, 8)
    for kw, name in (({'rand_ini': torch.zeros(2, 9)}, 'rand_ini'), ({'noise': torch.zeros(2, 8 * 256, 9)}, 'noise')):
        with pytest.raises(ValueError, match=f'row_seeds.*{name}'):
            HifiGanGenerator.forward(None, mel, torch.zeros(2, 8), row_seeds=[1, 2], **kw)
    with pytest.raises(ValueError, match='row_seeds.* x'):
        ParallelWaveGANGenerator.forward_ragged(None, torch.zeros(2, 1, 8 * 256), mel, lengths=[8, 4], row_seeds=[1, 2])
    with pytest.raises(ValueError, match='zs'):
        PWG.spec2wav_batch(None, [mel[0].T, mel[1].T], zs=[torch.zeros(8 * 256)] * 2, seeds=[1, 2])
    with pytest.raises(ValueError, match='1 entries for a batch of 2'):
        DiffSingerE2EInfer.forward_batch(None, [{}, {}], seeds=[1])
