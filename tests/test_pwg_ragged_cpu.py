"""CPU: the ragged Parallel WaveGAN surface without a GPU — the length refusals of ``ParallelWaveGANGenerator.forward_ragged`` (which come
before the handle is built) and of bsg_pwg_forward_ragged (which come before the handle is looked at), the new symbols against the
header, and, on the float64 restatement (tests/pwg_ref.py), WHY the entry exists: a short row inside a padded rectangle is not the row
alone.  The kernels: tests/test_gpu_pwg_ragged.py."""
import functools
import os
import re
from ctypes import c_int32

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import pwg_ref as ref
from tests.test_gpu_pwg import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
torch.set_grad_enabled(False)


def test_forward_ragged_refuses_bad_lengths_before_the_handle_is_built():
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    gen = ParallelWaveGANGenerator(**ref.params(False))
    mel = torch.zeros(3, 80, 5)
    with pytest.raises(_lib.BsgError, match=r'lengths has 2 entries for a batch of 3 rows'):
        gen.forward_ragged(None, mel, lengths=[5, 4], seed=1)
    assert gen._h is None
    for bad, row in (([5, 0, 3], 1), ([5, 4, 6], 2), (torch.tensor([-1, 4, 5]), 0)):
        with pytest.raises(_lib.BsgError, match=rf'lengths\[{row}\]=-?\d+ outside 1\.\.T=5'):
            gen.forward_ragged(None, mel, lengths=bad, seed=1)
        assert gen._h is None
    assert gen.last_tiles() == 0 and gen.last_path() == 'none'


def test_c_entry_looks_at_the_lengths_before_the_handle():
    lib = _lib.load()
    assert lib.bsg_pwg_forward_ragged(None, None, None, None, None, None, 2, 5, 0, None) == EINVAL
    assert 'lengths_host is null' in lib.bsg_last_error().decode()
    assert lib.bsg_pwg_forward_ragged(None, None, None, None, (c_int32 * 3)(5, 2, 6), None, 3, 5, 0, None) == EINVAL
    assert 'lengths[2]=6 outside 1..T=5' in lib.bsg_last_error().decode()
    assert lib.bsg_pwg_forward_ragged(None, None, None, None, (c_int32 * 3)(5, 0, 6), None, 3, 5, 0, None) == EINVAL
    assert 'lengths[1]=0 outside 1..T=5' in lib.bsg_last_error().decode()
    # good lengths: the padded call's own refusal, under the ragged entry's name
    assert lib.bsg_pwg_forward_ragged(None, None, None, None, (c_int32 * 3)(5, 2, 1), None, 3, 5, 0, None) == EINVAL
    msg = lib.bsg_last_error().decode()
    assert 'pwg_forward_ragged' in msg and 'null' in msg


def test_last_tiles_of_a_null_handle():
    assert _lib.load().bsg_pwg_last_tiles(None) == 0


def test_new_entries_match_the_header():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bisinger_hip.h')).read(), flags=re.S)
    for name in ('bsg_pwg_forward_ragged', 'bsg_pwg_last_tiles'):
        args = re.search(rf'\bint {name}\s*\((.*?)\);', src, flags=re.S).group(1).split(',')
        restype, argtypes = _lib._SIGS[name]
        assert restype is _lib.c_int32
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        for a, ty in zip(args, argtypes):
            assert ('*' in a) == (ty is _lib.c_void_p), (name, a.strip())
        assert name in _lib.declared_symbols()
        assert hasattr(_lib.load(), name)


@functools.lru_cache(maxsize=None)
def padded_against_alone(form):
    """One row of n = 23 frames inside T = 40: zeros behind it for the mel, coarse pitch 1, noise over the whole rectangle, the rectangle
    edge-padded as a caller of ``forward`` builds it; against the row alone.  -> (|difference| per frame of the row, peak of the row alone)"""
    n, T, w = 23, 40, 2
    pitch = form == 'pitch'
    z, c, p = ref.make_inputs(1, T, 77, w, pitch)
    mel = c[:, :, w:w + T].copy()
    mel[:, :, n:] = 0.0
    if pitch:
        p = p[:, w:w + T].copy()
        p[:, n:] = 1
    sd, q = weights(form)[1], ref.params(pitch)
    pad = lambda a, k: None if a is None else np.pad(a, ((0, 0),) * (a.ndim - 1) + ((w, w),), 'edge')
    inside = ref.forward(sd, z, pad(mel, w), pad(p, w), q, torch.float64)[0, 0, :n * ref.HOP]
    alone = ref.forward(sd, z[:, :, :n * ref.HOP], pad(mel[:, :, :n], w), None if p is None else pad(p[:, :n], w), q, torch.float64)[0, 0]
    return np.abs(inside - alone).reshape(n, ref.HOP).max(axis=1), float(np.abs(alone).max())


@pytest.mark.parametrize('form', ['plain', 'pitch'])
def test_a_short_row_inside_a_padded_rectangle_is_not_the_row_alone(form):
    """In float64, so no rounding is in play: the zero mel frames behind the row reach it through conv_in and the up-sampling
    convolutions, and the dilated convolutions (about 12 frames to each side) read the noise-driven x of the padding.  The last 10
    frames differ by far more than the 1e-3 asserted here; the first frames, out of the padding's reach, agree to float64 rounding
    (1e-12: the convolution library may block a longer row differently)."""
    per_frame, peak = padded_against_alone(form)
    print(f'{form}: last 10 frames differ by up to {per_frame[-10:].max():.3e} on a peak of {peak:.3f}; per frame: '
          + ' '.join(f'{v:.1e}' for v in per_frame))
    assert per_frame[-10:].max() > 1e-3
    assert per_frame[:5].max() <= 1e-12
