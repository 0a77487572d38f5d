"""CPU: ragged batches through the FFT denoiser (bsg_fftden_prepare_ragged, bsg_fftden_ddpm_sample, bsg_fftden_plms_sample) without a GPU —
the bounds of tests/fftden_ragged_cases.py against the float32 restatement of the oracle, the separation of the padded from the row-alone
result that makes those bounds meaningful, the exported symbols with ABI v22 unchanged, and the argument refusals through the loaded
library (status and message; no device is touched before them).

A handle cannot exist without a device, so the refusal of a forward whose (B, T) differ from the binding is checked where a handle exists
(tests/test_gpu_fftden_ragged.py::test_forward_refuses_another_shape_than_the_binding); here the null handle's refusal stands for it.
"""
import os
import re
from ctypes import c_int32, c_uint64, c_void_p

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import fftden_ragged_cases as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
X = c_void_p(0x1000)      # a non-null "device pointer": every refusal below comes before anything reads or launches on it
NEW = ('bsg_fftden_prepare_ragged', 'bsg_fftden_ddpm_sample', 'bsg_fftden_plms_sample')


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def err(lib):
    return lib.bsg_last_error().decode()


def lens(*v):
    return (c_int32 * len(v))(*v)


def test_bounds_cover_the_float32_restatement():
    """Every compared quantity, float32 oracle against float64 oracle over every case: within bound / 4 (= MEASURED_F32)."""
    sd = RC.oracle_sd()
    worst = {'eps': 0.0, 'ddpm': 0.0, 'plms': 0.0}
    for i, case in enumerate(RC.FWD_CASES):
        for b, n in enumerate(case[0]):
            worst['eps'] = max(worst['eps'], RC.figure(RC.eps_alone_case(i, b, RC.F32), RC.eps_alone_case(i, b, RC.F64)))
    for c, rows in ((RC.DDPM, list(enumerate(RC.DDPM['lens']))), (RC.DDPM_PADDED, [(b, RC.DDPM_PADDED['T']) for b in range(RC.DDPM_PADDED['B'])])):
        cond, noise = RC.ddpm_inputs(c, len(rows))
        for b, n in rows:
            a32, a64 = (RC.ddpm_alone(sd, cond, noise[0][b], noise[1:, b, :, :n], b, n, c, dt) for dt in (RC.F32, RC.F64))
            worst['ddpm'] = max(worst['ddpm'], RC.figure(a32, a64))
    sdp = RC.oracle_sd(RC.PLMS_GAIN)
    cond, xT = RC.plms_inputs()
    for b, n in enumerate(RC.PLMS['lens']):
        for nn in {n, RC.PLMS['T']}:      # the ragged binding's row, and the padded binding's
            a32, a64 = (RC.plms_alone(sdp, cond, xT, b, nn, RC.PLMS, dt) for dt in (RC.F32, RC.F64))
            assert float(np.abs(a64).max()) < 10.0      # the conditioning keeps the float64 result O(10) at the most
            worst['plms'] = max(worst['plms'], RC.figure(a32, a64))
    print({k: f'{v:.3e} (bound / 4 = {RC.MEASURED_F32[k]:.3e})' for k, v in worst.items()})
    for k, v in worst.items():
        assert 0 < v <= RC.MEASURED_F32[k], (k, v)
        assert RC.BOUND[k] == 4 * RC.MEASURED_F32[k]


def test_padded_and_alone_are_far_apart():
    """For every ragged case with a short row: the float64 PADDED result of that row is at least 1000 x the bound from its row-alone result
    (the reference's padding mask is never set: padded frames are attention keys, are counted by the positions, and the FFN convolution
    reads them)."""
    sd = RC.oracle_sd()
    seen = 0
    for i, case in enumerate(RC.FWD_CASES):
        row_lens, T = case[:2]
        if all(n == T for n in row_lens):
            continue
        x, t, cond = RC.fwd_inputs(case)
        pad = RC.eps_padded(sd, x, t, cond)
        for b, n in enumerate(row_lens):
            if n == T:
                continue
            want = RC.eps_alone_case(i, b, RC.F64)
            d = float(np.abs(pad[b, :, :n] - want).max())
            assert d >= 1000 * RC.bound('eps', want), (RC.name(case), b, n, d, RC.bound('eps', want))
            seen += 1
    assert seen >= 20


def test_padded_and_alone_loops_are_far_apart():
    """The same for the two loops: x of every short row after the padded float64 DDPM run (lengths 77 / 9 / 1) and after the padded float64
    PLMS run (40 / 9, the scaled last projection) lies at least 1000 x its bound from the row-alone result."""
    c = RC.DDPM
    sd = RC.oracle_sd()
    cond, noise = RC.ddpm_inputs(c)
    pad = RC.ddpm_padded(sd, cond, noise, c)
    for b, n in enumerate(c['lens']):
        if n < c['T']:
            want = RC.ddpm_alone(sd, cond, noise[0][b], noise[1:, b, :, :n], b, n, c, RC.F64)
            d = float(np.abs(pad[b, :, :n] - want).max())
            print(f'ddpm row {b} (n={n}): padded against alone {d:.2e}, bound {RC.bound("ddpm", want):.2e}')
            assert d >= 1000 * RC.bound('ddpm', want), (b, n, d)
    c = RC.PLMS
    sdp = RC.oracle_sd(RC.PLMS_GAIN)
    cond, xT = RC.plms_inputs()
    pad = RC.plms_padded(sdp, cond, xT, c)
    for b, n in enumerate(c['lens']):
        if n < c['T']:
            want = RC.plms_alone(sdp, cond, xT, b, n, c, RC.F64)
            d = float(np.abs(pad[b, :, :n] - want).max())
            print(f'plms row {b} (n={n}): padded against alone {d:.2e}, bound {RC.bound("plms", want):.2e}')
            assert d >= 1000 * RC.bound('plms', want), (b, n, d)


def test_cases_cover_what_they_claim():
    all_lens = {n for c in RC.FWD_CASES for n in c[0]}
    assert {1, 2, 8, 9, 10, 31, 32, 33, 63, 64, 65, 129, 130} <= all_lens
    assert {len(c[0]) for c in RC.FWD_CASES} == {1, 2, 3, 5}
    assert {c[1] for c in RC.FWD_CASES} >= {10, 11, 224, 225, 480, 481}      # both sides of every attention threshold in T at B <= 3
    assert {c[2] for c in RC.FWD_CASES} == {'split/nw2', 'planes/ks1', 'planes/ks2', 'planes/ks4'}
    # both sides of every GEMM-form threshold in T at B = 5, and every ragged form of the pre-split GEMM named by some case
    assert {c[1] for c in RC.FWD_CASES if len(c[0]) == 5} >= {384, 385, 512, 513, 1536, 1537, 1600, 1601}
    assert {tok for c in RC.FWD_CASES for tok in c[3]} == set(RC.GEMM_FORMS)
    for lens_, T, _, gemm in RC.FWD_CASES:      # the expected tokens against the dispatch rule as the module's comment states it
        B, want = len(lens_), set()
        for wn, taps in ((8, 9), (6, 1), (2, 1)):
            tiny, small = -(-T // 64) * wn * B < 256, -(-T // 128) * wn * B < 512
            want.add(('h2w/32/ring16' if taps > 1 else 'h2w/32/deep') if tiny else 'h2w/64/ring8' if small else 'h2w/128/ring4')
        assert set(gemm) == want, (lens_, T, gemm, want)
    assert any(c[0] == (c[1], 1) for c in RC.FWD_CASES) and all(n == RC.FULL_CASE[1] for n in RC.FULL_CASE[0])
    assert all(1 <= n <= c[1] for c in RC.FWD_CASES for n in c[0])


def test_symbols_exported_and_abi_still_22(lib):
    src = open(os.path.join(ROOT, 'include', 'bisinger_hip.h')).read()
    assert _lib.ABI_VERSION == 22 and re.search(r'#define BSG_ABI_VERSION 22\b', src)
    assert lib.bsg_abi_version() == 22
    for name in NEW:
        assert name in _lib.declared_symbols() and re.search(rf'\bint {name}\(', src), name
        assert getattr(lib, name) is not None


def test_prepare_ragged_refusals(lib):
    """Length 0, length > T, null lengths, bad B / T: BSG_EINVAL naming the row.  The lengths are judged before the handle is looked at (null
    here: no device call can follow)."""
    assert lib.bsg_fftden_prepare_ragged(None, X, None, 2, 8, None) == EINVAL and 'lengths_host is null' in err(lib)
    for bad, row in ((lens(8, 0), 1), (lens(9, 8), 0), (lens(8, -2), 1)):
        assert lib.bsg_fftden_prepare_ragged(None, X, bad, 2, 8, None) == EINVAL
        assert f'lengths[{row}]={bad[row]} outside 1..T=8' in err(lib) and 'fftden_prepare_ragged' in err(lib)
    assert lib.bsg_fftden_prepare_ragged(None, X, lens(1), 0, 8, None) == EINVAL and 'B=0' in err(lib)
    assert lib.bsg_fftden_prepare_ragged(None, X, lens(1), 1, 0, None) == EINVAL and 'T=0' in err(lib)
    assert lib.bsg_fftden_prepare_ragged(None, X, lens(8, 3), 2, 8, None) == EINVAL and 'null handle' in err(lib)
    assert lib.bsg_fftden_prepare_ragged(None, None, lens(8, 3), 2, 8, None) == EINVAL


def test_forward_and_sampler_refusals(lib):
    s = _lib.Schedule()
    assert lib.bsg_fftden_forward(None, X, X, X, 2, 8, None) == EINVAL and 'fftden_forward' in err(lib)
    seeds = (c_uint64 * 2)(1, 2)
    assert lib.bsg_fftden_ddpm_sample(None, s, X, None, 0, seeds, 3, 3, 2, 8, 0, 2, None) == EINVAL and 'fftden_ddpm_sample: null handle' in err(lib)
    assert lib.bsg_fftden_plms_sample(None, s, X, 100, 5, 2, 8, None) == EINVAL and 'fftden_plms_sample: null handle' in err(lib)

