"""CPU: the cases of tests/test_gpu_pe_ragged.py (tests/pe_ragged_cases.py) are decided by the float64 oracle alone, row by row.

The GPU test hands every row's slice to _check_pitch (tests/test_gpu_f2_fullsize.py) against the oracle on THAT ROW ALONE
(mel[b:b+1, :n_b]).  _check_pitch sets aside frames whose voicing logit is within 10 bars of 0 and wants more than 90 % of the frames
clear and a voiced one among them; a row of <= 5 frames has no frame to spare, so there every frame must be clear — by 100 bars, since the
bar holds the fp32 oracle's deviation, which may differ a little between hosts.

It also pins what the GPU test is worth: on rows 1-3 the oracle on the PADDED batch (GroupNorm over the padding, positions counting
through it, convolutions reading it) is more than 1000 bars away from the oracle on the row alone, so an extractor that still runs the
padded batch cannot pass."""
import numpy as np
import pytest
import torch

from oracle import pe as ope
from tests import pe_cases, pe_ragged_cases as rc


@pytest.fixture(scope='module')
def sd(sd_spec):
    return pe_cases.cpu_state_dict(pe_cases.pitch_extractor(sd_spec))


@pytest.mark.parametrize('T,lens', rc.CASES, ids=rc.IDS)
def test_oracle_on_the_row_alone_decides_every_row(T, lens, sd):
    m = rc.mel(T, lens)
    padded = ope.pitch_extractor_forward(sd, torch.from_numpy(m), dtype=torch.float64)['pitch_pred'].numpy()
    for b, n in enumerate(lens):
        row = m[b:b + 1, :n].copy()
        bar, logit, f0 = pe_cases.oracle_margin(sd, row)
        clear = logit > 10 * bar
        print(f'T={T} row {b} n={n}: bar {bar:.2e} clear {clear.mean():.3f} voiced {int((f0[clear] > 0).sum())} min |logit| / bar {float(logit.min()) / bar:.0f}')
        assert 1 - clear.mean() < 0.10, (b, n, float(clear.mean()))
        assert (f0[clear] > 0).any(), (b, n)
        if n <= 5:
            assert (logit > 100 * bar).all(), (b, n, float(logit.min()), bar)
        alone = ope.pitch_extractor_forward(sd, torch.from_numpy(row), dtype=torch.float64)['pitch_pred'].numpy()[0]
        gap = float(np.abs(padded[b, :n] - alone).max())
        if b == 0:
            assert gap < 1e-12, gap          # the full-length row has no padding
        else:
            assert gap > 1000 * bar, (b, n, gap, bar)
