"""CPU: the short pitch-extractor cases of tests/test_gpu_pe_shapes.py are decided by the float64 oracle alone.  _check_pitch
(tests/test_gpu_f2_fullsize.py) sets aside frames whose voicing logit is within 10 bars of 0 and wants more than 90 % of the frames
clear; at T <= 5 a single frame is more than 10 % of a case, so the inputs of those cases (tests/pe_cases.py SEEDS) are chosen such that
EVERY frame is clear, and some frame voiced, in the oracle."""
import pytest

from tests import pe_cases


@pytest.fixture(scope='module')
def sd(sd_spec):
    return pe_cases.cpu_state_dict(pe_cases.pitch_extractor(sd_spec))


@pytest.mark.parametrize('B', pe_cases.SHAPE_B)
@pytest.mark.parametrize('T', pe_cases.SHAPE_T)
def test_oracle_alone_decides_the_frames(B, T, sd):
    bar, logit, f0 = pe_cases.oracle_margin(sd, pe_cases.mel_for(B, T))
    clear = logit > 10 * bar
    assert (f0[clear] > 0).any()
    if T <= 5:
        # 100 bars, not 10: the bar holds the fp32 oracle's deviation, which may differ a little between hosts
        assert (logit > 100 * bar).all(), (float(logit.min()), bar)
    else:
        assert clear.mean() > 0.95, float(clear.mean())
