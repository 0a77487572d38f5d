"""GPU: the pitch extractor (csrc/pe_nsf.hip, the heaviest user of the generic GEMM) at its shape edges against
oracle.pe.pitch_extractor_forward in float64, on both pipes of its GEMMs: the default split-fp16 one and the fp32 matrix pipe
(set_gemm_split(False)).  Weights, fixture and bars are those of tests/test_gpu_f2_fullsize.py (_check_pitch: pitch_pred within 2 x the
fp32 oracle's deviation + 2e-5 of its scale, voicing and f0 wherever the float64 logit is clear of 0, f0 == 0 past each row).

T = 1 .. 5: the five taps are wider than the row; 63 / 64 / 65 and 127 / 128 / 129: positions_kernel's 64-frame chunks and carry, the
GEMM tiles; B x T % 4 != 0: the kernels with four rows per workgroup; T < 64: groupnorm_res_kernel with fewer elements (4 T) than
threads."""
import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import pe_cases
from tests.test_gpu_f2_fullsize import _check_pitch, pitch_ext  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PIPES = ['split', 'fp32']


@pytest.fixture(params=PIPES)
def pe_on(request, pitch_ext):  # noqa: F811
    """(PitchExtractor on the requested pipe, its CPU state dict); the default pipe is restored afterwards."""
    pe, sd = pitch_ext
    pe.set_gemm_split(request.param == 'split')
    assert pe.gemm_split_enabled() == (request.param == 'split')
    yield pe, sd
    pe.set_gemm_split(True)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ('pitch_pred', 'f0_denorm_pred'))


@pytest.mark.parametrize('B', pe_cases.SHAPE_B)
@pytest.mark.parametrize('T', pe_cases.SHAPE_T)
def test_pitch_extractor_shapes_vs_fp64(B, T, pe_on, request):
    pe, sd = pe_on
    mel = pe_cases.mel_for(B, T)
    if T <= 5:
        bar, logit, _ = pe_cases.oracle_margin(sd, mel)
        assert (logit > 10 * bar).all(), 'the float64 oracle alone must decide every frame of a case this short'
    retries = _lib.range_retries
    r = pe(torch.from_numpy(mel).cuda())
    assert r['pitch_pred'].shape == (B, T, 2) and r['f0_denorm_pred'].shape == (B, T)
    _check_pitch(f'pitch_extractor {request.node.callspec.id}', r, sd, mel, [T] * B)
    assert _lib.range_retries == retries, 'in-range input raised a range event of the split-fp16 GEMMs'


@pytest.mark.parametrize('T', [70, 129])
def test_rows_that_end_in_exact_zeros(T, pe_on):
    """Rows whose mel is exactly 0 from frame n on, n = 0 (the whole row), 1 and 64: f0 == 0 there, and the rest matches the oracle on
    the padded batch (GroupNorm's statistics run over the padding too)."""
    pe, sd = pe_on
    lens = [T, 64, 1, 0]
    mel = pe_cases.mel(np.random.RandomState(900 + T), 4, T, lens)
    r = pe(torch.from_numpy(mel).cuda())
    f0 = _check_pitch(f'pitch_extractor zero tails T={T}', r, sd, mel, lens)
    assert (f0[0] > 0).any() and (f0[3] == 0).all()


def test_short_call_after_a_long_one_is_bitwise_a_fresh_handle(pe_on, sd_spec):
    """The handle keeps its workspace between calls: B = 1, T = 3 after B = 3, T = 257 must not see anything the long call left."""
    pe, _ = pe_on
    fresh = pe_cases.pitch_extractor(sd_spec).cuda()
    fresh.set_gemm_split(pe.gemm_split_enabled())
    long_mel, short_mel = pe_cases.mel_for(3, 257), pe_cases.mel_for(1, 3)
    pe(torch.from_numpy(long_mel).cuda())
    got = pe(torch.from_numpy(short_mel).cuda())
    want = fresh(torch.from_numpy(short_mel).cuda())
    assert torch.isfinite(got['pitch_pred']).all()
    assert _same(got, want)


@pytest.mark.parametrize('T', [2, 5, 65, 129])
def test_batch_rows_equal_each_row_alone_bitwise(T, pe_on):
    """Every stage is per row (GroupNorm's statistics are per row and group, the convolutions pad per row), so a row of a batch of 3
    equals the same row alone, bit for bit; B x T = 6, 15, 195, 387 rows put the rows at different places of the GEMM tiles."""
    pe, _ = pe_on
    mel = torch.from_numpy(pe_cases.mel_for(3, T)).cuda()
    batch = pe(mel)
    for b in range(3):
        alone = pe(mel[b:b + 1].contiguous())
        assert _same({k: v[b:b + 1] for k, v in batch.items()}, alone), f'row {b}'
