"""GPU: the one weight check of _lib.HandleOwner.handle() where the CPU cannot reach it (tests/test_handle_owner_cpu.py): parameters that
ARE on the device."""
import pytest
import torch

from bisinger_amd import _lib
from tests import pe_cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def test_pitch_extractor_dtype_check_passes_the_integer_buffers_and_refuses_float64(sd_spec):
    """PitchExtractor's state_dict holds BatchNorm's int64 num_batches_tracked, which the library skips: the handle is built with them in
    place.  Floating weights of another width are refused before anything is created, and the float32 module works again."""
    pe = pe_cases.pitch_extractor(sd_spec).cuda()
    assert any(not w.is_floating_point() for w in pe._weights())
    mel = torch.from_numpy(pe_cases.mel_for(1, 5)).cuda()
    want = pe(mel)['f0_denorm_pred'].clone()
    assert pe._h is not None
    pe.double()
    with pytest.raises(_lib.BsgError, match='PitchExtractor parameters must be contiguous float32 on the GPU'):
        pe.handle()
    assert pe._h is None and pe._h_key is None
    pe.float()
    assert torch.equal(pe(mel)['f0_denorm_pred'], want)
