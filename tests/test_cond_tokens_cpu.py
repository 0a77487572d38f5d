"""CPU: the host-side argument checks of the token binding (include/bisinger_hip.h, ABI v17) need no device."""
from bisinger_amd import _lib

BSG_EINVAL = -22


def test_prepare_tokens_refuses_null_arguments_without_a_device():
    lib = _lib.load()
    assert lib.bsg_abi_version() >= 17
    assert lib.bsg_diffnet_prepare_tokens(None, None, None, 1, 2, 3, None) == BSG_EINVAL
    assert b'null' in lib.bsg_last_error()
    assert lib.bsg_fs2midi_token_rows(None, None, None, None, 1, 2, None, None) == BSG_EINVAL
    assert lib.bsg_diffnet_debug_cond_quads(None, None, 1, 1, None) == BSG_EINVAL
