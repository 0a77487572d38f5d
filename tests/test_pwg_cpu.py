"""CPU: the Parallel WaveGAN surface (`vocoder: pwg`) without a GPU — the restatement against the reference's goldens, the state-dict
layout of the drop-in against the recorded spec, the registry, and the refusals of bsg_pwg_create (which come before any device call).
The kernels themselves: tests/test_gpu_pwg.py."""
import json
import os
from collections import OrderedDict
from ctypes import POINTER, byref, c_void_p, cast

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests import pwg_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEEDS, CASES = ref.GOLDEN_SEEDS, ref.GOLDEN_CASES
EINVAL = -22
torch.set_grad_enabled(False)


@pytest.fixture(scope='module')
def spec():
    return json.load(open(os.path.join(GOLD, 'pwg_state_dict_spec.json')))


def formula_weights(spec, form):
    s = OrderedDict((k, tuple(shp)) for k, shp in spec[f'{form}_weight_norm'])
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(s, SEEDS[form]).items()}


@pytest.mark.parametrize('form', ['plain', 'pitch'])
def test_restatement_matches_the_reference_goldens(spec, form):
    """float32 mode against the reference's own output: <= 1e-6 (measured 7.153e-07 plain, 1.490e-07 pitch); float64 mode agrees with the
    reference to fp32 rounding."""
    gold = np.load(os.path.join(GOLD, f'pwg_{form}.npz'))
    sd = ref.fold(formula_weights(spec, form))
    assert [[k, list(v.shape)] for k, v in sd.items()] == spec[f'{form}_folded']
    p = ref.params(form == 'pitch')
    for tag, (B, T, seed) in CASES.items():
        z, c, pitch = ref.make_inputs(B, T, seed, 2, form == 'pitch')
        y32 = ref.forward(sd, z, c, pitch, p, torch.float32)
        assert y32.shape == gold[tag].shape == (B, 1, T * 256)
        e32 = float(np.abs(y32 - gold[tag]).max())
        e64 = float(np.abs(ref.forward(sd, z, c, pitch, p, torch.float64) - gold[tag]).max())
        print(f'{form} {tag}: float32 restatement vs reference {e32:.3e}, float64 restatement vs reference {e64:.3e}')
        assert e32 <= 1e-6
        assert e64 <= 4e-6


def test_recorded_spec_is_the_reference_generator(spec):
    assert len(spec['plain_weight_norm']) == 349 and len(spec['plain_folded']) == 221
    assert spec['plain_n_params'] == 1334309 and spec['receptive_field_size'] == 6139 and spec['hop_size'] == 256


@pytest.mark.parametrize('form', ['plain', 'pitch'])
def test_state_dict_keys_shapes_and_order_in_both_layouts(spec, form):
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    gp = json.loads(json.dumps(spec['generator_params']))
    gp['use_pitch_embed'] = form == 'pitch'
    g = ParallelWaveGANGenerator(**gp)
    assert [[k, list(v.shape)] for k, v in g.state_dict().items()] == spec[f'{form}_weight_norm']
    assert g.receptive_field_size == spec['receptive_field_size'] and g.hop_size == spec['hop_size']
    w = formula_weights(spec, form)
    g.load_state_dict(w, strict=True)
    g.remove_weight_norm()
    assert [[k, list(v.shape)] for k, v in g.state_dict().items()] == spec[f'{form}_folded']
    want = ref.fold(w)
    for k, v in g.state_dict().items():
        assert torch.equal(v, want[k]), k
    # an already folded state dict loads into a fresh (weight-norm) module, strictly; and the weight-norm layout loads into a folded one
    g2 = ParallelWaveGANGenerator(**gp)
    g2.load_state_dict(want, strict=True)
    assert list(g2.state_dict()) == [k for k, _ in spec[f'{form}_folded']]
    g2.load_state_dict(w, strict=True)
    assert list(g2.state_dict()) == [k for k, _ in spec[f'{form}_weight_norm']]
    with pytest.raises(RuntimeError):
        g2.load_state_dict({k: v for k, v in w.items() if k != 'first_conv.bias'}, strict=True)
    gp['use_weight_norm'] = False
    assert [[k, list(v.shape)] for k, v in ParallelWaveGANGenerator(**gp).state_dict().items()] == spec[f'{form}_folded']


def test_registry_resolves_pwg():
    from bisinger_amd import vocoders
    assert vocoders.get_vocoder_cls({'vocoder': 'pwg'}) is vocoders.PWG
    assert vocoders.get_vocoder_cls({'vocoder': 'vocoders.pwg.PWG'}) is vocoders.PWG
    assert issubclass(vocoders.PWG, vocoders.BaseVocoder)
    assert vocoders.get_vocoder_cls({'vocoder': 'vocoders.hifigan.HifiGAN'}) is vocoders.HifiGAN
    with pytest.raises(NotImplementedError):
        vocoders.PWG.wav2spec('x.wav')
    with pytest.raises(NotImplementedError):
        vocoders.PWG.wav2mfcc('x.wav')


def test_f0_to_coarse_bins():
    from bisinger_amd.vocoders import f0_to_coarse
    got = f0_to_coarse(np.array([0.0, 10.0, 50.0, 440.0, 1100.0, 5000.0], np.float32))
    assert got.dtype == np.int64 and got.tolist()[:3] == [1, 1, 1] and got[4] == 255 and got[5] == 255 and 1 < got[3] < 255
    mel = lambda f: 1127 * np.log(1 + f / 700)
    assert got[3] == int(np.rint((mel(440.0) - mel(50.0)) * 254 / (mel(1100.0) - mel(50.0)) + 1))


base_cfg = ref.base_cfg


def try_create(cfg, n=None):
    lib = _lib.load()
    n = lib.bsg_pwg_n_weights(byref(cfg)) if n is None else n
    dummy = (c_void_p * 400)(*([1] * 400))            # never dereferenced: every refusal below comes before the first device call
    h = c_void_p()
    rc = lib.bsg_pwg_create(byref(h), byref(cfg), cast(dummy, POINTER(c_void_p)), n, c_void_p(1))
    return rc, h.value, lib.bsg_last_error().decode()


def test_n_weights_is_the_folded_state_dict_length(spec):
    cfg = base_cfg()
    assert _lib.load().bsg_pwg_n_weights(byref(cfg)) == len(spec['plain_folded']) == 221
    cfg.use_pitch_embed, cfg.n_pitch = 1, 300
    assert _lib.load().bsg_pwg_n_weights(byref(cfg)) == len(spec['pitch_folded']) == 224


@pytest.mark.parametrize('field,value,words', [
    ('gate_channels', 64, ('gate_channels=64', '128')),
    ('kernel_size', 5, ('kernel_size=5', '3')),
    ('use_causal_conv', 1, ('use_causal_conv=1', 'causal')),
    ('hop_size', 300, ('256', 'hop_size=300')),
    ('residual_channels', 128, ('residual_channels=128', '64')),
    ('aux_channels', 100, ('aux_channels=100', '80')),
    ('stacks', 4, ('layers=30', 'stacks=4')),
    ('upsample_net', 1, ('upsample_net', 'ConvInUpsampleNetwork')),
])
def test_create_refuses_with_a_message_naming_the_value(field, value, words):
    cfg = base_cfg()
    setattr(cfg, field, value)
    rc, h, msg = try_create(cfg)
    assert rc == EINVAL and h is None
    for w in words:
        assert w in msg, msg


def test_create_refuses_a_scale_product_other_than_hop_and_a_wrong_weight_count():
    cfg = base_cfg()
    cfg.upsample_scales[3] = 8                        # 4 * 4 * 4 * 8 = 512 != 256
    rc, h, msg = try_create(cfg)
    assert rc == EINVAL and h is None and '512' in msg and 'hop_size=256' in msg, msg
    rc, h, msg = try_create(base_cfg(), n=220)
    assert rc == EINVAL and h is None and '220' in msg and '221' in msg, msg


def test_last_path_of_a_null_handle():
    assert _lib.load().bsg_pwg_last_path(None) == b'none'


def test_forward_refuses_bad_shapes_before_looking_at_the_handle():
    lib = _lib.load()
    assert lib.bsg_pwg_forward(None, None, None, None, None, 0, 5, 0, None) == EINVAL
    assert 'B=0' in lib.bsg_last_error().decode()
    assert lib.bsg_pwg_forward(None, None, None, None, None, 1, 5, 0, None) == EINVAL
    assert 'null' in lib.bsg_last_error().decode()
