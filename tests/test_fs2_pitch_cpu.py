"""CPU: the pitch adaptor and the plain FastSpeech2 front — the restatement of tests/fs2_pitch_ref.py against the reference's own outputs
(tests/golden/fs2_pitch.npz, tools/make_golden_fs2pitch.py), the drop-ins' state-dict layout, the refusals, the bin function on hand cases,
the bounds and the near-tie census that tests/test_gpu_fs2_pitch.py relies on.

Golden bound: float32 restatement <= 1e-6 x max(1, max |want|) on pitch_pred, decoder_inp and mel_out, bins and mel2ph exact (measured:
at most 2.5e-7, 3.4e-7 and 7.1e-7).
"""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from bisinger_amd import synth
from tests import fs2_pitch_ref as R
from tests.util import ROOT, cpu_sd, use_config

torch.set_grad_enabled(False)
F32, F64 = torch.float32, torch.float64
GOLD = os.path.join(ROOT, 'tests', 'golden')
GOLD_BOUND = dict.fromkeys(('pitch_pred', 'decoder_inp', 'mel_out'), 1e-6)


@pytest.fixture(autouse=True)
def goldens_inv_freq(monkeypatch):
    """The restatement with the inverse frequencies of the host that made the goldens (oracle/freq.py), as tests/test_oracle_golden.py."""
    from oracle import freq
    monkeypatch.setattr(freq, 'inv_freq', R.golden_host_inv_freq())


@pytest.fixture(scope='module')
def spec():
    with open(os.path.join(GOLD, 'fs2_pitch_spec.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'fs2_pitch.npz'))


def gold_inputs():
    inp = synth.synth_inputs(2, 12, 64, seed=1, ragged=True)
    rs = np.random.RandomState(64)
    inp['f0'] = R.bin_centre_f0(rs.randint(2, 255, size=(2, 64)))
    inp['uv'] = (rs.uniform(size=(2, 64)) < 0.2).astype(np.float32)
    return inp


def formula_sd(entries, prefix='fs2.'):
    sp = OrderedDict((prefix + k, tuple(s)) for k, s in entries)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(sp, 0, synth.DIFFNET_GAIN).items()}
    return R.make_pitch_visible(sd, prefix)


def hp_of(spec, chain):
    h = spec[chain]['hparams']
    return dict(hidden_size=256, enc_layers=h['enc_layers'], dec_layers=h['dec_layers'], num_heads=h['num_heads'],
                enc_ffn_kernel_size=h['enc_ffn_kernel_size'], dec_ffn_kernel_size=h['dec_ffn_kernel_size'],
                dur_predictor_layers=h['dur_predictor_layers'], dur_predictor_kernel=h['dur_predictor_kernel'], use_midi=bool(h['use_midi']),
                use_spk_id=bool(h['use_spk_id']), use_pitch_embed=True, use_uv=bool(h['use_uv']), predictor_layers=h['predictor_layers'],
                predictor_kernel=h['predictor_kernel'])


def nerr(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(got.double().numpy() - want).max()) / max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize('chain,run', [('popcs', 'pred'), ('popcs', 'given'), ('popcs', 'dur'), ('bisinger', 'pred'), ('bisinger', 'given')])
def test_restatement_against_the_reference(spec, gold, chain, run):
    hp = hp_of(spec, chain)
    assert (hp['predictor_layers'], hp['use_midi']) == ((2, False) if chain == 'popcs' else (5, True))
    sd = formula_sd(spec[chain]['fs2'])
    inp = {k: torch.from_numpy(v) for k, v in gold_inputs().items()}
    if run == 'dur':
        del inp['mel2ph']
    f0, uv = (inp['f0'], inp['uv']) if run == 'given' else (None, None)
    r = R.forward(sd, inp, hp, dtype=F32, f0=f0, uv=uv)
    g = lambda k: gold[f'{chain}.{run}.{k}']
    assert np.array_equal(r['mel2ph'].numpy(), g('mel2ph'))
    f0w = g('f0_denorm')
    assert np.array_equal(R.f0_to_mel_bins(torch.from_numpy(f0w))[1].numpy(), r['pitch_bin'].numpy()), 'bins'
    for k in ('pitch_pred', 'decoder_inp', 'mel_out'):
        e = nerr(r[k], g(k))
        print(f'{chain}.{run}.{k}: {e:.2e} (allowed {GOLD_BOUND[k]:.2e})')
        assert e <= GOLD_BOUND[k], k
    assert float(np.abs(r['f0_denorm'].numpy() - f0w).max() / max(1.0, f0w.max())) <= 1e-6
    assert bool(gold[f'{chain}.ref_writes_f0']), 'the reference zeroes the supplied f0 in place (INTEGRATION.md, Differences)'


def test_state_dict_layout_and_front_choice(spec):
    """Keys, shapes and order of (a) FastSpeech2 + pitch, (b) FastSpeech2MIDI + pitch, (c) the GaussianDiffusion around (a); and
    GaussianDiffusion builds FastSpeech2 when use_midi is absent."""
    from bisinger_amd.diffnet import DiffNet
    from bisinger_amd.diffusion import GaussianDiffusion
    from bisinger_amd.fs2 import FastSpeech2, FastSpeech2MIDI
    from bisinger_amd.hparams import hparams
    lst = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]
    m, _ = R.build('plain', 2, True)
    assert isinstance(m, FastSpeech2) and lst(m) == spec['popcs']['fs2'] and len(lst(m)) == 114
    m, _ = R.build('midi', 5, True)
    assert isinstance(m, FastSpeech2MIDI) and lst(m) == spec['bisinger']['fs2'] and len(lst(m)) == 168
    use_config()
    try:
        h = spec['popcs']['hparams']
        hparams.update({k: h[k] for k in ('use_pitch_embed', 'pitch_type', 'pitch_ar', 'pitch_norm', 'use_uv', 'use_spk_id', 'predictor_layers',
                                          'predictor_kernel', 'dur_predictor_layers', 'num_spk', 'dilation_cycle_length', 'timesteps', 'K_step')})
        hparams['rel_pos'] = False
        del hparams['use_midi']
        gd = GaussianDiffusion(R.PhoneEncoder(), 80, DiffNet(80), timesteps=100, K_step=51, loss_type='l1', spec_min=hparams['spec_min'],
                               spec_max=hparams['spec_max'])
        assert type(gd.fs2) is FastSpeech2
        assert lst(gd) == spec['popcs']['GaussianDiffusion'] and len(lst(gd)) == 298
    finally:
        use_config()


REFUSALS = [(dict(pitch_type='ph'), 'pitch_type'), (dict(pitch_type='cwt'), 'pitch_type'), (dict(pitch_ar=True), 'pitch_ar'),
            (dict(pitch_norm='standard'), 'pitch_norm'), (dict(use_energy_embed=True), 'use_energy_embed'),
            (dict(use_spk_embed=True, use_spk_id=False), 'use_spk_embed'), (dict(use_split_spk_id=True), 'use_split_spk_id'),
            (dict(encoder_type='conformer'), 'encoder_type'), (dict(decoder_type='conv'), 'decoder_type')]


# (rel_pos is the MIDI front's own encoder: refused together with the plain front only)
@pytest.mark.parametrize('front,over,key', [(f, o, k) for f in ('midi', 'plain') for o, k in REFUSALS] + [('plain', dict(rel_pos=True), 'rel_pos')],
                         ids=lambda v: v if isinstance(v, str) else '-'.join(map(str, v.values())))
def test_refusals_name_the_key(front, over, key):
    from bisinger_amd.fs2 import FastSpeech2, FastSpeech2MIDI
    from bisinger_amd.hparams import hparams
    use_config()
    try:
        if front == 'plain':
            hparams.update(R.POPCS_HP)
        hparams['use_pitch_embed'] = True
        hparams.update(over)
        with pytest.raises(NotImplementedError) as e:
            (FastSpeech2MIDI if front == 'midi' else FastSpeech2)(R.PhoneEncoder(), 80)
        assert str(e.value).startswith(key + ':'), str(e.value)
    finally:
        use_config()


def test_bin_function_hand_cases():
    f0 = torch.tensor([0.0, 30.0, 49.9, 50.0, 1100.0, 1500.0, float('inf'), 220.0], dtype=F64)
    mel, bins = R.f0_to_mel_bins(f0)
    assert bins.tolist()[:7] == [1, 1, 1, 1, 255, 255, 255]
    k = int(bins[7])
    assert abs(float(R.bin_centre_f0([k])[0]) - np.log2(220.0)) < np.log2(1.02)      # 220 Hz lies in the bin its centre names
    # a uv frame and a padded frame: f0_denorm 0 -> bin 1, whatever the supplied f0
    sd = formula_sd(json.load(open(os.path.join(GOLD, 'fs2_pitch_spec.json')))['popcs']['fs2'])
    hp = dict(use_pitch_embed=True, use_uv=True, predictor_layers=2, predictor_kernel=5)
    enc = torch.randn(1, 2, 256, generator=torch.Generator().manual_seed(0))
    r = R.frame_part(sd, 'fs2.', enc, torch.tensor([[1, 2, 0]]), None, None, hp, F64, f0=torch.full((1, 3), 8.0), uv=torch.tensor([[0.0, 1.0, 0.0]]))
    assert r['f0_denorm'].tolist() == [[256.0, 0.0, 0.0]] and r['pitch_bin'][0, 1:].tolist() == [1, 1] and int(r['pitch_bin'][0, 0]) > 1
    assert bool((r['decoder_inp'][0, 2] == 0).all())
    # bin centres invert the bin formula exactly
    ks = np.arange(2, 255)
    mel, bins = R.f0_to_mel_bins(2 ** torch.from_numpy(R.bin_centre_f0(ks)).double())
    assert bins.tolist() == ks.tolist() and float((mel - torch.from_numpy(ks)).abs().max()) < 1e-3


def _small_frame_cases():
    return [c for c in R.frame_cases() if c[5] <= 129]


def test_bounds_cover_the_float32_restatement_and_pitch_is_visible():
    """Every float32 figure <= bound / 4 over the frame cases up to 129 frames and the 2 x 12 x 64 end-to-end inputs; predicted f0 of the
    visible weights covers >= 20 distinct bins strictly between 1 and 255 with voiced and unvoiced frames each >= 10 % of the real frames."""
    mods = {}
    worst = dict.fromkeys(R.BOUND, 0.0)
    for case in _small_frame_cases():
        front, depth, use_uv, mode, B, T, lens = case
        if (front, depth, use_uv) not in mods:
            m, hp = R.build(front, depth, use_uv)
            mods[front, depth, use_uv] = (cpu_sd(m, 'fs2.'), hp)
        sd, hp = mods[front, depth, use_uv]
        inp = R.frame_inputs(B, max(1, min(12, T // 3 + 1)), T, lens)
        r32, r64 = R.frame_reference(sd, hp, inp, mode, F32), R.frame_reference(sd, hp, inp, mode, F64)
        for k in ('pitch_pred', 'decoder_inp'):
            worst[k] = max(worst[k], nerr(r32[k], r64[k].numpy()))
        worst['f0_denorm'] = max(worst['f0_denorm'], float(((r32['f0_denorm'].double() - r64['f0_denorm']).abs() / r64['f0_denorm'].clamp(min=1)).max()))
    for front, depth in (('plain', 2), ('midi', 5)):
        m, hp = R.build(front, depth, True)
        sd = cpu_sd(m, 'fs2.')
        inp = {k: torch.from_numpy(v) for k, v in synth.synth_inputs(2, 12, 64, seed=1, ragged=True).items()}
        r32, r64 = R.forward(sd, inp, hp, dtype=F32), R.forward(sd, inp, hp, dtype=F64)
        for k in ('pitch_pred', 'decoder_inp', 'enc_out', 'mel_out'):
            worst[k] = max(worst[k], nerr(r32[k], r64[k].numpy()))
        real = inp['mel2ph'] > 0
        bins = set(r64['pitch_bin'][real].tolist()) - {1, 255}
        unv = float((r64['f0_denorm'][real] == 0).double().mean())
        print(front, 'distinct bins', len(bins), 'unvoiced', unv)
        assert len(bins) >= 20 and 0.1 <= unv <= 0.9
    print({k: f'{v:.2e}' for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= R.BOUND[k] / 4 * 1.0000001, (k, v, R.BOUND[k] / 4)


def test_near_tie_census():
    """Near ties of the float64 restatement stay under 2 % of the real frames in every GPU case with predicted f0 or uv."""
    mods = {}
    for case in R.frame_cases():
        front, depth, use_uv, mode, B, T, lens = case
        if mode == 'f0uv' or T > 129 and mode != 'pred':
            continue
        if (front, depth, use_uv) not in mods:
            m, hp = R.build(front, depth, use_uv)
            mods[front, depth, use_uv] = (cpu_sd(m, 'fs2.'), hp)
        sd, hp = mods[front, depth, use_uv]
        inp = R.frame_inputs(B, max(1, min(12, T // 3 + 1)), T, lens)
        r64 = R.frame_reference(sd, hp, inp, mode, F64)
        real = torch.from_numpy(inp['mel2ph']) > 0
        tie, uv_tie = R.near_ties(r64)
        loose = ((tie if mode == 'pred' else torch.zeros_like(real)) | (uv_tie if use_uv else torch.zeros_like(real))) & real
        assert int(loose.sum()) <= 0.02 * int(real.sum()), (case, int(loose.sum()), int(real.sum()))


def test_create_refuses_bad_configurations_before_any_device_call():
    """bsg_fs2_create / bsg_fs2_n_weights: BSG_EINVAL and a message naming the field — checked here without a GPU."""
    from ctypes import POINTER, byref, c_void_p, cast
    from bisinger_amd import _lib
    lib = _lib.load()
    base = _lib.Fs2Cfg(256, 65, 4, 4, 2, 9, 9, 80, 2, 3, 0, 8, 2002, 2002)
    good = _lib.Fs2XCfg(base, _lib.FS2_FRONT_PLAIN, 1, 2, 5, 1, 2002)
    assert lib.bsg_fs2_n_weights(byref(good)) == 114
    midi = _lib.Fs2Cfg(256, 65, 4, 4, 2, 9, 9, 80, 5, 3, 22, 8, 5002, 5000)
    assert lib.bsg_fs2_n_weights(byref(_lib.Fs2XCfg(midi, _lib.FS2_FRONT_MIDI, 1, 5, 5, 1, 5002))) == 168
    assert lib.bsg_fs2_n_weights(byref(_lib.Fs2XCfg(midi, _lib.FS2_FRONT_MIDI, 0, 0, 0, 0, 0))) == 143 == lib.bsg_fs2midi_n_weights(byref(midi))

    def refused(cfg, n, *words):
        dummy = (c_void_p * 400)(*([1] * 400))
        h = c_void_p()
        rc = lib.bsg_fs2_create(byref(h), byref(cfg), cast(dummy, POINTER(c_void_p)), n, c_void_p(1), c_void_p(1), c_void_p(1), None)
        msg = lib.bsg_last_error().decode()
        assert rc == -22 and h.value is None and all(w in msg for w in words), (rc, msg)

    refused(_lib.Fs2XCfg(base, 2, 0, 0, 0, 0, 0), 114, 'front=2')
    refused(_lib.Fs2XCfg(base, _lib.FS2_FRONT_MIDI, 1, 2, 5, 1, 2002), 114, 'spk_rows=0')
    refused(_lib.Fs2XCfg(base, _lib.FS2_FRONT_PLAIN, 1, 2, 4, 1, 2002), 114, 'pitch_kernel=4')
    refused(_lib.Fs2XCfg(base, _lib.FS2_FRONT_PLAIN, 1, 0, 5, 1, 2002), 114, 'pitch_layers=0')
    refused(_lib.Fs2XCfg(base, _lib.FS2_FRONT_PLAIN, 1, 2, 5, 2, 2002), 114, 'use_uv=2')
    refused(_lib.Fs2XCfg(base, _lib.FS2_FRONT_PLAIN, 1, 2, 5, 1, 1), 114, 'n_pitch_pos=1')
    refused(good, 113, '114', '113')
    bad_h = _lib.Fs2Cfg(192, 65, 4, 4, 2, 9, 9, 80, 2, 3, 0, 8, 2002, 2002)
    refused(_lib.Fs2XCfg(bad_h, _lib.FS2_FRONT_PLAIN, 0, 0, 0, 0, 0), 100, '192', '256')
