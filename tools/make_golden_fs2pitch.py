#!/usr/bin/env python3
"""Goldens of the pitch adaptor and the plain FastSpeech2 front from the REFERENCE's own modules (build machine only: needs the reference
checkout that tools/ref_import.py names).

    python tools/make_golden_fs2pitch.py        # writes tests/golden/fs2_pitch_spec.json and tests/golden/fs2_pitch.npz

Two chains, each in a process of its own (the reference's hparams are one global table, and modules capture defaults at import):
  popcs     usr/configs/popcs_ds_beta6.yaml: plain FastSpeech2 + pitch (a) inside GaussianDiffusion, K_step = 51 of 100 (c)
  bisinger  usr/configs/lang-esm-style-ori-shift/diff.yaml with use_pitch_embed=True: FastSpeech2MIDI + pitch (b)
Weights are formula weights (synth.synth_state_dict over the recorded spec, then fs2_pitch_ref.make_pitch_visible), inputs are formula
inputs (synth.synth_inputs(2, 12, 64, seed=1, ragged=True); f0 / uv of GOLD_F0 below), so only OUTPUTS are stored, and the hyper-parameter
values the tests need are recorded as JSON data.  No program text of the reference is copied.
"""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bisinger_amd import synth          # noqa: E402
from tests import fs2_pitch_ref as R    # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
HP_KEYS = ('use_midi', 'use_pitch_embed', 'pitch_type', 'pitch_ar', 'pitch_norm', 'use_uv', 'use_spk_id', 'use_spk_embed', 'use_split_spk_id',
           'use_energy_embed', 'rel_pos', 'predictor_layers', 'predictor_kernel', 'predictor_hidden', 'dur_predictor_layers',
           'dur_predictor_kernel', 'hidden_size', 'enc_layers', 'dec_layers', 'num_heads', 'enc_ffn_kernel_size', 'dec_ffn_kernel_size',
           'num_spk', 'K_step', 'timesteps', 'max_beta', 'dilation_cycle_length', 'residual_layers', 'residual_channels', 'audio_num_mel_bins',
           'encoder_type', 'decoder_type', 'ffn_padding', 'use_pos_embed', 'schedule_type', 'gaussian_start', 'pndm_speedup', 'diff_decoder_type',
           'spec_min', 'spec_max', 'keep_bins')
torch.set_grad_enabled(False)


def gold_inputs():
    inp = synth.synth_inputs(2, 12, 64, seed=1, ragged=True)
    rs = np.random.RandomState(64)
    inp['f0'] = R.bin_centre_f0(rs.randint(2, 255, size=(2, 64)))
    inp['uv'] = (rs.uniform(size=(2, 64)) < 0.2).astype(np.float32)
    return inp


def load(model, prefix_fs2='fs2.'):
    spec = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
    w = synth.synth_state_dict(spec, 0, synth.DIFFNET_GAIN)
    R.make_pitch_visible(w, prefix_fs2)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and all(synth.is_computed_buffer(k) for k in missing), (missing, unexpected)
    return spec


def fs2_cases(fs2, inp, midi, out, tag):
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    kw = {k: t[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')} if midi else {}
    spk = t['spk_embed'] if midi else None
    keep = ('pitch_pred', 'f0_denorm', 'decoder_inp', 'mel_out', 'mel2ph')
    runs = {'pred': dict(mel2ph=t['mel2ph']), 'given': dict(mel2ph=t['mel2ph'], f0=t['f0'].clone(), uv=t['uv'].clone())}
    if not midi:
        runs['dur'] = {}
    for name, a in runs.items():
        r = fs2(t['txt_tokens'], spk_embed=spk, infer=True, **a, **kw)
        for k in keep:
            out[f'{tag}.{name}.{k}'] = r[k].numpy()
        if name == 'dur':
            out[f'{tag}.{name}.dur'] = r['dur'].numpy()
    f0 = t['f0'].clone()
    fs2(t['txt_tokens'], spk_embed=spk, infer=True, mel2ph=t['mel2ph'], f0=f0, uv=t['uv'].clone(), **kw)
    out[f'{tag}.ref_writes_f0'] = np.asarray(not torch.equal(f0, t['f0']))


def chain(name, path):
    import ref_import
    if name == 'popcs':
        import types
        sys.dont_write_bytecode = True
        sys.path.insert(0, ref_import.REF)
        os.chdir(ref_import.REF)
        for n in ('librosa', 'pycwt'):
            sys.modules.setdefault(n, types.ModuleType(n))
        sys.modules['pycwt'].wavelet = types.SimpleNamespace()
        from utils.hparams import hparams, set_hparams
        set_hparams(config='usr/configs/popcs_ds_beta6.yaml', print_hparams=False)      # (this chain has no pndm_speedup key to override)
        from utils.text_encoder import TokenTextEncoder
        from usr.diff.net import DiffNet
        import usr.diff.shallow_diffusion_tts as sdt
        sdt.tqdm = lambda it, **kw: it
        enc = TokenTextEncoder(None, vocab_list=['<AP>', '<SP>'] + [f'p{i}' for i in range(60)], replace_oov=',')
        GD = sdt.GaussianDiffusion
    else:
        Rf = ref_import.import_reference('timesteps=100,K_step=100,max_beta=0.06,pndm_speedup=0,use_pitch_embed=True')
        hparams, sdt, enc, DiffNet, GD = Rf['hparams'], Rf['sdt'], Rf['phone_encoder'], Rf['DiffNet'], Rf['GaussianDiffusion']
    T, K = int(hparams['timesteps']), int(hparams['K_step'])
    betas = sdt.linear_beta_schedule(T, max_beta=hparams['max_beta'])
    model = GD(enc, 80, DiffNet(80), timesteps=T, K_step=K, loss_type='l1', betas=betas, spec_min=hparams['spec_min'],
               spec_max=hparams['spec_max']).eval()
    spec = load(model)
    out = {}
    inp = gold_inputs()
    fs2_cases(model.fs2, inp, name != 'popcs', out, name)
    if name == 'popcs':
        from make_golden import SuppliedNoise
        noise = synth.synth_noise(K, 2, 80, 64, seed=3)
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        with SuppliedNoise(sdt, noise):
            r = model(t['txt_tokens'], mel2ph=t['mel2ph'], f0=t['f0'].clone(), uv=t['uv'].clone(), infer=True)
        for k in ('mel_out', 'fs2_mel', 'f0_denorm', 'pitch_pred'):
            out[f'popcs.gd.{k}'] = r[k].numpy()
    js = dict(model=type(model.fs2).__name__, hparams={k: hparams.get(k) for k in HP_KEYS},
              GaussianDiffusion=[[k, list(s)] for k, s in spec.items()],
              fs2=[[k[4:], list(s)] for k, s in spec.items() if k.startswith('fs2.')])
    np.savez_compressed(path + '.npz', **out)
    with open(path + '.json', 'w') as f:
        json.dump(js, f)


def main():
    if len(sys.argv) == 3:
        return chain(sys.argv[1], sys.argv[2])
    import tempfile
    tmp = tempfile.mkdtemp()
    spec, arrs = {}, {}
    for name in ('popcs', 'bisinger'):
        path = os.path.join(tmp, name)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), name, path], cwd=ROOT)
        spec[name] = json.load(open(path + '.json'))
        arrs.update(np.load(path + '.npz'))
    with open(os.path.join(GOLD, 'fs2_pitch_spec.json'), 'w') as f:
        json.dump(spec, f, indent=0, sort_keys=True)
    # a fixed archive (stored, no timestamps beyond the zip default epoch of numpy): regenerates bit-identically
    np.savez(os.path.join(GOLD, 'fs2_pitch.npz'), **{k: arrs[k] for k in sorted(arrs)})
    for n in ('fs2_pitch_spec.json', 'fs2_pitch.npz'):
        print(f'wrote tests/golden/{n} ({os.path.getsize(os.path.join(GOLD, n)) / 1024:.1f} KB)')
    print({k: (v['model'], len(v['fs2']), len(v['GaussianDiffusion'])) for k, v in spec.items()})


if __name__ == '__main__':
    main()
