#!/usr/bin/env python3
"""Goldens of the Parallel WaveGAN generator (`vocoder: pwg`) from the reference's own modules.  Build container only (needs the
reference checkout).  Records tests/golden/pwg_state_dict_spec.json (keys, shapes and order of the reference's state dict in the
weight-norm and the folded layout, with and without the pitch front) and writes tests/golden/pwg_plain.npz / pwg_pitch.npz: the
reference's output for formula weights (synth.synth_state_dict over the recorded spec) and formula inputs (tests/pwg_ref.make_inputs),
so that only the outputs are stored."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bisinger_amd import synth          # noqa: E402
from tests import pwg_ref               # noqa: E402
import ref_import                       # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
SEEDS, CASES = pwg_ref.GOLDEN_SEEDS, pwg_ref.GOLDEN_CASES
torch.set_grad_enabled(False)


def main():
    ref_import.import_reference()
    ref_import.import_hifigan()                          # the layers-package shim
    sys.modules['modules.parallel_wavegan.layers'].upsample = sys.modules['modules.parallel_wavegan.layers.upsample']
    from modules.parallel_wavegan.models.parallel_wavegan import ParallelWaveGANGenerator
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ref_import.REF, 'configs', 'tts', 'pwg.yaml')))
    spec_js = {'hop_size': int(cfg['hop_size']), 'generator_params': cfg['generator_params']}
    for form, pitch in (('plain', False), ('pitch', True)):
        gp = json.loads(json.dumps(cfg['generator_params']))
        gp['use_pitch_embed'] = pitch
        g = ParallelWaveGANGenerator(**gp)
        spec = OrderedDict((k, tuple(v.shape)) for k, v in g.state_dict().items())
        w = synth.synth_state_dict(spec, seed=SEEDS[form])
        g.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        g.remove_weight_norm()
        g.eval()
        folded = OrderedDict((k, v.clone()) for k, v in g.state_dict().items())
        spec_js[f'{form}_weight_norm'] = [[k, list(s)] for k, s in spec.items()]
        spec_js[f'{form}_folded'] = [[k, list(v.shape)] for k, v in folded.items()]
        spec_js[f'{form}_n_params'] = int(sum(v.numel() for v in folded.values()))
        spec_js['receptive_field_size'] = int(g.receptive_field_size)
        mine_sd = pwg_ref.fold({k: torch.from_numpy(v) for k, v in w.items()})
        assert list(mine_sd) == list(folded) and all(torch.equal(mine_sd[k], folded[k]) for k in folded), 'fold differs from remove_weight_norm'
        out = {}
        for tag, (B, T, seed) in CASES.items():
            z, c, p = pwg_ref.make_inputs(B, T, seed, gp['aux_context_window'], pitch)
            y = g(torch.from_numpy(z), torch.from_numpy(c), torch.from_numpy(p) if pitch else None).numpy()
            out[tag] = y
            q = pwg_ref.params(pitch)
            y32 = pwg_ref.forward(mine_sd, z, c, p, q, torch.float32)
            y64, big = pwg_ref.forward(mine_sd, z, c, p, q, torch.float64, return_max=True)
            print(f'{form} {tag}: restatement(float32) vs reference {np.abs(y32 - y).max():.3e}; reference vs float64 {np.abs(y - y64).max():.3e}; '
                  f'max |y| {np.abs(y).max():.3f}; largest intermediate {big:.1f}')
        path = os.path.join(GOLD, f'pwg_{form}.npz')
        np.savez_compressed(path, **out)
        print(f'{form}: {len(spec)} entries weight-norm, {len(folded)} folded, {spec_js[f"{form}_n_params"]} parameters, '
              f'receptive field {g.receptive_field_size}; {path} {os.path.getsize(path) / 1024:.1f} KB')
    json.dump(spec_js, open(os.path.join(GOLD, 'pwg_state_dict_spec.json'), 'w'), separators=(',', ':'))


if __name__ == '__main__':
    main()
