#!/usr/bin/env python3
"""Record bsg_hifigan_last_path of the loaded library (BSG_LIB, else the tree's build) as tests/golden/hifigan_paths.json.

Run it against the build of the commit whose launch choices are the reference (the parent of a refactor of csrc/hifigan.hip):

    BSG_LIB=<parent build>/libbisinger_hip.so python tools/make_golden_hifigan_paths.py --commit <parent commit id>

Three sets of cases (tests/test_gpu_hifigan_paths.py and tests/test_gpu_hifigan_shapes.py assert string equality against them):
  plain  the plain generator as bench.build_vocoder builds it, default switches, over GRID of tests/test_gpu_hifigan_paths.py
  forms  the switch sets of FORMS in tests/test_gpu_hifigan_shapes.py at its SHORT_LIST, one child process per set
  nsf, rb2  the NSF and the ResBlock2 generators of that file at its OTHER_SHAPES
The strings depend on the shapes and the constants of csrc/hifigan.hip only, not on the box.  --waves DIR also stores every waveform
(<set>.<B>x<T>.npy, from seeded inputs) so that two builds can be compared bit for bit.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bisinger_amd import _lib, synth  # noqa: E402
from tests.test_gpu_hifigan_paths import GRID  # noqa: E402
from tests.test_gpu_hifigan_shapes import FORMS, HOP, NH, OTHER_SHAPES, SHORT_LIST, _f0, _mel  # noqa: E402

torch.set_grad_enabled(False)


def _keep(waves, tag, B, T, y):
    if waves:
        np.save(os.path.join(waves, f'{tag}.{B}x{T}.npy'), y.cpu().numpy())


def plain_paths(shapes, waves, tag):
    voc, _ = bench.build_vocoder(torch.device('cuda', 0))
    out = OrderedDict()
    for B, T in sorted(shapes, key=lambda s: -s[0] * s[1]):      # largest first: the stage buffers grow once
        y = voc(torch.from_numpy(_mel(B, T)).cuda())
        out[f'{B}x{T}'] = voc.last_path()
        if B * T >= 999 or tag != 'plain':
            _keep(waves, tag, B, T, y)
    return OrderedDict((f'{B}x{T}', out[f'{B}x{T}']) for B, T in shapes)


def other_paths(waves):
    import yaml
    from bisinger_amd.hifigan import HifiGanGenerator
    spec_js = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_spec.json')))

    def gen(cfg, key, seed):
        spec = OrderedDict((k, tuple(s)) for k, s in spec_js[key])
        g = HifiGanGenerator(cfg)
        g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed).items()}, strict=True)
        g = g.cuda()
        g.remove_weight_norm()
        return g

    cfg = yaml.safe_load(open(os.path.join(ROOT, 'bisinger_amd', 'configs', 'hifigan.yaml')))
    cfg['use_pitch_embed'] = True
    nsf, rb2 = gen(cfg, 'HifiGanGenerator_nsf_weight_norm', 13), gen(spec_js['hifigan_rb2_cfg'], 'HifiGanGenerator_rb2_weight_norm', 27)
    out = {'nsf': OrderedDict(), 'rb2': OrderedDict()}
    for B, T in OTHER_SHAPES:      # the inputs of test_nsf_generator_vs_fp64 / test_resblock2_generator_vs_fp64
        rs = np.random.RandomState(500 * B + T)
        mel = (rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
        f0 = _f0(rs, B, T)
        rand_ini = rs.uniform(0, 1, size=(B, NH)).astype(np.float32)
        noise = rs.standard_normal((B, T * HOP, NH)).astype(np.float32)
        y = nsf(torch.from_numpy(mel).cuda(), torch.from_numpy(f0).cuda(), rand_ini=torch.from_numpy(rand_ini), noise=torch.from_numpy(noise))
        out['nsf'][f'{B}x{T}'] = nsf.last_path()
        _keep(waves, 'nsf', B, T, y)
        mel = (np.random.RandomState(700 * B + T).standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
        y = rb2(torch.from_numpy(mel).cuda())
        out['rb2'][f'{B}x{T}'] = rb2.last_path()
        _keep(waves, 'rb2', B, T, y)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--commit', default='unknown', help='commit id of the library that is recorded')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'hifigan_paths.json'))
    ap.add_argument('--waves', default=None, help='directory for the waveforms of every case with B T >= 999, of the forms and of the other generators')
    ap.add_argument('--child', default=None, help='internal: one switch set of FORMS (the switches are in the environment); prints its paths')
    a = ap.parse_args()
    if a.waves:
        os.makedirs(a.waves, exist_ok=True)
    if a.child:
        print(json.dumps(plain_paths(SHORT_LIST, a.waves, a.child)))
        return
    rec = OrderedDict(parent_commit=a.commit, parent_build_sha256=hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest())
    rec['plain'] = plain_paths(GRID, a.waves, 'plain')
    rec['forms'] = OrderedDict()
    for name, (env, *_checks) in FORMS.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name] + (['--waves', a.waves] if a.waves else []),
                             env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            sys.exit(f'{name}: child failed ({res.returncode})\n{res.stderr[-2000:]}')
        rec['forms'][name] = json.loads(res.stdout.strip().splitlines()[-1])
    rec.update(other_paths(a.waves))
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=0)
        f.write('\n')
    print(f"{a.out}: {len(rec['plain'])} plain, {sum(len(v) for v in rec['forms'].values())} form, {len(rec['nsf']) + len(rec['rb2'])} other cases")


if __name__ == '__main__':
    main()
