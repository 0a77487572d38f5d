#!/usr/bin/env python3
"""Record bsg_fs2midi_last_path / bsg_fftden_last_path of the loaded library (BSG_LIB, else the tree's build) as tests/golden/fs2_paths.json.

Run it against the build of the commit whose launch choices are the reference (the parent of a refactor of csrc/fs2.hip):

    BSG_LIB=<parent build>/libbisinger_hip.so python tools/make_golden_fs2_paths.py --commit <parent commit id>

Three sets of cases (tests/test_gpu_fs2_paths.py and tests/test_gpu_fs2_shapes.py assert string equality against them):
  default  FastSpeech2MIDI with the formula weights of tests/test_gpu_fs2_shapes.py, default switches, over GRID of
           tests/test_gpu_fs2_paths.py in one process; each case is an encode followed by the forward
  forms    the switch sets of FORMS in tests/test_gpu_fs2_shapes.py at its SHORT_LIST (and NW4 where the set runs it), one child process per set
  den      the FFT denoiser of that file at its DEN_SHAPES
The strings depend on the shapes and the constants of csrc/fs2.hip only, not on the box.  --outs DIR also stores every output (enc_out,
decoder_inp, mel_out; the denoiser's eps) as <set>.<case>.<output>.npy, from seeded inputs, so that two builds can be compared bit for bit:
--compare DIR_A DIR_B does that and exits non-zero on a difference.
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
from bisinger_amd import _lib, synth  # noqa: E402
from tests import test_gpu_fs2_shapes as S  # noqa: E402
from tests.test_gpu_fs2_paths import GRID, key  # noqa: E402

torch.set_grad_enabled(False)


def _keep(outs, tag, name, arrays):
    if outs:
        for k, v in arrays.items():
            np.save(os.path.join(outs, f'{tag}.{name}.{k}.npy'.replace(' ', '_')), v)


def default_paths(outs):
    m = S._make_fs2()
    out = {}
    for B, Tt, T in sorted(GRID, key=lambda c: -c[0] * c[2]):      # largest first: the workspaces grow once
        got, path = S._run(m, synth.synth_inputs(B, Tt, T, seed=5))
        out[key(B, Tt, T)] = path
        _keep(outs, 'default', key(B, Tt, T), got)
    return OrderedDict((key(*c), out[key(*c)]) for c in GRID)


def form_paths(outs, name):
    m = S._make_fs2()
    out = OrderedDict()
    for case in S.SHORT_LIST + ([S.NW4] if S.FORMS[name][2] else []):
        got, path = S._run(m, S._inputs(case), case[4])
        out[S._name(case)] = path
        _keep(outs, name, S._name(case), got)
    return out


def den_paths(outs):
    from bisinger_amd.diffnet import DIFF_DECODERS
    from bisinger_amd.hparams import hparams
    with open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_spec.json')) as f:
        spec = OrderedDict((k, tuple(s)) for k, s in json.load(f)['FFT'])
    S.use_config('diff_decoder_type=fft')      # the denoiser of the `den` fixture
    net = DIFF_DECODERS[hparams['diff_decoder_type']](hparams)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, seed=17).items()}, strict=False)
    S.use_config()
    net = net.cuda()
    out = OrderedDict()
    for B, T in S.DEN_SHAPES:
        eps, path = S._den_run(net, B, T)
        out[f'{B}x{T}'] = path
        _keep(outs, 'den', f'{B}x{T}', {'eps': eps})
    return out


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    other = sorted(f for f in os.listdir(b) if f.endswith('.npy'))
    differ = [f for f in names if f not in other or not np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f)), equal_nan=True)]
    differ += [f for f in other if f not in names]
    print(json.dumps({'arrays_compared': len(names), 'differ': differ}))
    return 1 if differ or not names else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--commit', default='unknown', help='commit id of the library that is recorded')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'fs2_paths.json'))
    ap.add_argument('--outs', default=None, help='directory for the outputs of every case of the three sets')
    ap.add_argument('--compare', nargs=2, metavar='DIR', default=None, help='compare two --outs directories bit for bit; nothing is run')
    ap.add_argument('--child', default=None, help='internal: one switch set of FORMS (the switches are in the environment); prints its paths')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.outs:
        os.makedirs(a.outs, exist_ok=True)
    if a.child:
        print(json.dumps(form_paths(a.outs, a.child)))
        return
    rec = OrderedDict(parent_commit=a.commit, parent_build_sha256=hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest())
    rec['default'] = default_paths(a.outs)
    rec['forms'] = OrderedDict()
    for name, (env, *_rest) in S.FORMS.items():      # one after another: one child with the device open at a time
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name] + (['--outs', a.outs] if a.outs else []),
                             env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            sys.exit(f'{name}: child failed ({res.returncode})\n{res.stderr[-2000:]}')
        rec['forms'][name] = json.loads(res.stdout.strip().splitlines()[-1])
    rec['den'] = den_paths(a.outs)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=0)
        f.write('\n')
    print(f"{a.out}: {len(rec['default'])} default, {sum(len(v) for v in rec['forms'].values())} form, {len(rec['den'])} denoiser cases")


if __name__ == '__main__':
    main()
