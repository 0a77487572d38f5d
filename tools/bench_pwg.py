#!/usr/bin/env python3
"""The Parallel WaveGAN generator alone (csrc/pwg.hip) at B = 1 and B = 8 rows of T = 1000 mel frames (256 000 samples, 11.6 s of audio
at 22 050 Hz per row), formula weights; beside it, in the same process on the same GPU: the float32 torch restatement of the same forward
(tests/pwg_ref.py) moved to the device — what a user would otherwise run — with its inputs, weights and result resident on the device (no copy
to the host, no wait inside the timed region) and the whole batch in one call, exactly as the HIP path is timed.  HIP events on the stream; 1 warm-up, then WINDOWS windows of
`reps` forwards: median and spread.  One JSON line; `ratio` = HIP / torch must be below 1: the script exits with status 1 otherwise.  The floors per layer: bytes 1.3 KB per sample
(x read 256 B, c read 320 B, skip read and written 512 B, x written 256 B) at 8 TB/s, products 86 016 FLOP per sample at 157.3 TFLOP/s
(the fp32 matrix pipe).  `--out FILE` also writes the line to FILE."""
import json
import os
import statistics
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bisinger_amd import _lib, synth  # noqa: E402
from bisinger_amd.pwg import ParallelWaveGANGenerator  # noqa: E402
from tests import pwg_ref  # noqa: E402

WINDOWS, T, SR = 5, 1000, 22050
HBM_BPS, F32_FLOPS = 8.0e12, 157.3e12
BYTES_PER_SAMPLE_LAYER, FLOP_PER_SAMPLE_LAYER = 4 * (64 + 80 + 2 * 64 + 64), 2 * 128 * (3 * 64 + 80) + 2 * 128 * 64
torch.set_grad_enabled(False)
assert torch.cuda.is_available(), 'bench_pwg needs a GPU: there is no CPU path to time'
dev = torch.device('cuda', 0)


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {'ms': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3), 'reps': reps}


spec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pwg_state_dict_spec.json')))
w = synth.synth_state_dict(OrderedDict((k, tuple(s)) for k, s in spec['plain_weight_norm']), 21)
gp = json.loads(json.dumps(spec['generator_params']))
gen = ParallelWaveGANGenerator(**gp)
gen.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
gen = gen.eval().to(dev)
gen.remove_weight_norm()
folded = {k: v.detach() for k, v in gen.state_dict().items()}
q = pwg_ref.params(False)
res = {'T': T, 'samples_per_row': T * 256, 'audio_s_per_row': round(T * 256 / SR, 2), 'windows': WINDOWS, 'device': torch.cuda.get_device_name(0)}
for B in (1, 8):
    z, c, _ = pwg_ref.make_inputs(B, T, 7)
    z, c = torch.from_numpy(z).to(dev), torch.from_numpy(c).to(dev)
    hip = events_ms(lambda: gen(z, c), 10 if B == 1 else 3)
    y = gen(z, c)
    eager = lambda: pwg_ref.forward(folded, z, c, None, q, torch.float32, device=dev, as_tensor=True, whole_batch=True)
    yt = eager()
    tor = events_ms(eager, 3 if B == 1 else 1)
    n = B * T * 256
    res[f'B{B}'] = {
        'hip': hip, 'torch_f32_on_device': tor, 'ratio': round(hip['ms'] / tor['ms'], 4),
        'rtf': round(hip['ms'] * 1e-3 / (n / SR), 6), 'audio_s_per_s': round((n / SR) / (hip['ms'] * 1e-3), 1),
        'per_layer_ms_upper': round(hip['ms'] / 30, 4),      # the whole forward / 30: the front, first convolution and tail are inside
        'per_layer_hbm_floor_ms': round(n * BYTES_PER_SAMPLE_LAYER / HBM_BPS * 1e3, 4),
        'per_layer_f32_pipe_floor_ms': round(n * FLOP_PER_SAMPLE_LAYER / F32_FLOPS * 1e3, 4),
        'tflops': round(30 * n * FLOP_PER_SAMPLE_LAYER / (hip['ms'] * 1e-3) / 1e12, 1),
        'max_abs_hip_vs_torch': float((y - yt).abs().max()), 'path_layers': gen.last_path().count('layer')}
torch.cuda.synchronize()
gen.release()
line = json.dumps(res)
print(line)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
        f.write(line + '\n')
slow = [k for k in ('B1', 'B8') if not res[k]['ratio'] < 1]
if slow:
    sys.exit(f'bench_pwg: the HIP path is not faster than the torch restatement at {slow}')
