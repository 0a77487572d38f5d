"""The pitch extractor of the parity tests and the cases of tests/test_gpu_pe_shapes.py, shared with tests/test_gpu_f2_fullsize.py (the
same weights at production length) and tests/test_pe_cases_cpu.py (the float64 oracle alone decides every frame of the short cases).
No GPU is needed to import this module."""
from collections import OrderedDict

import numpy as np
import torch

from bisinger_amd import synth
from oracle import pe as ope
from tests.util import use_config

SHAPE_T = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)
SHAPE_B = (1, 3)
# seed of mel_for(B, T) for the cases whose first seed, 100 * B + T, leaves a frame's voicing logit near 0 in the float64 oracle or no
# voiced frame at all (tests/test_pe_cases_cpu.py: at T <= 5 one frame is more than the 10 % that _check_pitch may set aside)
SEEDS = {(1, 1): 38, (3, 1): 4}


def pitch_extractor(sd_spec):
    """PitchExtractor (on the CPU: .cuda() it) on formula weights of seed 11 with tests/test_gpu_f2.py's running statistics."""
    hp = use_config()
    hp.update(pitch_type='frame', use_uv=True, pitch_norm='log')
    from bisinger_amd.pe import PitchExtractor
    pe = PitchExtractor()
    spec = OrderedDict((k, tuple(s)) for k, s in sd_spec['PitchExtractor'])
    w = synth.synth_state_dict(spec, seed=11)
    for k in spec:
        if k.endswith('running_var'):
            w[k] = (0.5 + np.abs(w[k]) * 5).astype(np.float32)
        if k.endswith('running_mean'):
            w[k] = (w[k] * 3).astype(np.float32)
    pe.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return pe


def cpu_state_dict(pe):
    return {k: v.detach().cpu() for k, v in pe.state_dict().items()}


def mel(rs, B, T, lens):
    """[B, T, 80] float32 mel-like frames, exactly 0 from frame lens[b] on."""
    m = (rs.standard_normal((B, T, 80)) * 1.5 - 3.0).astype(np.float32)
    for b, n in enumerate(lens):
        m[b, n:] = 0
    return m


def mel_for(B, T):
    """The input of shape case (B, T): every row at full length."""
    return mel(np.random.RandomState(SEEDS.get((B, T), 100 * B + T)), B, T, [T] * B)


def oracle_margin(sd, m):
    """What tests/test_gpu_f2_fullsize.py _check_pitch derives from the oracle alone: (bar of pitch_pred, |voicing logit| of every frame in
    the float64 oracle, its f0)."""
    want = ope.pitch_extractor_forward(sd, torch.from_numpy(m), dtype=torch.float64)
    w32 = ope.pitch_extractor_forward(sd, torch.from_numpy(m), dtype=torch.float32)
    pp64 = want['pitch_pred'].numpy()
    dev32 = float(np.abs(w32['pitch_pred'].double().numpy() - pp64).max())
    bar = 2 * dev32 + 2e-5 * max(1.0, float(np.abs(pp64).max()))
    return bar, np.abs(pp64[..., 1]), want['f0_denorm_pred'].numpy()
