"""Ragged batches through the FFT denoiser (diff_decoder_type: fft) against padding: real mel-frames/s and ms per sampler step of
GaussianDiffusion.sample (DDPM, Philox noise) on one request list, two ways —
  padded   the batch padded to its longest row: the Python step loop (bsg_fftden_forward + bsg_ddpm_step per step);
  ragged   every row at its own length (lengths=...): ONE call of bsg_fftden_ddpm_sample, the fused step tail.
Launches per step outside the FFT stack (the stack's own launches are the same both ways), READ FROM THE CODE, not counted by the run:
padded 11 (the torch.full of the step tensor, transpose, input projection, step gather, step GEMM, concat-Linear GEMM, positions, entry,
get_mel_out, transpose, bsg_ddpm_step), ragged 6 (transpose, input projection, concat-Linear GEMM, positions, entry, the fused tail).
The two modes are timed in alternation, one sample() call of --steps steps per pass and mode, each pass closed by a device
synchronisation; the line gives the median pass of each mode with its smallest and largest.  The difference mixes three things: fewer
frames, the loop in the library instead of Python, and the fused tail.  Nothing gates on these numbers.  Prints one JSON line:
  B = 16, T_max = 1000, lengths RandomState(0).randint(250, 1001) with the first row at 1000

    python tools/bench_fftden_ragged.py [--steps K] [--passes N] [--warmup W]      (defaults: 100 steps, 9 passes, 2 warm-up passes)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100, help='sampler steps per pass (of the 100-step schedule)')
    ap.add_argument('--passes', type=int, default=9, help='timed passes per mode')
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bisinger_amd.hparams import hparams
    from tests import fftden_ragged_cases as RC
    from tests.util import use_config
    from bisinger_amd.diffusion import GaussianDiffusion
    torch.set_grad_enabled(False)

    class Enc:
        def __len__(self):
            return 65

        def pad(self):
            return 0

    net = RC.build_net()
    use_config('diff_decoder_type=fft')
    model = GaussianDiffusion(Enc(), 80, net, timesteps=100, K_step=100, spec_min=hparams['spec_min'], spec_max=hparams['spec_max']).cuda().eval()
    use_config()
    B, T = 16, 1000
    lens = [int(v) for v in np.random.RandomState(0).randint(250, T + 1, size=B)]
    lens[0] = T
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(B, 256, T, generator=g).cuda()
    x0 = torch.randn(B, 1, 80, T, generator=g).cuda()

    modes = (('padded', {}, 11), ('ragged', {'lengths': lens}, 6))
    times, paths = {name: [] for name, _, _ in modes}, {}
    for p in range(args.warmup + args.passes):
        for name, kw, _ in modes:      # alternated: a drift of the clock or of the machine falls on both modes alike
            x = x0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.sample(cond, x, seed=3, n_steps=args.steps, **kw)
            torch.cuda.synchronize()
            if p >= args.warmup:
                times[name].append(time.perf_counter() - t0)
            paths[name] = net.last_path()
    real = sum(lens)
    out = {'B': B, 'T_max': T, 'lengths': lens, 'real_frames': real, 'padded_frames': B * T, 'steps': args.steps, 'passes': args.passes}
    for name, _, outside in modes:
        ms = sorted(1e3 * t / args.steps for t in times[name])
        med = ms[len(ms) // 2]
        out[name] = {'ms_per_step_median': round(med, 4), 'ms_per_step_min': round(ms[0], 4), 'ms_per_step_max': round(ms[-1], 4),
                     'real_frames_per_s': round(real / (med * 1e-3), 1), 'launches_per_step_outside_the_stack_read_from_the_code': outside,
                     'path': paths[name]}
    out['speedup_of_medians'] = round(out['padded']['ms_per_step_median'] / out['ragged']['ms_per_step_median'], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
